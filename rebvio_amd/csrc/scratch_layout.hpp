// Scratch of the on-demand entries: each feature's device scratch is ONE allocation of the context, made at the
// feature's first call and kept; its views are stated here, once. A layout's lay(base, ...) hands the pieces to a Carve in the order
// they lie in memory and returns the bytes they take: with a null base it only measures, with the allocation's address it sets the
// views - so the size asked for and the views cut from it cannot disagree. No HIP in this file: tests/cpp/scratch_layout_check.cpp
// lays every scratch out over host memory. Types this file cannot name (they need the HIP headers) are template parameters.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "edge_chains.hpp"    // ech::ChainNode
#include "edge_segments.hpp"  // esg::SegPoint, esg::SegSpan
#include "kf_handover.hpp"    // kfp::HandoverStage; kfp::kSums (kf_pose.hpp)
#include "place.hpp"          // plc::kWords
#include "rebvio_hip.h"

namespace rh {
namespace scratch {
// A cursor over one allocation. A view's offset is exactly the bytes taken in front of it: nothing is aligned unless align() is
// called (the layouts below are the ones the kernels and the copies were written against).
class Carve {
 public:
  explicit Carve(char* base) : base_(base) {}
  template <class T>
  T* take(size_t count) {
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += count * sizeof(T);
    return p;
  }
  void align(size_t a) { off_ = (off_ + a - 1) / a * a; }
  size_t size() const { return off_; }

 private:
  char* base_;
  size_t off_ = 0;
};

inline size_t slots256(size_t kmax) { return (kmax + 255) / 256 * 256; }

struct Layout {
  char* base = nullptr;  // the allocation; null until the feature's first call
};

// rebvio_hip_map_keyframe_matches (and _pose, which runs it): the slot table - ceil(kmax / 256) * 256 winner keys, as many claimant
// counts, then `blocks` block counts and the record count. The kmax records (rec) are a second allocation of their own.
struct KfMatches : Layout {
  unsigned long long* key = nullptr;
  int *claimants = nullptr, *blk = nullptr;  // blk[blocks] is the record count
  rebvio_hip_kf_match* rec = nullptr;
  size_t lay(char* b, size_t kmax, size_t blocks) {
    Carve c(base = b);
    key = c.take<unsigned long long>(slots256(kmax));
    claimants = c.take<int>(slots256(kmax));
    blk = c.take<int>(blocks + 1);
    return c.size();
  }
};

// rebvio_hip_map_keyframe_pose (assoc_words = 0) and rebvio_hip_map_keyframe_align (assoc_words = kmax): the result block the
// kernels iterate on, rounded up to 64 bytes so that the partials start on a line; `blocks` partials of kfp::kSums doubles; as
// many used counts; the association words.
struct KfSolve : Layout {
  rebvio_hip_kf_pose* state = nullptr;
  double* part = nullptr;
  int *used = nullptr, *assoc = nullptr;
  size_t lay(char* b, size_t blocks, size_t assoc_words) {
    Carve c(base = b);
    state = c.take<rebvio_hip_kf_pose>(1);
    c.align(64);
    part = c.take<double>(blocks * kfp::kSums);
    used = c.take<int>(blocks);
    assoc = c.take<int>(assoc_words);
    return c.size();
  }
};

// rebvio_hip_map_keyframe_align_many: REBVIO_HIP_KF_HYP_MAX descriptors (Desc = KfHypDesc, 64 bytes each) and as many result
// blocks with nothing between them - the host stages both in one struct and uploads them in ONE copy - then per hypothesis
// `blocks` partials, used counts and inlier counts. sizeof(the host's stage) is a multiple of 64: the partials start on a line.
template <class Desc>
struct KfMany : Layout {
  Desc* desc = nullptr;
  rebvio_hip_kf_hyp_result* res = nullptr;
  double* part = nullptr;
  int *used = nullptr, *inl = nullptr;
  size_t lay(char* b, size_t blocks) {
    const size_t H = REBVIO_HIP_KF_HYP_MAX;
    Carve c(base = b);
    desc = c.take<Desc>(H);
    res = c.take<rebvio_hip_kf_hyp_result>(H);
    part = c.take<double>(H * blocks * kfp::kSums);
    used = c.take<int>(H * blocks);
    inl = c.take<int>(H * blocks);
    return c.size();
  }
};

// 8 count words - the kernel leaves its result struct in the first of them, and one clear of 32 bytes in front of the launch
// covers any of them - then `lists` (1 or 2) arrays of kmax words per keyline: rebvio_hip_kf_snapshot_fuse_depth (the six words of
// rebvio_hip_kf_fuse; out = the association), the depth-image entries (rebvio_hip_depth_prior_counts; out = the outcome) and the
// stereo entries (rebvio_hip_stereo_prior_counts; out = the outcome, out2 = the winner).
struct Counted : Layout {
  int *cnt = nullptr, *out = nullptr, *out2 = nullptr;
  size_t lay(char* b, size_t kmax, int lists) {
    Carve c(base = b);
    cnt = c.take<int>(8);
    out = c.take<int>(kmax);
    out2 = c.take<int>(lists > 1 ? kmax : 0);
    return c.size();
  }
};

// rebvio_hip_kf_snapshot_handover_depth: kmax claim words, kmax 8-byte staging records, 8 count words (the seven of
// rebvio_hip_kf_handover in front), kmax association words
struct KfHandover : Layout {
  unsigned long long* key = nullptr;
  kfp::HandoverStage* stage = nullptr;
  int *cnt = nullptr, *assoc = nullptr;
  size_t lay(char* b, size_t kmax) {
    Carve c(base = b);
    key = c.take<unsigned long long>(kmax);
    stage = c.take<kfp::HandoverStage>(kmax);
    cnt = c.take<int>(8);
    assoc = c.take<int>(kmax);
    return c.size();
  }
};

// rebvio_hip_map_edge_chains / _edge_polylines: Dev = ChainDev with its views (common.hpp says what each holds) laid over kp =
// ceil(kmax / 256) * 256 entries per keyline - the 16-byte records first, then the 8-byte ones, then the ints
template <class Dev>
struct Chains : Layout, Dev {
  size_t lay(char* b, size_t kmax, size_t blocks, size_t words_n) {
    const size_t kp = slots256(kmax);
    Carve c(base = b);
    this->node[0] = c.take<ech::ChainNode>(kp);
    this->node[1] = c.take<ech::ChainNode>(kp);
    this->refs = c.take<rebvio_hip_chain_ref>(kp);
    this->points = c.take<rebvio_hip_cloud_point>(kp);
    this->lines = c.take<rebvio_hip_polyline>(kp);
    this->refs2 = c.take<typename std::remove_pointer<decltype(Dev::refs2)>::type>(kp);
    this->succ = c.take<int>(kp);
    this->len = c.take<int>(kp);
    this->start_of = c.take<int>(kp);
    this->order = c.take<int>(kp);
    this->starts = c.take<int>(kp + 4);
    this->blk = c.take<int>(4 * blocks);
    this->words = c.take<int>(words_n);
    return c.size();
  }
};

// rebvio_hip_map_edge_segments: Dev = SegDev with its views (common.hpp says what each holds) laid over kp = ceil(kmax / 256) * 256
// entries per point - the 16-byte records first (80 = 5 x 16), then the 8-byte ones, then the ints
template <class Dev>
struct Segments : Layout, Dev {
  size_t lay(char* b, size_t kmax, size_t blocks, size_t words_n) {
    const size_t kp = slots256(kmax);
    Carve c(base = b);
    this->q = c.take<esg::SegPoint>(kp);
    this->recs = c.take<rebvio_hip_line_segment>(kp);
    this->span = c.take<esg::SegSpan>(kp);
    this->far[0] = c.take<unsigned long long>(kp);
    this->far[1] = c.take<unsigned long long>(kp);
    this->nxt = c.take<int>(kp);
    this->line_of = c.take<int>(kp);
    this->seg = c.take<int>(kp);
    this->blk = c.take<int>(4 * blocks);
    this->words = c.take<int>(words_n);
    return c.size();
  }
};

// the place entries: 385 histogram words (padded to 388: the query row stays 16-byte aligned), the query row of plc::kWords u16
// words and, next to it, its counted word - the row and the word are fetched in ONE copy - in a 16-byte tail
struct Place : Layout {
  unsigned* hist = nullptr;
  uint16_t* query = nullptr;
  int* counted = nullptr;
  size_t lay(char* b) {
    Carve c(base = b);
    hist = c.take<unsigned>(388);
    query = c.take<uint16_t>(plc::kWords);
    counted = c.take<int>(4);
    return c.size();
  }
};
}  // namespace scratch
}  // namespace rh
