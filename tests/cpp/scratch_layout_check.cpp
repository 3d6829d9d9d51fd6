// The layouts of the on-demand entries' device scratch (rebvio_amd/csrc/scratch_layout.hpp, the header api.hip allocates and
// carves them by) run as a stand-alone host program, meant to be built with -fsanitize=address,undefined: no GPU, no library,
// nothing loaded into another process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I rebvio_amd/csrc
//       tests/cpp/scratch_layout_check.cpp -o scratch_layout_check && ./scratch_layout_check
// For keylines_max in {1, 255, 256, 257, 1000, 65536} every scratch is laid out over a heap buffer of exactly the bytes its layout
// reports (256-byte aligned, as a device allocation is): the first and the last element of every view are written (a view past its
// allocation is caught), views may not overlap, every view's offset and every total must equal the expression api.hip used before
// the layouts were stated in one place - written out below: they are the specification - and the partials behind a result block lie
// on 64 bytes, the place query row on 16. Prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "scratch_layout.hpp"

using namespace rh;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

// stand-ins of the two types of common.hpp (it needs the HIP headers): the same sizes and member names
struct Desc {
  const void *prs, *matches, *normals;
  void *res, *part, *part_used, *part_inl;
  int size, pad;
};
static_assert(sizeof(Desc) == 64, "KfHypDesc: seven pointers, the size, padding");
struct Int2 {
  int x, y;
};
struct Dev {
  void* node[2];
  int *succ, *len, *start_of;
  rebvio_hip_chain_ref* refs;
  int *order, *starts, *blk, *words;
  void* points;
  Int2* refs2;
  rebvio_hip_polyline* lines;
};
struct Stage {  // what rebvio_hip_map_keyframe_align_many uploads in ONE copy
  Desc desc[REBVIO_HIP_KF_HYP_MAX];
  rebvio_hip_kf_hyp_result res[REBVIO_HIP_KF_HYP_MAX];
};
static_assert(sizeof(Stage) % 64 == 0 && offsetof(Stage, res) == sizeof(Desc) * REBVIO_HIP_KF_HYP_MAX, "no gap, a multiple of a line");

constexpr size_t kBlocks = 256, kChainWords = 32;  // kMaxRecBlocks, kChainWords (common.hpp)

struct View {
  const char* name;
  size_t off, bytes, want_off;
};

// One scratch over a heap buffer of exactly `size` bytes: lay(base) sets the views, views(base) lists them with the offsets wanted.
template <class LayFn, class ViewsFn>
void run(const char* what, size_t kmax, size_t want_size, LayFn lay, ViewsFn views) {
  const size_t size = lay(nullptr);
  CHECK(size == want_size);
  if (size != want_size) std::printf("  %s kmax %zu: %zu bytes, want %zu\n", what, kmax, size, want_size);
  char* base = static_cast<char*>(::operator new(size, std::align_val_t(256)));
  std::memset(base, 0, size);
  CHECK(lay(base) == size);
  std::vector<View> v = views(base);
  for (const View& a : v) {
    if (a.off != a.want_off) std::printf("  %s.%s kmax %zu: offset %zu, want %zu\n", what, a.name, kmax, a.off, a.want_off);
    CHECK(a.off == a.want_off);
    CHECK(a.off + a.bytes <= size);
    if (a.bytes && a.off + a.bytes <= size) {  // the first and the last byte of the view's first and last element lie in the buffer
      base[a.off] = 1;
      base[a.off + a.bytes - 1] = 1;
    }
  }
  std::sort(v.begin(), v.end(), [](const View& a, const View& b) { return a.off < b.off; });
  for (size_t i = 1; i < v.size(); ++i) CHECK(v[i - 1].off + v[i - 1].bytes <= v[i].off);
  ::operator delete(base, std::align_val_t(256));
}

#define VIEW(p, count, want) View{#p, (size_t)(reinterpret_cast<const char*>(p) - base), (size_t)(count) * sizeof(*(p)), (size_t)(want)}
#define VIEW_BYTES(p, bytes, want) View{#p, (size_t)(static_cast<const char*>(p) - base), (size_t)(bytes), (size_t)(want)}

int main() {
  const size_t I = sizeof(int), ULL = sizeof(unsigned long long);
  static_assert(sizeof(rebvio_hip_kf_pose) == 456 && sizeof(kfp::HandoverStage) == 8 && sizeof(ech::ChainNode) == 16, "as api.hip asserts");
  for (size_t kmax : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)1000, (size_t)65536}) {
    const size_t slots = (kmax + 255) / 256 * 256;
    {  // kf_scratch: slots * (sizeof(unsigned long long) + sizeof(int)) + (kMaxRecBlocks + 1) * sizeof(int)
      scratch::KfMatches s;
      run("kf", kmax, slots * (ULL + I) + (kBlocks + 1) * I, [&](char* b) { return s.lay(b, kmax, kBlocks); }, [&](const char* base) {
        return std::vector<View>{VIEW(s.key, slots, 0), VIEW(s.claimants, slots, slots * ULL), VIEW(s.blk, kBlocks + 1, slots * (ULL + I))};
      });
    }
    const size_t head = (sizeof(rebvio_hip_kf_pose) + 63) / 64 * 64, part = kBlocks * kfp::kSums * sizeof(double);
    for (size_t assoc : {(size_t)0, kmax}) {  // keyframe_pose: head + part + kMaxRecBlocks * sizeof(int); _align: + keylines_max * sizeof(int)
      scratch::KfSolve s;
      run(assoc ? "kfa" : "kfp", kmax, head + part + kBlocks * I + assoc * I, [&](char* b) { return s.lay(b, kBlocks, assoc); },
          [&](const char* base) {
            CHECK(reinterpret_cast<uintptr_t>(s.part) % 64 == 0);
            return std::vector<View>{VIEW(s.state, 1, 0), VIEW(s.part, kBlocks * kfp::kSums, head), VIEW(s.used, kBlocks, head + part),
                                     VIEW(s.assoc, assoc, head + part + kBlocks * I)};
          });
    }
    {  // keyframe_align_many: sizeof(Stage) + REBVIO_HIP_KF_HYP_MAX * (part + 2 * cnt)
      const size_t H = REBVIO_HIP_KF_HYP_MAX, cnt = kBlocks * I;
      scratch::KfMany<Desc> s;
      run("kfm", kmax, sizeof(Stage) + H * (part + 2 * cnt), [&](char* b) { return s.lay(b, kBlocks); }, [&](const char* base) {
        CHECK(reinterpret_cast<uintptr_t>(s.part) % 64 == 0);
        return std::vector<View>{VIEW(s.desc, H, 0), VIEW(s.res, H, offsetof(Stage, res)), VIEW(s.part, H * kBlocks * kfp::kSums, sizeof(Stage)),
                                 VIEW(s.used, H * kBlocks, sizeof(Stage) + H * part), VIEW(s.inl, H * kBlocks, sizeof(Stage) + H * part + H * cnt)};
      });
    }
    for (int lists : {1, 2}) {  // fuse_depth, the depth image: (8 + keylines_max) * sizeof(int); stereo: (8 + 2 * keylines_max) * sizeof(int)
      scratch::Counted s;
      run(lists == 1 ? "kff/dpr" : "spr", kmax, (8 + lists * kmax) * I, [&](char* b) { return s.lay(b, kmax, lists); }, [&](const char* base) {
        return std::vector<View>{VIEW(s.cnt, 8, 0), VIEW(s.out, kmax, 8 * I), VIEW(s.out2, lists == 2 ? kmax : 0, (8 + kmax) * I)};
      });
    }
    {  // handover_depth: kmax * (sizeof(unsigned long long) + sizeof(kfp::HandoverStage) + sizeof(int)) + 8 * sizeof(int)
      scratch::KfHandover s;
      run("kfh", kmax, kmax * (ULL + sizeof(kfp::HandoverStage) + I) + 8 * I, [&](char* b) { return s.lay(b, kmax); }, [&](const char* base) {
        return std::vector<View>{VIEW(s.key, kmax, 0), VIEW(s.stage, kmax, kmax * ULL), VIEW(s.cnt, 8, kmax * (ULL + sizeof(kfp::HandoverStage))),
                                 VIEW(s.assoc, kmax, kmax * (ULL + sizeof(kfp::HandoverStage)) + 8 * I)};
      });
    }
    {  // ech_scratch: the 16-byte records first, then the 8-byte ones, then the ints
      const size_t kp = slots, N = sizeof(ech::ChainNode), R = sizeof(rebvio_hip_chain_ref), P = sizeof(rebvio_hip_cloud_point),
                   L = sizeof(rebvio_hip_polyline), R2 = sizeof(Int2);
      const size_t bytes = kp * (2 * N + R + P + L + R2 + 4 * I) + (kp + 4 + 4 * kBlocks + kChainWords) * I;
      scratch::Chains<Dev> s;
      run("ech", kmax, bytes, [&](char* b) { return s.lay(b, kmax, kBlocks, kChainWords); }, [&](const char* base) {
        size_t o = 0;
        auto next = [&o](size_t n) { const size_t at = o; o += n; return at; };
        std::vector<View> v;
        v.push_back(VIEW_BYTES(s.node[0], kp * N, next(kp * N)));
        v.push_back(VIEW_BYTES(s.node[1], kp * N, next(kp * N)));
        v.push_back(VIEW(s.refs, kp, next(kp * R)));
        v.push_back(VIEW_BYTES(s.points, kp * P, next(kp * P)));
        v.push_back(VIEW(s.lines, kp, next(kp * L)));
        v.push_back(VIEW(s.refs2, kp, next(kp * R2)));
        v.push_back(VIEW(s.succ, kp, next(kp * I)));
        v.push_back(VIEW(s.len, kp, next(kp * I)));
        v.push_back(VIEW(s.start_of, kp, next(kp * I)));
        v.push_back(VIEW(s.order, kp, next(kp * I)));
        v.push_back(VIEW(s.starts, kp + 4, next((kp + 4) * I)));
        v.push_back(VIEW(s.blk, 4 * kBlocks, next(4 * kBlocks * I)));
        v.push_back(VIEW(s.words, kChainWords, next(kChainWords * I)));
        CHECK(o == bytes);
        return v;
      });
    }
    {  // place_scratch: 388 * sizeof(unsigned) + kPlcRowBytes + 16; the row and its counted word are read in one copy
      const size_t hist = 388 * sizeof(unsigned), row = plc::kWords * sizeof(uint16_t);
      scratch::Place s;
      run("plc", kmax, hist + row + 16, [&](char* b) { return s.lay(b); }, [&](const char* base) {
        CHECK(reinterpret_cast<uintptr_t>(s.query) % 16 == 0);
        CHECK(reinterpret_cast<const char*>(s.counted) == reinterpret_cast<const char*>(s.query) + row);
        return std::vector<View>{VIEW(s.hist, 388, 0), VIEW(s.query, plc::kWords, hist), VIEW(s.counted, 4, hist + row)};
      });
    }
  }
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
