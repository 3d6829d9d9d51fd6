// C-ABI of the gfx950 backend (include/rebvio_hip.h): context / edge-map pool management, stream ordering
// between the detect stream and the track stream, and the O(1) host glue of one frame pair. All heavy work
// is in detect.hip / track.hip; nothing here falls back to a CPU implementation of the hot path.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <shared_mutex>
#include <thread>
#include <string>
#include <vector>

#include "common.hpp"
#include "depth_prior.hpp"
#include "glue.hpp"
#include "hostmath.hpp"
#include "kf_cloud.hpp"
#include "edge_chains.hpp"
#include "kf_handover.hpp"
#include "kf_many.hpp"
#include "kf_pose.hpp"
#include "owned.hpp"
#include "pixel_format.hpp"
#include "place.hpp"
#include "scratch_layout.hpp"
#include "stereo_prior.hpp"

using namespace rh;

namespace {
thread_local std::string g_err;
// streams a context under construction adopts instead of creating its own (lanes of a batch share one set)
struct SharedStreams {
  hipStream_t s_det, s_key, s_trk;
};
thread_local const SharedStreams* t_adopt_streams = nullptr;

// ---- device-wide registry of the persistent LM kernels' users (this process) -------------------------------------------------
// The workgroups of a persistent LM launch wait for each other's records, so all of them have to be resident together; the
// occupancy check of a batch (lm_chain_b_max_lanes) assumes it has the device to itself. Every context with the persistent
// kernel and every batch registers here when it is created; a batch sizes each LM launch to ITS SHARE of the device - capacity /
// live users on that GPU - so that two batches (or a batch beside single streams) still fit together: slower, not timed out.
// Kernels of other processes are invisible to this registry: what remains for them is the bounded poll (-9).
struct Residency {
  std::mutex mu;
  std::map<int, std::map<const void*, int>> users;  // device -> owner -> workgroups of its largest LM launch
};
Residency& residency() {
  static Residency r;
  return r;
}
void residency_add(int device, const void* owner, int wgs) {
  std::lock_guard<std::mutex> lk(residency().mu);
  residency().users[device][owner] = wgs;
}
void residency_remove(int device, const void* owner) {
  std::lock_guard<std::mutex> lk(residency().mu);
  auto it = residency().users.find(device);
  if (it != residency().users.end()) it->second.erase(owner);
}
int residency_users(int device) {
  std::lock_guard<std::mutex> lk(residency().mu);
  auto it = residency().users.find(device);
  return it == residency().users.end() ? 0 : (int)it->second.size();
}
std::string residency_describe(int device, const void* self) {
  std::lock_guard<std::mutex> lk(residency().mu);
  auto it = residency().users.find(device);
  int others = 0, wgs = 0;
  if (it != residency().users.end())
    for (auto& u : it->second)
      if (u.first != self) {
        ++others;
        wgs += u.second;
      }
  char msg[200];
  std::snprintf(msg, sizeof(msg), "%d other context(s) / batch(es) of this process run persistent LM kernels on GPU %d (up to %d workgroups "
                "together); kernels of other processes are not visible to this check", others, device, wgs);
  return msg;
}

// REBVIO_HIP_DM_HEAD / REBVIO_HIP_BATCH_DM_HEAD -> form of the directedMatch launch (track.hip: dm_head_wide, dm_compact)
int dm_form_by_name(const char* e) {
  static const char* const names[] = {"", "compact8", "compact4", "compact1"};
  for (int i = 1; i < 4; ++i)
    if (std::strcmp(e, names[i]) == 0) return i;
  return 0;
}

int fail(const char* what, hipError_t e) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return -(int)e - 1000;
}
int fail_msg(const char* what, int code) {
  g_err = what;
  return code;
}
#define HIPCHK(expr)                          \
  do {                                        \
    hipError_t _e = (expr);                   \
    if (_e != hipSuccess) return fail(#expr, _e); \
  } while (0)
// the same for a callee that has already set g_err and returns the entry's code
#define RCCHK(expr)            \
  do {                         \
    const int _rc = (expr);    \
    if (_rc) return _rc;       \
  } while (0)

// ---- profiler ------------------------------------------------------------------------------------
struct Profiler {
  bool on = false;
  std::string only;
  int stride = 1;        // record every stride-th launch of a kernel (keeps the timed region cheap)
  std::map<std::string, unsigned> seen;
  struct Sample {
    int name;
    hipEvent_t e0, e1;
    int count;  // launches bracketed by this event pair
  };
  std::vector<std::string> names;
  std::vector<Sample> samples;
  std::vector<hipEvent_t> free_events;
  std::map<int, std::pair<double, int>> acc;  // name -> (sum us, calls)
  size_t cap = 1 << 16;
  std::mutex mu;

  int name_id(const char* n) {
    for (size_t i = 0; i < names.size(); ++i)
      if (names[i] == n) return (int)i;
    names.emplace_back(n);
    return (int)names.size() - 1;
  }
  hipEvent_t get_event() {
    if (!free_events.empty()) {
      hipEvent_t e = free_events.back();
      free_events.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
  void drain() {
    for (auto& s : samples) {
      float ms = 0.f;
      if (hipEventSynchronize(s.e1) == hipSuccess && hipEventElapsedTime(&ms, s.e0, s.e1) == hipSuccess) {
        auto& a = acc[s.name];
        a.first += (double)ms * 1e3;
        a.second += s.count;
      }
      free_events.push_back(s.e0);
      free_events.push_back(s.e1);
    }
    samples.clear();
  }
};
Profiler g_prof;
// The open bracket belongs to the launching THREAD (a batch's caller thread and its detect worker launch concurrently).
struct ProfOpen {
  int group_depth = 0;  // inside prof_group_begin/end the individual launches are not bracketed again
  int count = 1;
  int name = -1;
  hipEvent_t e0{}, e1{};
};
thread_local ProfOpen t_open;
}  // namespace

namespace rh {
// selection by exact name, or by prefix when the selector ends with '*'
static bool prof_name_selected(const std::string& only, const char* name) {
  if (!only.empty() && only.back() == '*') return std::strncmp(only.c_str(), name, only.size() - 1) == 0;
  return only == name;
}
void prof_begin(hipStream_t s, const char* name) {
  if (!g_prof.on) return;
  if (t_open.group_depth > 0) return;
  t_open.count = 1;
  t_open.name = -1;
  {
    std::lock_guard<std::mutex> g(g_prof.mu);
    if (!g_prof.only.empty() && !prof_name_selected(g_prof.only, name)) return;
    if (g_prof.stride > 1 && (g_prof.seen[name]++ % (unsigned)g_prof.stride) != 0) return;
    if (g_prof.samples.size() >= g_prof.cap) return;
    t_open.name = g_prof.name_id(name);
    t_open.e0 = g_prof.get_event();
    t_open.e1 = g_prof.get_event();
  }
  (void)hipEventRecord(t_open.e0, s);
}
void prof_end(hipStream_t s) {
  if (!g_prof.on) return;
  if (t_open.group_depth > 0) return;
  if (t_open.name < 0) return;
  (void)hipEventRecord(t_open.e1, s);
  std::lock_guard<std::mutex> g(g_prof.mu);
  g_prof.samples.push_back({t_open.name, t_open.e0, t_open.e1, t_open.count});
  t_open.name = -1;
}
// One event pair around `count` back-to-back launches of the same kernel on one stream: the fixed cost of an event
// pair (~4.5 us measured around an empty kernel) is amortised, so the per-launch average agrees with rocprofv3's.
void prof_group_begin(hipStream_t s, const char* name, int count) {
  if (!g_prof.on) return;
  prof_begin(s, name);
  t_open.count = count;
  t_open.group_depth = 1;
}
void prof_group_end(hipStream_t s) {
  if (!g_prof.on) return;
  t_open.group_depth = 0;
  prof_end(s);
}
}  // namespace rh

// ---- objects ----------------------------------------------------------------------------------------
// Shared by a context and every map handle it has handed out: a map released (or queried) after rebvio_hip_destroy must not
// touch the freed context. The block outlives the context for as long as a handle is still out; `dead` is set by destroy,
// under `mu`, which also serialises destroy against a release from another thread (an EdgeMap::SharedPtr kept by an
// edge-image consumer, ros_rebvio.cpp:32-51, is released whenever that consumer lets go of it).
struct LifeBlock {
  std::shared_mutex mu;  // shared: every entry point that takes a map alone, for its whole duration; exclusive: rebvio_hip_destroy
  std::atomic<bool> dead{false};
};

struct rebvio_hip_map {
  rebvio_hip_ctx* ctx = nullptr;
  std::shared_ptr<LifeBlock> life;
  Owned own;  // the arrays of `d` and the three events below
  MapDev d{};
  bool in_use = false;
  uint64_t ts = 0;
  hipEvent_t detected{};  // keylines + mask + chaining finished (detect stream)
  hipEvent_t ready{};     // ... and distance field built (distance-field stream)
  hipEvent_t done{};   // last track-stream consumer finished, recorded at release
  hipEvent_t done_ref{};  // ... or (streaming driver) the result-slot event of the pair that used the map last: no packet of its own
  bool has_done = false;
  // ... or (streaming driver, stamp hand-over) no event at all: the map's last consumer has finished once the pair queue has proven
  // this many steps complete (PairQueue::proven). 0: none, `done` / `done_ref` hold.
  uint64_t done_token = 0;
  uint64_t release_seq = 0;  // order of release (pool reuse is oldest-first)
  bool df_built = false;
  bool raster_order = false;  // keylines + row_start as detection left them (false after map_upload)
  std::atomic<int> enqueued{1};  // 0 while the batch's detect worker still has to record `ready`
  bool pre_rotated = false;  // the next pair's first rotateKeylines (+ histogram) was already applied by the fused B-chain
  int n_host = -1;
  float thr_host = -1.0f;
  bool trk_waited = false;  // the track stream already holds a wait on `ready` (a second one is another barrier packet)
  // set once any track-stream operation referencing this map has been enqueued: until then a download only has to wait for
  // the map's own detection (`ready`), not for the track stream (which may hold another pair's parked second half)
  std::atomic<bool> trk_touched{false};
  hm::M3 pre_R{};           // ... with this rotation (per-pair API: checked against the prior the next _begin is given)
  // per-pair API: _finish_async was given R_prior_next for this map and the next _begin has not consumed it yet - the keylines are
  // (or will be, in stream order) in the next pair's frame: the point-cloud entries refuse the map (-7)
  std::atomic<bool> promised{false};
  // per-pair API: rebvio_hip_track_pair / _begin has taken this map as a pair's OLD map - its rho / sigma_rho have been (or will be,
  // in stream order) carried into a newer frame: the depth-image entries refuse it (-7). Host-side only; cleared by acquire_map.
  bool served_old = false;
  // streaming / batch drivers: the gyro rotation the frame was pushed with (interval from the frame pushed before it to this one;
  // rebvio_hip_push_frame_px_gyro*). Not set: the identity.
  bool gyro_set = false;
  float gyro_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  // streaming driver: rebvio_hip_keyframe_next was called in front of this frame - the map is marked (k_mark_keyframe) in front of
  // the pair it is the OLD map of. Cleared there, and wherever the map goes back to the pool (release_map).
  bool kf_flag = false;
  int tab_idx = -1;         // entry of this map in its lane's device map table (batch driver)
  MapDev canon{};           // ... as uploaded there (the live `d` differs from it by the ping-pong swaps only)
};

// One point cloud (rebvio_hip_map_point_cloud*): the device buffer the extraction kernels write (track stream), the host-visible
// buffer the copy kernel fills from it (cloud stream) - head, then the records, in both - and the events behind the two. Pooled
// per context; like a map handle it may outlive the context as a husk.
struct rebvio_hip_cloud {
  rebvio_hip_ctx* ctx = nullptr;
  std::shared_ptr<LifeBlock> life;
  Owned own;                   // the two buffers and the two events
  CloudHdr* hdr = nullptr;     // pinned: 64-byte head + keylines_max records
  char* dev_buf = nullptr;     // device, the same shape: the count at byte 0, the records at byte 64
  void* dev = nullptr;         // device address of the records (dev_buf + 64)
  hipEvent_t extracted{};      // recorded on the track stream behind the extraction
  hipEvent_t done{};           // recorded on the cloud stream behind the copy to the host
  unsigned seq = 0;            // the extraction's sequence stamp
  int cap = 0;                 // records the extraction may write
  bool in_use = false;
};

// A keyframe snapshot (rebvio_hip_map_keyframe_snapshot): one device buffer - ceil(keylines_max / 256) * 256 records of 16 bytes
// (pos_img, rho, sigma_rho), as many matches words, the size - written by k_kf_snapshot on the track stream. Listed in its
// context, which frees the buffer when it is destroyed; like a map handle it may outlive the context as a husk.
struct rebvio_hip_kf_snapshot {
  rebvio_hip_ctx* ctx = nullptr;
  std::shared_ptr<LifeBlock> life;
  Owned own;                   // the buffer
  char* buf = nullptr;
  void* prs = nullptr;         // views into buf
  unsigned* matches = nullptr;
  int* n_dev = nullptr;
  int n_host = -1;             // the size, once a synchronous entry has fetched it
  // rebvio_hip_kf_snapshot_add_normals: a second buffer of `own`, one float2 per slot, made at the first call (normals_buf) and
  // handed to its readers (normals) only once a kernel that fills it has been queued: a call that fails in between leaves a
  // snapshot without normals, not one with uninitialised ones. nor_mu guards both pointers in every entry that touches them.
  std::mutex nor_mu;
  void* normals_buf = nullptr;
  void* normals = nullptr;
};

// A place database (rebvio_hip_place_db_create): `cap` signature rows of 768 bytes in one device buffer, and a second one with the
// cap distance words of a query, the cap counted words of the entries and the result block (a 16-byte head with the count, 16
// records). Size and tags live on the host. Listed in its context, which frees the buffers when it is destroyed; like a snapshot
// it may outlive the context as a husk.
struct rebvio_hip_place_db {
  rebvio_hip_ctx* ctx = nullptr;
  std::shared_ptr<LifeBlock> life;
  Owned own;                   // the two buffers
  uint16_t* rows = nullptr;
  unsigned* dist = nullptr;    // views into the second buffer
  int* counted = nullptr;
  char* res = nullptr;
  int cap = 0;
  int size = 0;
  std::vector<uint64_t> tags;
};

// A finished pair's record as the caller gets it.
struct PairRec {
  rebvio_hip_pair_out out;
  int keylines;
};

// What the streaming driver (one lane) and a batch (its lanes, in lock-step) share from queueing a step's pairs on the track stream
// to handing their records to the caller. A step holds one pair per lane; the queue never holds more than kPairSlots - 1 steps
// (the result slot of step k is reused by step k + kPairSlots), so it is a fixed ring: no heap allocation per step.
struct PairQueue {
  struct Step {                     // a step whose kernels are queued and whose records have not been read yet
    rebvio_hip_map* nm[kMaxLanes];  // each lane's new map
    uint32_t seq = 0;               // the step's sequence stamp (all lanes)
    int slot = -1;
    int ev_slot = -1;               // the slot whose event stands for this step's completion (its group's last step); -1: none,
                                    // the successor's record stamp does (streaming driver, see harvest)
    uint64_t idx = 0;               // steps queued before this one
  };
  Step ring[kPairSlots];
  int head = 0, count = 0;
  uint64_t pushed = 0;               // steps queued so far
  // Steps the HOST knows to be complete: it has read their records. Every kernel of step k < proven has ended; maps released with
  // the token k + 1 are idle once proven reaches it (release_map). Written by the tracking thread, read by whoever detects.
  std::atomic<uint64_t> proven{0};
  Step& operator[](int i) { return ring[(head + i) % kPairSlots]; }
  void push_back(const Step& st) {
    Step& d = ring[(head + count++) % kPairSlots];
    d = st;
    d.idx = pushed++;
  }
  void pop_front() {
    proven.store(ring[head].idx + 1, std::memory_order_release);
    head = (head + 1) % kPairSlots;
    --count;
  }
  std::deque<PairRec> done;          // records waiting for the caller: one per lane and step, in lane order
  hipEvent_t slot_ev[kPairSlots]{};  // recorded behind a group's last kernel
  double t_wait = 0;                 // REBVIO_HIP_DEBUG: host time spent waiting for result slots (us)
};

struct rebvio_hip_ctx {
  std::shared_ptr<LifeBlock> life = std::make_shared<LifeBlock>();
  // Every device buffer, pinned buffer, event and stream of the context, those allocated on first use included. The pointers
  // and handles below are views of them (copied by value into MapDev, LaneStatic and kernel arguments); pooled maps and clouds
  // own theirs, a batch owns the streams its lanes adopt.
  Owned own;
  rebvio_hip_params P{};
  KParams K{};
  int device = 0;
  hipStream_t s_det{}, s_key{}, s_trk{};  // scans | keylines + distance field (+ the synchronous API's copies) | tracking
  double t_begin_enq = 0, t_begin_wait = 0;  // REBVIO_HIP_DEBUG: host time of track_pair_begin (enqueue / wait for the first half)
  uint64_t t_begin_n = 0;
  std::mutex dl_mu;             // aos_dev / scratch_i users (map_download, map_upload, render, field decode) and trk_touched
  float* sa2[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [frame parity][filter]: sb.a per parity ([0] aliases sb.a)
  // scale-space outputs (DoG, squared gradient, per-row counts) are double buffered: the scans of frame f+1 (s_det)
  // overlap the keyline extraction of frame f (s_key)
  float* dog2[kDetPar]{};  // (the single-stream driver alternates between [0] and [1], a batch uses all: common.hpp kDetPar)
  float* mag2[kDetPar]{};
  int* rowcount2[kDetPar]{};
  hipEvent_t ev_scan[2]{};
  // `ready` event of the map detected two frames ago (same parity): what the scans of this frame wait for before they rewrite
  // that frame's buffers. It is recorded a few microseconds behind the point the buffers are free (after the distance field
  // instead of after joinEdges), two frame times before anyone waits for it - and it is an event the frame records anyway: one
  // hipEventRecord less per frame on the launching thread (3.5 us of its 62, round 4).
  hipEvent_t prev_ready[2]{};
  uint64_t launch_index = 0;
  uint64_t release_counter = 0;
  ScaleBufs sb{};
  DetectBufs db{};
  DetState* det = nullptr;  // [kDetRing] servo-state ring + [kDetRing]: scratch sink
  uint64_t frame_index = 0;
  rebvio_hip_map* last_detected = nullptr;
  int widths[2][3]{};
  std::vector<rebvio_hip_map*> pool;
  float* img_dev = nullptr;
  uint8_t* img8_dev = nullptr;
  static constexpr int kPin = 16;  // pinned staging ring of the host-frame detect entries (allocated on first use)
  uint8_t* pin[kPin]{};
  hipEvent_t pin_ev[kPin]{};
  bool pin_used[kPin]{};
  uint64_t pin_next = 0;
  int2* undist_map = nullptr;      // fixed-point source coordinates (null: no lens distortion, front end = x3 only)
  float* undist_img[kDetPar]{};    // undistorted fp32 frame, buffered like dog2 / mag2
  uint8_t* dmask_buf = nullptr;    // static detection mask, rows*cols bytes (rebvio_hip_set_detection_mask; allocated on first use)
  const uint8_t* dmask = nullptr;  // dmask_buf while a static mask is set, else null
  rebvio_hip_batch* batch = nullptr;  // the batch this context is a lane of (null: a stand-alone context)
  rebvio_hip_keyline* aos_dev = nullptr;
  int* scratch_i = nullptr;  // 2 * rows*cols ints (df decode)
  float* diag0 = nullptr;
  float* diag1 = nullptr;
  // tracking
  LmState* lm = nullptr;    // [16]
  float* part = nullptr;    // [kMaxLmCalls+1][maxblocks][kPartStride]
  float* xrv_part = nullptr;
  int* hist = nullptr;      // [128]
  float* fscratch = nullptr;
  int maxblocks = 0;
  // persistent LM kernel: record exchange words, tags consumed so far, sticky time-out flag
  unsigned long long* lm_xch = nullptr;
  unsigned lm_tag_base = 0;
  bool lm_spec = true;          // the speculative kernel may be used ...
  bool lm_spec_forced = false;  // ... always (REBVIO_HIP_LM=spec / spec3), instead of by the stream's recent miss rates
  int lm_spec_forced_kf = 2;    // first speculative evaluation of the forced form
  int lm_mix = 0;               // REBVIO_HIP_LM=mix<seed> (seed >= 1): see lm_kernel_choice
  float lm_miss_ema = 0.f;      // recent rate of "a step after the first was accepted" (the hypothesis of kf = 2 failed)
  float lm_miss3_ema = 0.f;     // ... "a step after the second was accepted" (the hypothesis of kf = 3 failed)
  int* lm_bar_err = nullptr;  // pinned, zero-copy
  unsigned long long* lm_stamps = nullptr;  // pinned; REBVIO_HIP_LM_STAMPS diagnostic (phase stamps of workgroup 0)
  unsigned long long* dm_stats = nullptr;   // device; REBVIO_HIP_DM_STATS diagnostic (workload shape + per-wave phase times of k_directed_match_c)
  size_t dm_stats_words = 0;
  double lm_stamp_acc[64]{};
  uint64_t lm_stamp_n = 0;
  bool lm_stamp_spec = false;
  bool lm_persistent = true;
  bool residency_registered = false;  // this context launches persistent LM kernels of its own (Residency)
  rebvio_hip_map* df_map = nullptr;
  // pinned host staging
  LmState* h_lm = nullptr;   // [2]
  float* h_part = nullptr;
  float* h_xrv = nullptr;
  MapState* h_st = nullptr;  // [2]
  float* h_f = nullptr;
  // glue state (types/imu.hpp:171-187)
  float Bg[3]{};
  hm::M3 W_Bg{}, RGBias{}, RGyro{};
  LmState* lm_zero = nullptr;  // constant start state of minimizeVel (Vg = 0, rebvio.cpp:167)
  int lm_threads = 512;        // workgroup size of the persistent LM kernels (REBVIO_HIP_LM_THREADS: 256 | 512 | 1024)
  int dm_head_form = 0;        // directedMatch launch form: 0 by map size, 1 compact8, 2 compact4, 3 compact1 (REBVIO_HIP_DM_HEAD; track.hip dm_form)
  // Result slots. slot[0] also serves the per-pair API. The streaming driver (rebvio_hip_push_frame_u8_device) keeps the
  // WHOLE pair step on the device - the glue between the halves runs in front of the directedMatch head (glue.hpp) - and the
  // host reads a pair's records kSlots - 1 pairs late at most.
  static constexpr int kSlots = kPairSlots;
  PairSlot* slot[kSlots]{};    // pinned: LM state + map state records, written by the pair's first kernel
  GlueRec* rec[kSlots]{};      // pinned: what the device glue of the pair reports
  GlueDev* glue_dev = nullptr;    // [kSlots] second-half inputs left by the device glue for the kernels behind it
  GlueStage* glue_stage = nullptr;  // [kSlots] host records on their way out: written by the glue, forwarded by the directedMatch launch
  GlueState* gstate = nullptr;    // [2] device: gyro-bias filter state + prior rotation, by pair parity
  GlueState* h_gstate = nullptr;  // [2] pinned staging for the upload in front of a stream's first pair
  hm::M3 gs_R{};                  // host mirror of the device state's prior rotation (with Bg / W_Bg above)
  int min_pool = 0;               // edge maps to allocate before one is reused (see acquire_map)
  int lead = 5;                   // detected frames queued when a pair is started (REBVIO_HIP_LEAD 3..12, see push_frame)
  // How the streaming driver's track stream hands pairs to the host and maps back to the detect stage. Default: it records no
  // event - harvest reads the successor's record stamp, a pair's old map is released with a token. REBVIO_HIP_HANDOVER=events:
  // one event per group of pairs (and per pair queued alone), event-based harvest and release.
  bool handover_events = false;
  // [stream: track, scan, keyline] waits queued / waits left out because the host knew their reason gone (a map's release token
  // observed) / events recorded, and the reuses of a map whose token the host had not observed yet
  // (rebvio_hip_test_handover_counters; printed by flush with REBVIO_HIP_DEBUG)
  struct Handover {
    std::atomic<uint64_t> queued[3]{}, skipped[3]{}, events[3]{}, reuse_fallbacks{0};
  } ho;
  int group = 4;                  // pairs queued together (REBVIO_HIP_GROUP 1..6, see stream_enqueue_group)
  // Sequence stamps of the host-visible records (PairSlot::seq, GlueRec::seq_gs / seq_out): every pair that is queued takes
  // the next non-zero value, its kernels store it behind everything else they write into the records, and whoever reads a
  // record compares. A record read before its pair ran (an event or a synchronisation that reported too early - seen once with
  // kernel-bound stop events) still holds its previous user's stamp: status -12 instead of silently stale poses.
  uint32_t stamp_seq = 0;         // last value handed out
  uint32_t last_stamp = 0;        // stamp of the pair enqueue_pair_lm queued last
  bool forge_stamp = false;       // rebvio_hip_test_forge_record_stamp: the next pair's kernels are handed a wrong stamp
  // Pool bookkeeping (in_use, has_done / done / done_ref, release_seq, release_counter, df_map, the pool vector) is written by
  // whoever releases a map - the tracking thread, or any thread that lets go of an EdgeMap (an edge-image consumer,
  // ros_rebvio.cpp:32-51) - and read by the acquisition thread: one mutex around both sides, so that a map seen as free is seen
  // with the event its next user has to wait for.
  std::mutex pool_mu;
  std::vector<rebvio_hip_map*> frames;  // detected maps not yet consumed as "old"
  PairQueue q;                          // pairs in flight and records waiting for the caller (streaming driver)
  uint64_t pair_seq = 0;
  // Gyro rotations in the streaming driver (rebvio_hip_push_frame_px_gyro*). gyro_stream: a frame has been pushed with a rotation;
  // from then on a flush leaves the newest map un-rotated (its successor's rotation is not known) and keeps it in `carry`, and the
  // next push continues the stream from it. plain_flushed: a stream WITHOUT rotations was flushed, i.e. its newest map was rotated
  // for an identity measurement and dropped: a rotation pushed next has no frame to refer to (refused, -7).
  bool gyro_stream = false;
  bool plain_flushed = false;
  rebvio_hip_map* carry = nullptr;
  // rebvio_hip_test_glue_set_next: GlueParams::R_next / has_next of the rebvio_hip_test_glue calls
  float test_R_next[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  int test_has_next = 1;
  // one frame's detection: its map and servo-state ring slots (detect_prepare), launched by detect_launch
  struct DetJob {
    rebvio_hip_map* m;
    const void* img;
    int is_u8;
    const DetState* det_in;
    DetState* det_out;
    const MapState* prev_st;
    int pin_slot = -1;      // host-frame entries: pinned ring slot to copy to `img` (device staging frame) ahead of the scans
    size_t pin_bytes = 0;
    int fmt = 0;            // pixel format of a u8 frame (pixel_format.hpp)
    const uint8_t* mask_static = nullptr;  // detection masks of this frame (null: none): the context's static mask ...
    const uint8_t* mask_frame = nullptr;   // ... and the caller's per-frame device mask
  };
  std::mutex det_mu;
  std::string det_error;  // a detection failed half way (detect_failed): every later detect / push reports -8 with it
  // host-side phase timing of the streaming driver (printed by flush when REBVIO_HIP_DEBUG is set)
  double t_detect_enq = 0, t_enq = 0, t_queued = 0;
  double t_det_launch = 0;  // the detect launches alone (us, one per frame) ...
  uint64_t t_det_n = 0;     // ... over this many frames
  bool dbg = false;
  // host shadow of the information matrix W_Bg the DEVICE glue works on (streaming driver, glue_params_pre)
  hm::M3 wbg_shadow{};
  bool wbg_shadow_valid = false;
  bool gyro_pre_on = true;  // REBVIO_HIP_GYRO_PRE=0: the device forms the gyroBiasCorrection matrices itself
  uint64_t t_frames = 0;
  bool owns_streams = true;  // false for the lanes of a batch (rebvio_hip_batch_*)
  rebvio_hip_map* bf_map[2] = {nullptr, nullptr};  // new map of the pair whose counters result slot r will report
  bool bf_have[2] = {false, false};           // h_bf[r] already holds them (taken from the next pair's slot, or copied)
  bool bf_copy_queued[2] = {false, false};    // a device-to-host copy + bf_done[r] are queued for them
  // two result slots: the next pair's first half (and its parked second half) may be queued before the caller fetches the
  // previous pair's counters (rebvio_hip_track_pair_finish_async / _result)
  hipEvent_t bf_done[2]{};
  // fetch_map_state: orders its copy behind another stream (created on first use). Only the tracking thread's entries
  // (directed_match, regularize) pass that stream, and they already share h_st, so neither the first use nor the event is raced.
  hipEvent_t fetch_ev{};
  MapState* h_bf = nullptr;  // [2] pinned
  int bf_cur = 0;            // slot of the pair between _begin and _finish_async
  int bf_res = -1;           // slot whose result is to be fetched (-1: none)
  bool bf_nan[2] = {false, false};
  // point clouds: buffers (allocated on first use, kept), the block counts + ticket word of the extraction kernels, and the
  // stamp counter. cloud_mu: the pool (rebvio_hip_cloud_release may come from any thread). The entries that queue an extraction
  // follow the track-entry thread rule: they launch on the track stream.
  std::mutex cloud_mu;
  std::vector<rebvio_hip_cloud*> clouds;
  int* cloud_scratch = nullptr;  // [kMaxRecBlocks] counts, then the ticket word
  hipStream_t s_cloud{};         // the copies to the host: PCIe writes next to the track stream's kernels, not between them
  unsigned cloud_seq = 0;
  // keyframes: rebvio_hip_keyframe_next is pending for the next frame pushed
  bool kf_pending = false;
  // keyframe snapshots and place databases that are out (their mutexes: a release may come from any thread)
  std::mutex snap_mu;
  std::vector<rebvio_hip_kf_snapshot*> snaps;
  // Scratch of the on-demand entries, track-side ones all: each ONE device allocation made at the entry's first call and kept
  // (scratch_layout.hpp states what lies where; ensure_scratch makes it). kf: the correspondences, with the records as a second
  // allocation; kfp / kfa / kfm: the solves of keyframe_pose, _align and _align_many; kff / kfh: fuse_depth and handover_depth; ech:
  // the edge chains and polylines; dpr / spr: the depth-image and stereo entries; plc: the place entries.
  scratch::KfMatches kf;
  scratch::KfSolve kfp, kfa;
  scratch::KfMany<KfHypDesc> kfm;
  scratch::Counted kff, dpr, spr;
  scratch::KfHandover kfh;
  scratch::Chains<ChainDev> ech;
  scratch::Segments<SegDev> esg;  // the straight segments (behind ech)
  scratch::Place plc;
  // dpr_pin: the host-image entry's pinned staging frame (rows * cols * 4 bytes, on ITS first use), which the kernel reads in
  // place. dpr_queued / spr_queued: a fusion has been queued.
  char* dpr_pin = nullptr;
  bool dpr_queued = false, spr_queued = false;
  std::mutex place_mu;
  std::vector<rebvio_hip_place_db*> place_dbs;
};

namespace {
void release_map(rebvio_hip_map* m, hipEvent_t done_ref = nullptr, bool record_done = true, uint64_t done_token = 0);
void free_cloud_device(rebvio_hip_cloud* cl);
// the map a flushed stream with gyro rotations would continue from (rebvio_hip_ctx::carry) goes back to the pool
inline void drop_carry(rebvio_hip_ctx* c) {
  if (!c->carry) return;
  (void)hipSetDevice(c->device);
  release_map(c->carry, nullptr);
  c->carry = nullptr;
}

// what an entry answers (-10) with for a handle whose context is gone
inline const char* gone_text(const rebvio_hip_map*) { return "the map's context has been destroyed (rebvio_hip_destroy)"; }
inline const char* gone_text(const rebvio_hip_kf_snapshot*) { return "the snapshot's context has been destroyed (rebvio_hip_destroy)"; }
inline const char* gone_text(const rebvio_hip_place_db*) { return "the place database's context has been destroyed (rebvio_hip_destroy)"; }
// Holds the life block of a map, a snapshot or a place database (shared) for as long as it lives - declared at the top of an
// entry, for the rest of it: a rebvio_hip_destroy on another thread waits until the entry has returned instead of freeing the
// context under it (the check alone would leave a window between test and use). dead(): the context is gone already (g_err says
// so); the entry returns -10 at once. A null handle, or one without a life block, counts as dead. say = false: a release, which
// returns nothing and leaves the thread's message alone.
class Alive {
 public:
  template <class Handle>
  explicit Alive(const Handle* h, bool say = true) : hold_(h ? h->life : nullptr) {
    if (hold_) lock_ = std::shared_lock<std::shared_mutex>(hold_->mu);
    dead_ = !hold_ || hold_->dead.load(std::memory_order_acquire);
    if (dead_ && say) g_err = gone_text(h);
  }
  bool dead() const { return dead_; }

 private:
  std::shared_ptr<LifeBlock> hold_;
  std::shared_lock<std::shared_mutex> lock_;
  bool dead_;
};

// Makes a feature's scratch at its first call: one allocation of exactly the bytes its layout measures (scratch_layout.hpp).
template <class Layout, class... Args>
int ensure_scratch(rebvio_hip_ctx* c, Layout& s, Args... args) {
  if (s.base) return 0;
  char* b = nullptr;
  HIPCHK(c->own.device_bytes(&b, Layout().lay(nullptr, args...)));
  s.lay(b, args...);
  return 0;
}

// Snapshots and place databases are listed in their context. At rebvio_hip_destroy every listed handle is still out: its device
// memory goes with the context, the host struct stays as a husk for its release to delete.
template <class Handle, class Buffer>
void leave_husks(std::vector<Handle*>& list, Buffer Handle::*first) {
  for (Handle* h : list) {
    h->own.release();
    h->*first = nullptr;
    h->ctx = nullptr;
  }
  list.clear();
}

// A listed handle's release. While the context lives: off the list (under the list's mutex: a release may come from any thread)
// and its device memory freed (hipFree waits for the kernels that still use it); after rebvio_hip_destroy, which freed it: the husk.
template <class Handle>
void unlist_and_release(std::vector<Handle*> rebvio_hip_ctx::*list, std::mutex rebvio_hip_ctx::*mu, Handle* h) {
  if (!h) return;
  {
    const Alive alive(h, false);
    if (!alive.dead()) {
      rebvio_hip_ctx* c = h->ctx;
      (void)hipSetDevice(c->device);
      {
        std::lock_guard<std::mutex> sl(c->*mu);
        auto& v = c->*list;
        for (size_t i = 0; i < v.size(); ++i)
          if (v[i] == h) {
            v.erase(v.begin() + (std::ptrdiff_t)i);
            break;
          }
      }
      h->own.release();
    }
  }
  delete h;
}

// events of a map may only be waited on once the batch's detect worker has recorded them
inline void wait_enqueued(rebvio_hip_map* m) {
  while (!m->enqueued.load(std::memory_order_acquire)) std::this_thread::yield();
}

size_t part_call_stride(const rebvio_hip_ctx* c) { return (size_t)c->maxblocks * kPartStride; }

// Wait for the track stream by polling: hipStreamQuery holds no runtime lock while it waits, so launches of other threads
// of the process (rebvio::Rebvio's acquisition thread) are not held up behind a blocked hipStreamSynchronize.
int trk_sync(rebvio_hip_ctx* c) {
  for (;;) {
    const hipError_t e = hipStreamQuery(c->s_trk);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) HIPCHK(e);
    std::this_thread::yield();
  }
}

int alloc_map(rebvio_hip_ctx* c, rebvio_hip_map* m) {
  // keyline arrays are padded to the launch grids (256- and 1024-thread workgroups) so kernels may load before checking n
  const size_t M = (size_t)div_up(c->P.keylines_max, 1024) * 1024, Pn = (size_t)c->P.rows * c->P.cols;
  MapDev& d = m->d;
  Owned& own = m->own;
  HIPCHK(own.device(&d.pos, M));
  HIPCHK(own.device(&d.pos_img, M));
  HIPCHK(own.device(&d.mpos_img, M));
  HIPCHK(own.device(&d.grad, M));
  HIPCHK(own.device(&d.mgrad, M));
  HIPCHK(own.device(&d.gnorm, M));
  HIPCHK(own.device(&d.mgnorm, M));
  HIPCHK(own.device(&d.rs, M));
  HIPCHK(own.device(&d.rs_tmp, M));
  HIPCHK(own.device(&d.grad_tmp, M));
  HIPCHK(own.device(&d.id_prev, M));
  HIPCHK(own.device(&d.id_next, M));
  HIPCHK(own.device(&d.match_id, M));
  HIPCHK(own.device(&d.match_fwd, M));
  HIPCHK(own.device(&d.match_kf, M));
  HIPCHK(own.device(&d.matches, M));
  HIPCHK(own.device(&d.fwd_key, M));
  HIPCHK(own.device(&d.residual, M));
  HIPCHK(own.device(&d.mask, Pn, 0xFF));
  HIPCHK(own.device(&d.df, Pn, 0xFF));
  HIPCHK(own.device(&d.unit, M));
  {
    const DfGrid g = df_grid(c->P.rows, c->P.cols);
    const size_t nt = (size_t)g.ntx * g.nty;
    HIPCHK(own.device(&d.tile_cnt, nt, 0));
    HIPCHK(own.device(&d.tile_list, nt * kDfTileCap * 2));
  }
  HIPCHK(own.device(&d.row_start, (size_t)c->P.rows + 1, 0));
  HIPCHK(own.device(&d.st, 1, 0));
  // hipMemset on device memory returns BEFORE the fill has run (tools/memset_probe.hip on this runtime: the call takes 2.5 us, the
  // device finishes 10 us later for 1.2 MB), on the null stream, which the context's non-blocking streams do not wait for. A map
  // the pool grows by while the pipeline is running is handed to the detect kernels microseconds later: without this wait a late
  // fill wiped what they had written - the state record (n = 0), the dense mask, the distance field (every tryVel evaluation a
  // penalty: zero velocity, NaN covariance) - on a few per cent of fresh streams' first frames. (Round 3 saw records of this kind
  // on its 192x144 stream with kernel-bound stop events; the race explains them, that configuration was not re-run.)
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(own.event(&m->ready));
  HIPCHK(own.event(&m->detected));
  HIPCHK(own.event(&m->done));
  return 0;
}

// device arrays and events of a map; the host struct stays (a handle the caller still holds is deleted by its release)
void free_map_device(rebvio_hip_map* m) {
  m->own.release();
  m->d = MapDev{};
  m->canon = MapDev{};
  m->ready = m->detected = m->done = hipEvent_t{};
  m->ctx = nullptr;
}

int alloc_map(rebvio_hip_ctx* c, rebvio_hip_map* m);
rebvio_hip_map* acquire_map(rebvio_hip_ctx* c) {
  std::lock_guard<std::mutex> pool_lk(c->pool_mu);
  // Oldest release first: a map is released in stream order, i.e. before its last consumer (the pair's B-chain) has
  // run; reusing the most recently released one makes the new frame's keyline kernels wait for that consumer.
  rebvio_hip_map* best = nullptr;
  for (auto* m : c->pool)
    if (!m->in_use && (!best || m->release_seq < best->release_seq)) best = m;
  // The streaming drivers release a map when its group of pairs is QUEUED, up to a ring of pairs before the tracker has run it
  // on the device; the frame that reuses it waits (in stream order) for that group. With too few maps the detect stage can
  // only work a few pairs ahead of the tracker and the tracker ends up waiting for its maps: min_pool keeps the reuse distance
  // at two groups and more.
  if (best && (int)c->pool.size() < c->min_pool) best = nullptr;
  if (best) {
    rebvio_hip_map* m = best;
    m->in_use = true;
    m->df_built = false;
    m->raster_order = false;
    m->pre_rotated = false;
    m->gyro_set = false;
    m->kf_flag = false;
    m->promised.store(false, std::memory_order_relaxed);
    m->served_old = false;
    m->n_host = -1;
    m->thr_host = -1.0f;
    m->trk_waited = false;
    m->trk_touched.store(false, std::memory_order_relaxed);  // (its previous life drained before its detection: m->done)
    return m;
  }
  // every pooled map is alive (a caller queues detections faster than it tracks, like the reference's unbounded
  // edge_map_buffer_): grow the pool, ~4 MB per map at 640x480, bounded
  if (c->pool.size() >= 256) return nullptr;
  rebvio_hip_map* m = new rebvio_hip_map;
  m->ctx = c;
  m->life = c->life;
  if (alloc_map(c, m) != 0) {
    free_map_device(m);
    delete m;
    return nullptr;
  }
  c->pool.push_back(m);
  m->in_use = true;
  return m;
}

int fetch_map_state(rebvio_hip_map* m, MapState* out, hipStream_t after) {
  // copy stream: wait for the producer, copy, block the host only on this small transfer
  rebvio_hip_ctx* c = m->ctx;
  wait_enqueued(m);
  HIPCHK(hipStreamWaitEvent(c->s_key, m->ready, 0));
  if (after) {
    if (!c->fetch_ev) HIPCHK(c->own.event(&c->fetch_ev));
    HIPCHK(hipEventRecord(c->fetch_ev, after));
    HIPCHK(hipStreamWaitEvent(c->s_key, c->fetch_ev, 0));
  }
  HIPCHK(hipMemcpyAsync(c->h_st, m->d.st, sizeof(MapState), hipMemcpyDeviceToHost, c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_key));
  *out = *c->h_st;
  m->n_host = out->n;
  m->thr_host = out->threshold;
  return 0;
}

// Every use of a map on the track stream starts with this wait on its detection (+ distance field).
hipError_t trk_wait_ready(hipStream_t s, rebvio_hip_map* m) {
  if (!m->trk_touched.load(std::memory_order_relaxed)) {
    // first use by the tracker: not while a download of an "untouched" map is packing it on the copy stream
    // (rebvio_hip_map_download decides and packs under the same mutex)
    std::lock_guard<std::mutex> dl(m->ctx->dl_mu);
    m->trk_touched.store(true, std::memory_order_release);
  }
  return hipStreamWaitEvent(s, m->ready, 0);
}
// The streaming driver's waits and records, counted (`on`: kOnTrk / kOnScan / kOnKey, the stream s of context c). A wait on an
// event that has completed is not asked about first: the runtime drops such a wait itself (tools/handover_probe.hip: no packet,
// 0.14 us of the caller, as much as the hipEventQuery that would replace it). A record is what costs: 2.9 us between the two
// kernels it stands between and 1.1 - 1.4 us of the launching thread.
enum { kOnTrk = 0, kOnScan = 1, kOnKey = 2 };
hipError_t wait_counted(rebvio_hip_ctx* c, int on, hipStream_t s, hipEvent_t e) {
  c->ho.queued[on].fetch_add(1, std::memory_order_relaxed);
  return hipStreamWaitEvent(s, e, 0);
}
hipError_t record_counted(rebvio_hip_ctx* c, int on, hipStream_t s, hipEvent_t e) {
  c->ho.events[on].fetch_add(1, std::memory_order_relaxed);
  return hipEventRecord(e, s);
}
// The same, once per map and context stream: every wait is a barrier packet of its own between two kernels of the track
// stream (~2 us each on the pair-to-pair critical path); `ready` is recorded once per detection, a second wait adds nothing.
hipError_t trk_wait_ready_once(rebvio_hip_ctx* c, rebvio_hip_map* m) {
  if (m->trk_waited) return hipSuccess;
  m->trk_waited = true;
  return trk_wait_ready(c->s_trk, m);
}

int ensure_size(rebvio_hip_map* m) {
  if (m->n_host >= 0) return 0;
  MapState st;
  return fetch_map_state(m, &st, nullptr);
}

int detect_launch(rebvio_hip_ctx* c, const rebvio_hip_ctx::DetJob& j) {
  rebvio_hip_map* m = j.m;
  const int b = (int)(c->launch_index & 1);
  c->launch_index++;
  ScaleBufs sb = c->sb;
  sb.scale0 = sb.scale1 = nullptr;
  sb.dog = c->dog2[b];
  sb.mag = c->mag2[b];
  sb.a[0] = c->sa2[b][0];  // the third filter's integral images change streams (below): one pair per frame parity
  sb.a[1] = c->sa2[b][1];
  DetectBufs db = c->db;
  db.rowcount = c->rowcount2[b];
  if (j.pin_slot >= 0) {  // host frame: pinned slot -> device staging frame, read by this stream's own kernels only
    launch_copy_from_pinned(c->s_det, c->pin[j.pin_slot], const_cast<void*>(j.img), j.pin_bytes);
    HIPCHK(hipEventRecord(c->pin_ev[j.pin_slot], c->s_det));
  }
  // scans of this frame (s_det); its DoG / gradient buffers were last read by the candidate kernel two frames ago
  if (c->prev_ready[b]) HIPCHK(wait_counted(c, kOnScan, c->s_det, c->prev_ready[b]));
  const void* img = j.img;
  int is_u8 = j.is_u8;
  int fmt = is_u8 ? j.fmt : 0;
  if (is_u8 && c->undist_map) {  // x3 + undistort (rebvio.cpp:43-47); its output was last read by the scans two frames ago
    if (fmt == px::GRAY8)
      launch_front_end_u8(c->s_det, c->K, (const uint8_t*)img, c->undist_map, c->undist_img[b]);
    else  // grey byte of every tap first (cv_bridge MONO8), then x3 + undistort
      launch_front_end_px(c->s_det, c->K, (const uint8_t*)img, fmt, c->undist_map, c->undist_img[b]);
    img = c->undist_img[b];
    is_u8 = 0;
    fmt = 0;
  }
  // The scan stream is the busiest of the three: it hands the frame over after the last ROW pass, the last column pass and
  // the DoG / gradient kernel run at the head of the keyline stream.
  // Their inputs sb.a[] are then read while the scan stream already works on the next frame, hence the pair per parity;
  // the frame after next waits for this frame's `ready` event (prev_ready[b]) above.
  launch_scale_space(c->s_det, c->K, img, is_u8, sb, c->widths, db.rowcount, 1, fmt);
  HIPCHK(record_counted(c, kOnScan, c->s_det, c->ev_scan[b]));
  // keyline extraction + chaining (s_key), overlapping the next frame's scans
  HIPCHK(wait_counted(c, kOnKey, c->s_key, c->ev_scan[b]));
  launch_scale_space(c->s_key, c->K, img, is_u8, sb, c->widths, db.rowcount, 2);
  // the map's previous life: its last consumer on the track stream
  if (m->has_done && m->done_token == 0) {
    HIPCHK(wait_counted(c, kOnKey, c->s_key, m->done_ref ? m->done_ref : m->done));
  } else if (m->has_done && c->q.proven.load(std::memory_order_acquire) >= m->done_token) {
    c->ho.skipped[kOnKey].fetch_add(1, std::memory_order_relaxed);  // the host has read the records that prove it idle
  } else if (m->has_done) {
    // Released with a token the host has not observed yet (rare: the pool hands out the oldest release first). Every consumer of
    // the map was queued before its release and the track stream is in order: an event recorded there now stands for the last.
    c->ho.reuse_fallbacks.fetch_add(1, std::memory_order_relaxed);
    HIPCHK(record_counted(c, kOnTrk, c->s_trk, m->done));
    HIPCHK(wait_counted(c, kOnKey, c->s_key, m->done));
  }
  launch_keylines(c->s_key, c->K, sb, db, m->d, j.det_in, j.det_out, j.prev_st, c->widths, j.mask_static, j.mask_frame);
  HIPCHK(hipGetLastError());
  // distance field of this map, behind its keylines on the same stream (stream order is the dependency)
  launch_df_build(c->s_key, c->K, m->d, j.det_out, true);
  HIPCHK(hipGetLastError());
  HIPCHK(record_counted(c, kOnKey, c->s_key, m->ready));
  c->prev_ready[b] = m->ready;  // (pooled maps and their events live as long as the context)
  return 0;
}

// caller-thread half: takes a pooled map and fixes the servo-state ring slots of this frame (and its detection masks: the
// context's static mask as it is now, mask_frame the caller's per-frame device mask or null)
int detect_prepare(rebvio_hip_ctx* c, const void* img_dev, int is_u8, uint64_t ts, rebvio_hip_ctx::DetJob* job, int fmt = 0,
                   const uint8_t* mask_frame = nullptr) {
  rebvio_hip_map* m = acquire_map(c);
  if (!m) return fail_msg("edge-map pool exhausted (release maps or raise map_pool)", -2);
  m->ts = ts;
  m->df_built = true;
  m->raster_order = true;
  job->m = m;
  job->img = img_dev;
  job->is_u8 = is_u8;
  job->fmt = fmt;
  job->mask_static = c->dmask;
  job->mask_frame = mask_frame;
  job->det_in = c->det + (c->frame_index % kDetRing);
  job->det_out = c->det + ((c->frame_index + 1) % kDetRing);
  job->prev_st = c->last_detected ? c->last_detected->d.st : nullptr;
  c->frame_index++;
  c->last_detected = m;
  return 0;
}

// A detect_launch that failed half way: the frame's map has been taken, the servo ring and last_detected have advanced and some of
// its kernels may be queued. The map goes back to the pool and the context is marked failed (every later push / detect reports
// -8 with this error) - the detector's state is one frame out of step and cannot be trusted.
void detect_failed(rebvio_hip_ctx* c, const rebvio_hip_ctx::DetJob& job) {
  {
    std::lock_guard<std::mutex> lk(c->det_mu);
    if (c->det_error.empty()) c->det_error = g_err.empty() ? std::string("detect launch failed") : g_err;
  }
  release_map(job.m, nullptr);
}

int stage_host_frame(rebvio_hip_ctx* c, const void* img, size_t pitch_bytes, size_t row_bytes, int* slot_out, size_t* bytes_out);

// Detection of one frame, launched by the caller's thread. (Handing the launches to a detect worker thread was measured twice
// and removed: with rebvio::Rebvio in round 2 the acquisition thread's time per frame dropped and the fusion thread's own launches
// slowed down by as much - runtime calls of different threads largely serialise; for the streaming driver in round 3 a burst of
// pushes ran at 10.2-10.7 k frames/s with the worker and at 12.9-13.0 k without it)
// img_dev: the frame in device memory, or (host != null) the device staging frame that a host frame is copied to. A host frame
// (rows of row_bytes, pitch_bytes apart) goes through the pinned ring; detect_launch queues its copy ahead of the scans, on the
// scan stream (stream order is reuse order). fmt: pixel format of a u8 frame (pixel_format.hpp). mask_frame: per-frame detection
// mask in device memory (null: none).
int detect(rebvio_hip_ctx* c, const void* img_dev, int is_u8, int fmt, uint64_t ts, rebvio_hip_map** out, const void* host = nullptr,
           size_t pitch_bytes = 0, size_t row_bytes = 0, const uint8_t* mask_frame = nullptr) {
  {
    std::lock_guard<std::mutex> lk(c->det_mu);
    if (!c->det_error.empty()) return fail_msg(c->det_error.c_str(), -8);
  }
  rebvio_hip_ctx::DetJob job;
  int rc = host ? stage_host_frame(c, host, pitch_bytes, row_bytes, &job.pin_slot, &job.pin_bytes) : 0;
  if (rc) return rc;
  rc = detect_prepare(c, img_dev, is_u8, ts, &job, fmt, mask_frame);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  rc = detect_launch(c, job);
  if (c->dbg) {
    c->t_det_launch += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    c->t_det_n++;
  }
  if (rc) {
    detect_failed(c, job);
    return rc;
  }
  *out = job.m;
  return 0;
}

void rotate_inputs(const rebvio_hip_ctx* c, const float vel[3], const float Rvel[9], const float Rback[9], float vel_r[3],
                   float Rvel_r[9]) {
  // EdgeMap::directedMatch prologue (edge_map.cpp:193-194)
  (void)c;
  const hm::M3 Rb = hm::load3(Rback);
  hm::mulv(Rb, vel, vel_r);
  hm::store3(hm::mul(hm::mul(Rb, hm::load3(Rvel)), hm::transpose(Rb)), Rvel_r);
}

void sum_xrv(const float* h_xrv, int nblocks, float Wx[36], float JtF[6], int* nm) {
  double acc[28];
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  for (int b = 0; b < nblocks; ++b)
    for (int k = 0; k < 28; ++k) acc[k] += (double)h_xrv[(size_t)b * kXrvStride + k];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      Wx[i * 6 + j] = (float)acc[k];
      Wx[j * 6 + i] = (float)acc[k];
      ++k;
    }
  for (int i = 0; i < 6; ++i) JtF[i] = (float)acc[21 + i];
  if (nm) *nm = (int)std::lround(acc[27]);
}

// The speculative LM kernel bets that minimizeVel rejects every step after the first accepted one (track.hip). Where the
// bet fails often - large inter-frame motion: 35 % of the pairs when a 20 Hz stream is replayed in jumps of 1..6 frames - it
// costs more than it saves (measured there: 3.7 % slower than the sequential kernel; 4-5 % faster on consecutive frames;
// break-even near one miss in six). Both kernels give the same bits, so the choice follows the recent miss rate of the
// stream (exponential average over ~16 pairs, known with a lag of two pairs in the streaming driver).
// 1 = k_lm_chain, 2 / 3 = the speculative kernel with its first speculative evaluation at that index: the earliest hypothesis
// the stream's recent accept masks have been supporting (a failed hypothesis costs a roll-back: break-even near one miss in six)
int lm_kernel_choice(const rebvio_hip_ctx* c) {
  if (c->lm_mix) {  // REBVIO_HIP_LM=mix<seed>: a pseudo-random kernel per pair (tests: every sequence of choices gives the same records)
    unsigned x = (unsigned)c->pair_seq * 2654435761u + (unsigned)c->lm_mix * 40503u;
    x ^= x >> 15;
    x *= 2246822519u;
    x ^= x >> 13;
    return 1 + (int)(x % 3u);
  }
  if (!c->lm_spec) return 1;
  if (c->lm_spec_forced) return c->lm_spec_forced_kf;
  if (c->lm_miss_ema < 0.17f) return 2;
  if (c->lm_miss3_ema < 0.17f) return 3;
  return 1;
}
void note_accept_mask(rebvio_hip_ctx* c, int mask) {
  const float miss = (mask >> 1) != 0 ? 1.0f : 0.0f;  // an accept after the second evaluation = a failed hypothesis
  c->lm_miss_ema += (miss - c->lm_miss_ema) * (1.0f / 16.0f);
  const float miss3 = (mask >> 2) != 0 ? 1.0f : 0.0f;
  c->lm_miss3_ema += (miss3 - c->lm_miss3_ema) * (1.0f / 16.0f);
}

void lm_to_out(const LmState& s, float vel[3], float Rvel[9], float* F, int* mask, float* srm) {
  for (int i = 0; i < 3; ++i) vel[i] = s.vel[i];
  hm::M3 J;
  J.a[0][0] = s.JtJ[0]; J.a[1][1] = s.JtJ[1]; J.a[2][2] = s.JtJ[2];
  J.a[0][1] = J.a[1][0] = s.JtJ[3];
  J.a[0][2] = J.a[2][0] = s.JtJ[4];
  J.a[1][2] = J.a[2][1] = s.JtJ[5];
  hm::store3(hm::invert3(J), Rvel);  // _Rvel = invert(JtJ) (core.cpp:186)
  if (F) *F = s.F;
  if (mask) *mask = s.accept_mask;
  if (srm) *srm = s.sigma_rho_min;
}

// Start state of minimizeVel from vel0: the constant zero state, or vel0 uploaded into c->lm[0] on the track stream.
LmState* start_lm_state(rebvio_hip_ctx* c, const float vel0[3]) {
  if (vel0[0] == 0.f && vel0[1] == 0.f && vel0[2] == 0.f) return c->lm_zero;
  LmState init;
  std::memset(&init, 0, sizeof(init));
  for (int i = 0; i < 3; ++i) init.vel[i] = vel0[i];
  c->h_lm[1] = init;
  (void)hipMemcpyAsync(c->lm, &c->h_lm[1], sizeof(LmState), hipMemcpyHostToDevice, c->s_trk);
  return c->lm;
}

// minimizeVel on the track stream: histogram must already be in c->hist and residuals zeroed.
void enqueue_lm_chain(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const float vel0[3]) {
  LmState* first = start_lm_state(c, vel0);
  const int calls = (int)c->P.iterations + 1;
  const size_t cs = part_call_stride(c);
  prof_group_begin(c->s_trk, "k_try_vel", calls);
  for (int i = 0; i < calls; ++i)
    launch_try_vel(c->s_trk, c->K, om->d, nm->d, 1, i, i == calls - 1, i ? c->lm + i : first, c->lm + i + 1,
                   i ? c->part + (size_t)(i - 1) * cs : c->part, c->part + (size_t)i * cs, c->hist, 0);
  prof_group_end(c->s_trk);
}

// minimizeVel + forwardMatch + extRotVel of one pair on the track stream (rebvio.cpp:167-177); results land in `slot`.
// Default: the persistent kernel (one launch); REBVIO_HIP_LM=percall selects the per-evaluation kernels, which compute
// identical bits (same per-keyline code, same record order).
// xrv_dst: where the extRotVel block records go - the pinned slot's tail (per-pair API: the host sums them) or device
// memory (streaming driver: the device glue sums them).
// ga.lm != null: the pair's glue runs on the device behind the extRotVel sums (streaming driver).
uint32_t next_stamp(uint32_t* counter) {
  if (++*counter == 0u) ++*counter;  // (zero is what a never-written record holds)
  return *counter;
}
constexpr int kStaleRecord = -12;
const char* const kStaleRecordMsg = "a pair's record was read before the device had written it (sequence stamp mismatch)";

// A result slot counts once its stamp AND its checksum fit: the words are re-read on every try (writes to host memory may arrive
// out of order; a torn read fails the sum and is simply repeated).
bool slot_complete(const PairSlot* slot, uint32_t seq) {
  static_assert(offsetof(PairSlot, seq) == sizeof(LmState) + 2 * sizeof(MapState), "PairSlot::sum covers lm, new_st, old_st");
  const volatile unsigned* w = reinterpret_cast<const volatile unsigned*>(slot);
  if (*reinterpret_cast<const volatile unsigned*>(&slot->seq) != seq) return false;
  unsigned x = 0u;
  for (size_t i = 0; i < offsetof(PairSlot, seq) / sizeof(unsigned); ++i) x ^= w[i];
  return (x ^ seq) == *reinterpret_cast<const volatile unsigned*>(&slot->sum);
}

// Waits for a pair's host records (per-pair API: the result slot and the extRotVel block records behind it) by polling their
// sequence stamps. The stream is queried now and then so that a device-side failure ends the wait with its error; after two
// seconds without the stamps the stream is synchronised and the stamps decide (-12).
int poll_pair_records(rebvio_hip_ctx* c, const PairSlot* slot, uint32_t seq) {
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  bool synced = false;
  // one step of waiting: 0 keep polling, < 0 error. The stream is queried now and then so that a device-side failure ends the wait
  // with its error; after two seconds the stream is synchronised and the records get one last look.
  auto wait_step = [&]() -> int {
    if (synced) return fail_msg(kStaleRecordMsg, kStaleRecord);
    __builtin_ia32_pause();
    if ((++spins & 0x3FFFu) != 0u) return 0;
    const hipError_t q = hipStreamQuery(c->s_trk);
    if (q != hipSuccess && q != hipErrorNotReady) return fail("track stream", q);
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      const hipError_t e = hipStreamSynchronize(c->s_trk);
      if (e != hipSuccess) return fail("track stream", e);
      synced = true;
    }
    return 0;
  };
  while (!slot_complete(slot, seq)) {
    const int e = wait_step();
    if (e) return e;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  const int nb = std::min(div_up(std::max(slot->new_st.n, 0), 256), c->maxblocks);
  for (int b = 0; b < nb; ++b) {
    const volatile unsigned* w = reinterpret_cast<const volatile unsigned*>(slot->xrv + (size_t)b * kXrvStride);
    auto rec_ok = [&]() -> bool {
      if (w[kXrvStride - 1] != seq) return false;
      unsigned x = 0u;
      for (int k = 0; k < 28; ++k) x ^= w[k];
      return (x ^ seq) == w[kXrvStride - 2];
    };
    while (!rec_ok()) {
      const int e = wait_step();
      if (e) return e;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// 0, or -9 once a persistent LM kernel of lane c has set its sticky time-out flag: the error names what the kernel reports and
// the other users of the device's persistent kernels (residency_describe; owner: the context or batch that launched it).
int lm_timed_out(const rebvio_hip_ctx* c, int device, const void* owner, const char* who) {
  if (!*c->lm_bar_err) return 0;
  const int* e = c->lm_bar_err;
  char msg[320];
  std::snprintf(msg, sizeof(msg),
                "%spersistent LM kernel: record exchange timed out (workgroup %d/%d thread %d waited for tag %u, last saw tag %u; "
                "tags issued so far %u); ",
                who, e[1], e[6], e[2], (unsigned)e[3], (unsigned)e[4], c->lm_tag_base);
  return fail_msg((std::string(msg) + residency_describe(device, owner)).c_str(), -9);
}

// The exchange tags one persistent LM launch of lane c takes (the speculative kernel numbers repeated evaluations in a second
// range). Tags must stay unique and non-zero: before the sequence could wrap it restarts on clean exchange words.
void advance_lm_tags(rebvio_hip_ctx* c, int calls) {
  c->lm_tag_base += 2u * ((unsigned)calls + 1u);
  if (c->lm_tag_base > 0xFFFFFF00u) {
    (void)hipMemsetAsync(c->lm_xch, 0, lm_xch_words(c->maxblocks) * sizeof(unsigned long long), c->s_trk);
    c->lm_tag_base = 0;
  }
}

int enqueue_pair_lm(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const float vel0[3], PairSlot* slot, float* xrv_dst,
                    const GlueArgs& ga_in) {
  const int calls = (int)c->P.iterations + 1;
  GlueArgs ga = ga_in;
  c->last_stamp = next_stamp(&c->stamp_seq);
  ga.seq = c->last_stamp;
  if (c->forge_stamp) {  // test hook: what a record looks like when it is read before its pair wrote it
    ga.seq ^= 0x40000000u;
    c->forge_stamp = false;
  }
  if (!c->lm_persistent) {
    enqueue_lm_chain(c, om, nm, vel0);
    launch_ext_rot_vel(c->s_trk, c->K, om->d, nm->d, 1, 1, calls, c->lm + calls, c->lm + calls + 1,
                       c->part + (size_t)(calls - 1) * part_call_stride(c), xrv_dst, vel0, slot, c->hist, ga.seq);
    if (ga.lm) launch_pair_glue(c->s_trk, nm->d, ga);
    return 0;
  }
  {
    const int rc = lm_timed_out(c, c->device, c, "");
    if (rc) return rc;
  }
  if (!c->residency_registered) {  // (the lane contexts of a batch never come here: the batch registers for them)
    residency_add(c->device, c, (c->K.kmax + c->lm_threads - 1) / c->lm_threads);
    c->residency_registered = true;
  }
  LmState* first = start_lm_state(c, vel0);
  if (c->lm_stamps && c->lm_stamps[0]) {  // stamps of the previous launch (the caller has synchronised on its slot since)
    // the buffer may be half rewritten by a launch that is already running (streaming driver): take a snapshot and use it
    // only if it is monotonic and spans less than a millisecond
    const bool spec = c->lm_stamps[0] == 1ull;  // k_lm_chain_spec: stamps 1..14, [0] is a marker
    const int i0 = spec ? 1 : 0;
    const int ns = spec ? 16 : 3 + calls * 6;
    unsigned long long snap[64];
    for (int i = 0; i < ns; ++i) snap[i] = c->lm_stamps[i];
    bool sane = snap[ns - 1] > snap[i0] && snap[ns - 1] - snap[i0] < 100000ull;
    for (int i = i0 + 1; i < ns && sane; ++i) sane = snap[i] >= snap[i - 1];
    if (sane) {
      for (int i = i0 + 1; i < ns; ++i) c->lm_stamp_acc[i] += (double)(snap[i] - snap[i - 1]) * 0.01;
      c->lm_stamp_n++;
      c->lm_stamp_spec = spec;
    }
  }
  launch_lm_chain(c->s_trk, c->K, om->d, nm->d, calls, lm_kernel_choice(c), first, c->lm + calls + 1, c->lm_xch, c->lm_tag_base, c->lm_bar_err, c->hist,
                  xrv_dst, slot, c->hist, c->lm_stamps, c->lm_threads, ga);
  advance_lm_tags(c, calls);
  return 0;
}

// Host frame -> pinned ring slot (plain memcpy) -> asynchronous copy on the scan stream. A copy straight from pageable
// memory is staged inside the runtime, which stays busy for the whole transfer and stalls the launches of the tracking
// thread of rebvio::Rebvio (measured: second half of the pair step 215 us -> 47 us); it also must not outlive the caller's
// buffer. The device staging frames are read by the scan stream's own kernels only, so stream order is reuse order.
// Host half: frame -> pinned ring slot. The copy to the device and the slot's reuse event are queued by the frame's
// detect_launch, in the same call, in stream order with its kernels.
int stage_host_frame(rebvio_hip_ctx* c, const void* img, size_t pitch_bytes, size_t row_bytes, int* slot_out, size_t* bytes_out) {
  if (!c->pin[0]) {
    for (int i = 0; i < rebvio_hip_ctx::kPin; ++i) {
      HIPCHK(c->own.pinned(&c->pin[i], (size_t)c->P.rows * c->P.cols * sizeof(float) + 16, false));  // (+16: copied in whole 16-byte units)
      HIPCHK(c->own.event(&c->pin_ev[i]));
    }
  }
  const int ps = (int)(c->pin_next++ % rebvio_hip_ctx::kPin);
  if (c->pin_used[ps]) HIPCHK(hipEventSynchronize(c->pin_ev[ps]));  // its previous copy has left the slot
  uint8_t* dst = c->pin[ps];
  const uint8_t* src = static_cast<const uint8_t*>(img);
  if (pitch_bytes == row_bytes)
    std::memcpy(dst, src, (size_t)c->P.rows * row_bytes);
  else
    for (int r = 0; r < c->P.rows; ++r) std::memcpy(dst + (size_t)r * row_bytes, src + (size_t)r * pitch_bytes, row_bytes);
  c->pin_used[ps] = true;
  *slot_out = ps;
  *bytes_out = (size_t)c->P.rows * row_bytes;
  return 0;
}

// Device staging frame of a host u8 frame of pixel format fmt. MONO8: img8_dev (rows * cols bytes). Wider formats: img_dev, the
// fp32 host frame's staging (rows * cols * 4 bytes + 16, as large as the widest format), allocated with the context - a colour
// stream allocates nothing, and nothing grows or stalls the frames in flight when the format changes. Both are written and read
// by the scan stream's own operations only, so stream order is reuse order, whichever format each frame has.
void* u8_staging(rebvio_hip_ctx* c, int fmt) { return fmt == px::GRAY8 ? (void*)c->img8_dev : (void*)c->img_dev; }

// Argument checks of the *_px entries, before anything touches the device. host: pitch_bytes is checked (0 = dense).
int check_px(const rebvio_hip_ctx* c, const char* who, const void* frame, int fmt, bool host, size_t pitch_bytes) {
  char buf[192];
  if (!px::valid(fmt)) {
    std::snprintf(buf, sizeof(buf), "%s: unknown pixel format %d (REBVIO_HIP_PX_GRAY8 .. REBVIO_HIP_PX_UYVY)", who, fmt);
    return fail_msg(buf, -3);
  }
  if (!frame) {
    std::snprintf(buf, sizeof(buf), "%s: null frame", who);
    return fail_msg(buf, -3);
  }
  if (px::needs_even_cols(fmt) && (c->P.cols & 1)) {
    std::snprintf(buf, sizeof(buf), "%s: YUYV / UYVY frames need an even width (cols = %d)", who, c->P.cols);
    return fail_msg(buf, -3);
  }
  const size_t rowb = (size_t)c->P.cols * px::bytes_per_pixel(fmt);
  if (host && pitch_bytes != 0 && pitch_bytes < rowb) {
    std::snprintf(buf, sizeof(buf), "%s: pitch_bytes %zu below a row's %zu bytes (cols * bytes per pixel)", who, pitch_bytes, rowb);
    return fail_msg(buf, -3);
  }
  return 0;
}

}  // namespace

extern "C" {

int rebvio_hip_abi_version(void) { return REBVIO_HIP_ABI_VERSION; }
const char* rebvio_hip_last_error(void) { return g_err.c_str(); }

void rebvio_hip_default_params(rebvio_hip_params* p, int rows, int cols) {
  std::memset(p, 0, sizeof(*p));
  p->rows = rows; p->cols = cols;
  const float fx = 458.654, fy = 457.296;  // camera.hpp:26-30
  p->fm = 0.5 * (fx + fy);
  p->cx = 367.215; p->cy = 248.375;
  p->keylines_ref = 12000; p->keylines_max = 16000;
  p->pos_neg_threshold = 0.4; p->dog_threshold = 0.095259868922420; p->threshold = 0.01; p->gain = 5e-7;
  p->max_threshold = 0.5; p->min_threshold = 0.005;
  p->search_range = 40.0; p->reweight_distance = 2.0; p->match_treshold = 0.5;
  p->min_match_threshold = 0; p->iterations = 5; p->global_min_matches_threshold = 500;
  p->pixel_uncertainty = 1; p->quantile_cutoff = 0.9; p->quantile_num_bins = 100; p->reshape_q_abs = 1e-4;
  p->pixel_uncertainty_match = 2.0; p->match_threshold_norm = 1.0; p->match_threshold_angle = 45.0;
  p->regularization_threshold = 0.5;
  p->gyro_std_dev = 1.6968e-04; p->gyro_bias_std_dev = 1.9393e-05;
  p->device_id = 0; p->map_pool = 0;
}

void rebvio_hip_reset_state(rebvio_hip_ctx* c) {
  // While the streaming driver has pairs in flight the filter state lives on the device: they are completed first (their records
  // stay available through rebvio_hip_next_record), so that no harvested record writes the old state back over the reset one.
  if (c->q.count || !c->frames.empty()) (void)rebvio_hip_flush(c);
  drop_carry(c);  // a reset ends a stream with gyro rotations too: the next frame pushed is a first frame
  c->kf_pending = false;  // a keyframe request belongs to the stream it was made in
  c->plain_flushed = false;  // ... and whatever it is pushed with is a first frame's rotation: ignored, as on a fresh context
  c->wbg_shadow_valid = false;  // (the next stream's first pair uploads this state and starts the shadow from it)
  c->Bg[0] = c->Bg[1] = c->Bg[2] = 0.f;
  c->RGBias = hm::identity3();
  c->RGyro = hm::identity3();
  c->W_Bg = hm::invert3(hm::diag3(100.0f));  // W_Bg{invert(100.0*RGBias)} (types/imu.hpp:181)
}

int rebvio_hip_get_gyro_state(rebvio_hip_ctx* c, float Bg[3], float W_Bg[9]) {
  for (int i = 0; i < 3; ++i) Bg[i] = c->Bg[i];
  hm::store3(c->W_Bg, W_Bg);
  return 0;
}

int rebvio_hip_set_gyro_state(rebvio_hip_ctx* c, const float Bg[3], const float W_Bg[9]) {
  // While the streaming driver has pairs or frames in flight the filter state lives on the device (and the next pair's first
  // rotation has already been applied with it): it can only be replaced between streams.
  if (c->q.count || !c->frames.empty())
    return fail_msg("set_gyro_state: the streaming driver has frames in flight (rebvio_hip_flush first)", -7);
  for (int i = 0; i < 3; ++i) c->Bg[i] = Bg[i];
  c->W_Bg = hm::load3(W_Bg);
  c->wbg_shadow_valid = false;  // (the next stream's first pair uploads this state and starts the shadow from it)
  return 0;
}

// The detection parameters a context may be created with. The gradient gate of the candidate test is
//   !(g2 < gradient_threshold_squared),   gradient_threshold_squared = (thr * 765 * dog_threshold)^2 in fp32,
// and thr never falls below lo = min(min_threshold, max_threshold) with the servo on (gain > 0: both clamps apply on every frame),
// threshold itself otherwise. A bound of zero lets a zero gradient through (theta2 / 0 is NaN and fabs(NaN) > 0.5 is false), the
// keyline gets a NaN position, and the reference's joinEdges indexes its mask with it (edge_detector.cpp:125-165) - so such
// parameters are refused here, before any device is touched. Evaluated as the kernels spell it (detect.hip).
static int check_detection_params(const rebvio_hip_params* p) {
  const float six[6] = {p->pos_neg_threshold, p->dog_threshold, p->threshold, p->gain, p->min_threshold, p->max_threshold};
  for (float v : six)
    if (!std::isfinite(v))
      return fail_msg("pos_neg_threshold, dog_threshold, threshold, gain, min_threshold and max_threshold must be finite", -3);
  if (!(p->pos_neg_threshold >= 0.0f)) return fail_msg("pos_neg_threshold must be >= 0", -3);
  const volatile float lo = p->gain > 0 ? std::min(p->min_threshold, p->max_threshold) : p->threshold;
  const volatile float g = lo * kMaxImageValue * p->dog_threshold;
  const volatile float gradient_threshold_squared = g * g;
  if (!(gradient_threshold_squared > 0.0f))
    return fail_msg(p->gain > 0
                        ? "(min(min_threshold, max_threshold) * 765 * dog_threshold)^2 must be > 0 in fp32 (gain > 0): the gradient "
                          "gate could not reject a zero gradient"
                        : "(threshold * 765 * dog_threshold)^2 must be > 0 in fp32 (gain <= 0): the gradient gate could not reject "
                          "a zero gradient",
                    -3);
  return 0;
}

// The field kernels walk r in [-(df_nr >> 1), df_nr >> 1) with df_nr = 2 * (int)search_range: the half is the truncated range on
// both sides. The reference walks `for (int r = -search_range_; r < search_range_; ++r)` with the float itself as the upper bound
// (core.hpp:49), one step more for a fractional range (7.5: r = -7 .. 7 against -7 .. 6). The two agree for a whole number only, so
// anything else is refused here, before any device is touched. (A float of 2^23 or more has no fraction; the size checks take it.)
static int check_search_range(const rebvio_hip_params* p) {
  const float s = p->search_range;
  if (!std::isfinite(s) || (std::fabs(s) < 8388608.0f && s != (float)(int)s))
    return fail_msg("search_range must be a whole number of pixels (the distance field of a fractional range would miss the "
                    "reference's last step)", -3);
  return 0;
}

int rebvio_hip_create(const rebvio_hip_params* p, rebvio_hip_ctx** out) {
  *out = nullptr;
  if (int rc = check_search_range(p)) return rc;
  if (p->rows < 32 || p->cols < 32) return fail_msg("rows/cols must be >= 32", -3);
  if (p->cols > 4096) return fail_msg("cols > 4096 unsupported", -3);
  if ((size_t)(p->rows + 12) * 16 * sizeof(float) > 160 * 1024 || (size_t)(p->cols + 3 + 8) * 4 * sizeof(float) > 160 * 1024)
    return fail_msg("image too large for the LDS-staged scan strips (rows <= 2548)", -3);
  if (p->quantile_num_bins > 128 || p->quantile_num_bins < 1) return fail_msg("quantile_num_bins must be in 1..128", -3);
  if ((int)p->iterations + 2 > 15) return fail_msg("iterations too large", -3);
  const int nr = 2 * (int)p->search_range;
  if (nr < 2 || (long long)p->keylines_max * nr >= (1ll << kDfSeqBits) || (int)p->search_range > 255)
    return fail_msg("keylines_max * 2*search_range must stay below 2^23", -3);
  if (p->keylines_max < 1 || div_up(p->keylines_max, 256) > kMaxRecBlocks)
    return fail_msg("keylines_max must be in 1..65536 (the LM reduction stages at most 256 record groups of 256 keylines)", -3);
  if (!(p->pixel_uncertainty_match >= 0.0f) || p->search_range + 2.0f * p->pixel_uncertainty_match + 2.0f > 260.0f)
    return fail_msg("search_range + 2 * pixel_uncertainty_match must be at most 258 (probe sequence buffer)", -3);
  if (int rc = check_detection_params(p)) return rc;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail_msg("no HIP device present: the gfx950 backend has no CPU fallback", -4);
  if (p->device_id < 0 || p->device_id >= ndev) return fail_msg("device_id out of range", -3);
  HIPCHK(hipSetDevice(p->device_id));

  rebvio_hip_ctx* c = new rebvio_hip_ctx;
  struct Guard {  // every early return below (HIPCHK, fail_msg) frees what was allocated so far
    rebvio_hip_ctx* c;
    ~Guard() {
      if (c) rebvio_hip_destroy(c);
    }
  } guard{c};
  c->P = *p;
  c->device = p->device_id;
  KParams& K = c->K;
  K.rows = p->rows; K.cols = p->cols; K.fm = p->fm; K.cx = p->cx; K.cy = p->cy;
  K.kmax = p->keylines_max; K.kref = p->keylines_ref;
  K.pos_neg_threshold = p->pos_neg_threshold; K.dog_threshold = p->dog_threshold; K.gain = p->gain;
  K.max_threshold = p->max_threshold; K.min_threshold = p->min_threshold;
  K.search_range = p->search_range; K.reweight_distance = p->reweight_distance; K.match_treshold = p->match_treshold;
  K.min_match_threshold = p->min_match_threshold;
  K.pixel_uncertainty = p->pixel_uncertainty; K.quantile_cutoff = p->quantile_cutoff;
  K.quantile_num_bins = p->quantile_num_bins; K.reshape_q_abs = p->reshape_q_abs;
  K.pixel_uncertainty_match = p->pixel_uncertainty_match; K.match_threshold_norm = p->match_threshold_norm;
  K.cang_min_edge = std::cos(p->match_threshold_angle * M_PI / 180.0);  // edge_map.cpp:104
  K.regularization_threshold = p->regularization_threshold;
  K.nseg = div_up(p->cols, 64);
  K.df_nr = nr;

  // FastGaussian widths (scale_space.cpp:14-41,186)
  float st0 = 0, st1 = 0;
  hm::kovesi_widths(3.56359, 3, c->widths[0], &st0);
  hm::kovesi_widths(st0 * 1.2599, 3, c->widths[1], &st1);
  for (int f = 0; f < 2; ++f)
    for (int k = 0; k < 3; ++k)
      if (c->widths[f][k] < 3 || c->widths[f][k] > 11) return fail_msg("unexpected box width", -5);
  float recip[128], pinv[75];
  recip[0] = 0.f;
  for (int n = 1; n < 128; ++n) recip[n] = (float)(1.0 / (double)(float)n);
  hm::plane_fit_pinv(pinv);
  upload_tables(recip, pinv);

  // the tracking chain is the serial dependency of the pipeline: highest priority; the atomics-bound distance field is
  // needed one frame later: lowest
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  int prio_mid = (prio_least + prio_greatest) / 2;
  if (const char* e = std::getenv("REBVIO_HIP_PRIO"))  // "flat": every stream at the default priority (diagnostic, several contexts per GPU)
    if (std::strcmp(e, "flat") == 0) prio_least = prio_greatest = prio_mid = 0;
  if (t_adopt_streams) {
    c->s_det = t_adopt_streams->s_det;
    c->s_key = t_adopt_streams->s_key;
    c->s_trk = t_adopt_streams->s_trk;
    c->owns_streams = false;
  } else {
    HIPCHK(c->own.stream(&c->s_det, hipStreamNonBlocking, prio_mid));
    // one stream per priority class: the runtime pools hardware queues per class (GPU_MAX_HW_QUEUES each) and lets streams of
    // a class share a queue once the pool is full, so two of our streams in one class can end up serialised behind each
    // other depending on what else the process created (measured with extra torch streams: 9.3k -> 7.0k frames/s)
    HIPCHK(c->own.stream(&c->s_key, hipStreamNonBlocking, prio_least));
    HIPCHK(c->own.stream(&c->s_trk, hipStreamNonBlocking, prio_greatest));
    // Three streams per context (scans | keylines + distance field | tracking), deliberately not more: on this runtime every
    // additional stream of the process slowed the whole pipeline (measured, same code: 3 streams 9.3k frames/s, 4 streams
    // 9.2k, 5 streams 9.1k; creating a sixth, even unused, 2.6k). The rare copies of the synchronous API ride on the keyline stream.
  }
  const size_t Pn = (size_t)p->rows * p->cols;
  // the integral-image buffers have a row pitch of cols rounded up to 4 floats (the scans move 16-byte vectors); every
  // other per-pixel array is dense
  const size_t Pp = (size_t)p->rows * ((p->cols + 3) & ~3);
  for (int f = 0; f < 2; ++f) {
    HIPCHK(c->own.device(&c->sb.a[f], Pp));
    HIPCHK(c->own.device(&c->sb.b[f], Pp));
  }
  // (DoG / gradient buffers have the size of an integral image, padded pitch: a batch's fused path keeps the third pass's
  // integral images of a step parity in them)
  HIPCHK(c->own.device(&c->sb.dog, Pp));
  HIPCHK(c->own.device(&c->sb.mag, Pp));
  HIPCHK(c->own.device(&c->db.stash, Pn));
  HIPCHK(c->own.device(&c->db.bits, (size_t)p->rows * K.nseg));
  HIPCHK(c->own.device(&c->db.rowcount, (size_t)p->rows, 0));
  c->dog2[0] = c->sb.dog;
  c->mag2[0] = c->sb.mag;
  c->rowcount2[0] = c->db.rowcount;
  for (auto& e : c->ev_scan) HIPCHK(c->own.event(&e));
  for (int f = 0; f < 2; ++f) {
    c->sa2[0][f] = c->sb.a[f];
    HIPCHK(c->own.device(&c->sa2[1][f], Pp));
  }
  for (int i = 1; i < kDetPar; ++i) {
    HIPCHK(c->own.device(&c->dog2[i], Pp));
    HIPCHK(c->own.device(&c->mag2[i], Pp));
    HIPCHK(c->own.device(&c->rowcount2[i], (size_t)p->rows, 0));
  }
  HIPCHK(c->own.device(&c->det, kDetRing + 1));
  DetState d0[kDetRing + 1];
  for (int i = 0; i < kDetRing + 1; ++i) {
    d0[i].threshold = p->threshold;       // config_->threshold
    d0[i].count = 0;                      // keylines_count_(0) (edge_detector.cpp:18)
    d0[i].auto_threshold = p->threshold;  // auto_threshold_(config_->threshold) (edge_detector.cpp:20)
    d0[i].pad = 0;
  }
  HIPCHK(hipMemcpy(c->det, d0, sizeof(d0), hipMemcpyHostToDevice));
  HIPCHK(c->own.device_bytes(&c->img_dev, Pn * sizeof(float) + 16));  // (+16: host frames arrive in whole 16-byte units)
  HIPCHK(c->own.device(&c->img8_dev, Pn + 16));
  HIPCHK(c->own.device(&c->aos_dev, (size_t)p->keylines_max));
  HIPCHK(c->own.device(&c->scratch_i, 2 * Pn));

  c->maxblocks = div_up(p->keylines_max, 1024) * 4;  // record groups of 256 keylines, padded to whole 1024-thread workgroups
  // [2 parity slots][record groups][kPartStride] + the final-velocity broadcast words
  HIPCHK(c->own.device(&c->lm_xch, lm_xch_words(c->maxblocks), 0));  // tag 0 = never published
  HIPCHK(c->own.pinned(&c->lm_bar_err, 8, true));
  if (std::getenv("REBVIO_HIP_LM_STAMPS")) {
    HIPCHK(c->own.pinned(&c->lm_stamps, 64, true));
    K.dbg = c->lm_stamps;
    if (std::getenv("REBVIO_HIP_DM_STATS")) {
      c->dm_stats_words = 16 * (size_t)(p->keylines_max / 8 + 130);
      HIPCHK(c->own.device(&c->dm_stats, c->dm_stats_words, 0));
      K.dm_stats = c->dm_stats;
    }
  }
  // REBVIO_HIP_LM = percall (one kernel per evaluation) | seq (persistent kernel, one evaluation per exchange round) |
  // anything else / unset: persistent kernel with the speculative reject chain (track.hip, k_lm_chain_spec)
  if (const char* e = std::getenv("REBVIO_HIP_LM")) {
    c->lm_persistent = std::strcmp(e, "percall") != 0;
    c->lm_spec = std::strcmp(e, "seq") != 0;
    c->lm_spec_forced = std::strcmp(e, "spec") == 0 || std::strcmp(e, "spec3") == 0;
    c->lm_spec_forced_kf = std::strcmp(e, "spec3") == 0 ? 3 : 2;
    if (std::strncmp(e, "mix", 3) == 0) c->lm_mix = std::max(1, std::atoi(e + 3));
  }
  HIPCHK(c->own.device(&c->lm, 16, 0));
  HIPCHK(c->own.device(&c->part, (size_t)(kMaxLmCalls + 1) * part_call_stride(c), 0));
  HIPCHK(c->own.device(&c->xrv_part, (size_t)c->maxblocks * kXrvStride));
  HIPCHK(c->own.device(&c->hist, 128, 0));
  HIPCHK(c->own.device(&c->lm_zero, 1, 0));
  for (int i = 0; i < rebvio_hip_ctx::kSlots; ++i) {
    HIPCHK(c->own.pinned_bytes(&c->slot[i], sizeof(PairSlot) + (size_t)c->maxblocks * kXrvStride * sizeof(float), true));
    HIPCHK(c->own.pinned(&c->rec[i], 1, true));
    HIPCHK(c->own.event(&c->q.slot_ev[i]));
  }
  HIPCHK(c->own.device(&c->fscratch, 64));
  HIPCHK(c->own.device(&c->glue_dev, rebvio_hip_ctx::kSlots, 0));
  HIPCHK(c->own.device(&c->glue_stage, rebvio_hip_ctx::kSlots, 0));
  HIPCHK(c->own.device(&c->gstate, 2, 0));
  HIPCHK(c->own.pinned(&c->h_gstate, 2, false));
  if (const char* l = std::getenv("REBVIO_HIP_LEAD")) c->lead = std::min(12, std::max(3, std::atoi(l)));
  if (const char* g = std::getenv("REBVIO_HIP_GROUP")) c->group = std::min(6, std::max(1, std::atoi(g)));
  if (const char* e = std::getenv("REBVIO_HIP_HANDOVER")) c->handover_events = std::strcmp(e, "events") == 0;
  if (const char* e = std::getenv("REBVIO_HIP_LM_THREADS")) {
    const int v = std::atoi(e);
    if (v == 256 || v == 512 || v == 1024) c->lm_threads = v;
  }
  if (const char* e = std::getenv("REBVIO_HIP_DM_HEAD"))  // directedMatch head form (track.hip, dm_head_wide): thread | wide; default by map size
    c->dm_head_form = dm_form_by_name(e);
  HIPCHK(c->own.pinned(&c->h_lm, 2, false));
  HIPCHK(c->own.pinned(&c->h_part, part_call_stride(c), false));
  HIPCHK(c->own.pinned(&c->h_xrv, (size_t)c->maxblocks * kXrvStride, false));
  HIPCHK(c->own.pinned(&c->h_st, 2, false));
  HIPCHK(c->own.pinned(&c->h_f, 64, false));

  int pool = p->map_pool > 0 ? p->map_pool : 6;
  if (pool < 4) pool = 4;
  for (int i = 0; i < pool; ++i) {
    rebvio_hip_map* m = new rebvio_hip_map;
    m->ctx = c;
    m->life = c->life;
    c->pool.push_back(m);
    int rc = alloc_map(c, m);
    if (rc) return rc;
  }
  rebvio_hip_reset_state(c);
  c->dbg = std::getenv("REBVIO_HIP_DEBUG") != nullptr;
  if (const char* e = std::getenv("REBVIO_HIP_GYRO_PRE")) c->gyro_pre_on = e[0] != '0';
  HIPCHK(hipDeviceSynchronize());
  guard.c = nullptr;
  *out = c;
  return 0;
}

void rebvio_hip_destroy(rebvio_hip_ctx* c) {
  if (!c) return;
  // Map handles the caller still holds outlive the context as inert husks: every map entry point checks `dead`, and the
  // husk is deleted by its rebvio_hip_map_release. The lock serialises this against a release running on another thread.
  const std::shared_ptr<LifeBlock> life = c->life;
  std::unique_lock<std::shared_mutex> life_lk(life->mu);
  residency_remove(c->device, c);
  (void)hipSetDevice(c->device);
  if (std::getenv("REBVIO_HIP_DEBUG") && c->t_begin_n)
    std::fprintf(stderr, "[rebvio_hip] track_pair_begin over %llu pairs (us): enqueue %.1f  wait for the first half %.1f\n",
                 (unsigned long long)c->t_begin_n, c->t_begin_enq / c->t_begin_n, c->t_begin_wait / c->t_begin_n);
  (void)hipDeviceSynchronize();
  {
    std::lock_guard<std::mutex> g(g_prof.mu);
    g_prof.drain();
  }
  // maps the streaming driver still holds are the library's own, not the caller's
  for (auto* m : c->frames) m->in_use = false;
  if (c->carry) c->carry->in_use = false;
  life->dead.store(true, std::memory_order_release);
  for (auto* m : c->pool) {
    free_map_device(m);
    if (!m->in_use) delete m;  // (else: a handle is still out; its release deletes the husk)
  }
  c->pool.clear();
  for (auto* cl : c->clouds) {
    free_cloud_device(cl);
    if (!cl->in_use) delete cl;  // (else: the handle is still out; its release deletes the husk)
  }
  leave_husks(c->snaps, &rebvio_hip_kf_snapshot::buf);  // (every listed snapshot or database is out: its release deletes the husk)
  leave_husks(c->place_dbs, &rebvio_hip_place_db::rows);
  c->own.release();
  delete c;
}

int rebvio_hip_scale_space(rebvio_hip_ctx* c, const float* img, float* scale0, float* scale1, float* dog, float* mag) {
  HIPCHK(hipSetDevice(c->device));
  const size_t nb = (size_t)c->P.rows * c->P.cols * sizeof(float);
  if (!c->diag0) {
    HIPCHK(c->own.device_bytes(&c->diag0, nb));
    HIPCHK(c->own.device_bytes(&c->diag1, nb));
  }
  HIPCHK(hipMemcpyAsync(c->img_dev, img, nb, hipMemcpyHostToDevice, c->s_det));
  ScaleBufs sb = c->sb;
  sb.scale0 = c->diag0;
  sb.scale1 = c->diag1;
  launch_scale_space(c->s_det, c->K, c->img_dev, 0, sb, c->widths, c->db.rowcount);
  HIPCHK(hipGetLastError());
  if (scale0) HIPCHK(hipMemcpyAsync(scale0, c->diag0, nb, hipMemcpyDeviceToHost, c->s_det));
  if (scale1) HIPCHK(hipMemcpyAsync(scale1, c->diag1, nb, hipMemcpyDeviceToHost, c->s_det));
  if (dog) HIPCHK(hipMemcpyAsync(dog, c->sb.dog, nb, hipMemcpyDeviceToHost, c->s_det));
  if (mag) HIPCHK(hipMemcpyAsync(mag, c->sb.mag, nb, hipMemcpyDeviceToHost, c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_det));
  return 0;
}

int rebvio_hip_detect(rebvio_hip_ctx* c, const float* img, size_t pitch_bytes, uint64_t ts_us, rebvio_hip_map** out) {
  HIPCHK(hipSetDevice(c->device));
  const size_t rowb = (size_t)c->P.cols * sizeof(float);
  return detect(c, c->img_dev, 0, 0, ts_us, out, img, pitch_bytes ? pitch_bytes : rowb, rowb);
}

int rebvio_hip_detect_u8_device(rebvio_hip_ctx* c, const uint8_t* frame_dev, uint64_t ts_us, rebvio_hip_map** out) {
  HIPCHK(hipSetDevice(c->device));
  return detect(c, frame_dev, 1, px::GRAY8, ts_us, out);
}

int rebvio_hip_detect_u8(rebvio_hip_ctx* c, const uint8_t* img, size_t pitch_bytes, uint64_t ts_us, rebvio_hip_map** out) {
  HIPCHK(hipSetDevice(c->device));
  const size_t rowb = (size_t)c->P.cols;
  return detect(c, c->img8_dev, 1, px::GRAY8, ts_us, out, img, pitch_bytes ? pitch_bytes : rowb, rowb);
}

int rebvio_hip_detect_px(rebvio_hip_ctx* c, const void* img, size_t pitch_bytes, int fmt, uint64_t ts_us, rebvio_hip_map** out) {
  int rc = check_px(c, "detect_px", img, fmt, true, pitch_bytes);
  if (rc) return rc;
  if (fmt == px::GRAY8) return rebvio_hip_detect_u8(c, static_cast<const uint8_t*>(img), pitch_bytes, ts_us, out);
  HIPCHK(hipSetDevice(c->device));
  const size_t rowb = (size_t)c->P.cols * px::bytes_per_pixel(fmt);
  return detect(c, u8_staging(c, fmt), 1, fmt, ts_us, out, img, pitch_bytes ? pitch_bytes : rowb, rowb);
}

int rebvio_hip_detect_px_device(rebvio_hip_ctx* c, const void* frame_dev, int fmt, uint64_t ts_us, rebvio_hip_map** out) {
  int rc = check_px(c, "detect_px_device", frame_dev, fmt, false, 0);
  if (rc) return rc;
  if (fmt == px::GRAY8) return rebvio_hip_detect_u8_device(c, static_cast<const uint8_t*>(frame_dev), ts_us, out);
  HIPCHK(hipSetDevice(c->device));
  return detect(c, frame_dev, 1, fmt, ts_us, out);
}

int rebvio_hip_detect_px_masked_device(rebvio_hip_ctx* c, const void* frame_dev, int fmt, const uint8_t* mask_dev, uint64_t ts_us,
                                       rebvio_hip_map** out) {
  int rc = check_px(c, "detect_px_masked_device", frame_dev, fmt, false, 0);
  if (rc == 0 && !mask_dev) rc = fail_msg("detect_px_masked_device: null mask", -3);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  return detect(c, frame_dev, 1, fmt, ts_us, out, nullptr, 0, 0, mask_dev);
}

int rebvio_hip_set_undistort(rebvio_hip_ctx* c, const float K4[4], const float D5[5]) {
  // refused before the context is touched (the model in force stays), an all-zero D5 included; a word that is not finite first
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(i < 4 ? K4[i] : D5[i - 4])) return fail_msg("set_undistort: K4 and D5 must be finite", -3);
  if (!(K4[0] > 0.0f) || !(K4[1] > 0.0f)) return fail_msg("set_undistort: focal lengths must be positive", -3);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());  // no frame in flight may still read the old map
  bool any = false;
  for (int i = 0; i < 5; ++i) any = any || (D5[i] != 0.0f);
  if (!any) {  // identity: the fixed-point map reproduces x3 exactly, skip the gather
    c->own.drop(&c->undist_map);
    return 0;
  }
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  std::vector<int> map(2 * Pn);
  hm::undistort_fixed_map(c->P.rows, c->P.cols, K4[0], K4[1], K4[2], K4[3], D5[0], D5[1], D5[2], D5[3], D5[4], map.data());
  if (!c->undist_map) HIPCHK(c->own.device(&c->undist_map, Pn));
  for (int i = 0; i < kDetPar; ++i)
    if (!c->undist_img[i]) HIPCHK(c->own.device(&c->undist_img[i], Pn));
  HIPCHK(hipMemcpy(c->undist_map, map.data(), Pn * sizeof(int2), hipMemcpyHostToDevice));
  return 0;
}

int rebvio_hip_front_end_u8(rebvio_hip_ctx* c, const uint8_t* img, float* out) {
  HIPCHK(hipSetDevice(c->device));
  if (!c->undist_map) return fail_msg("front_end_u8: no distortion model set (rebvio_hip_set_undistort)", -3);
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  HIPCHK(hipMemcpyAsync(c->img8_dev, img, Pn, hipMemcpyHostToDevice, c->s_det));
  launch_front_end_u8(c->s_det, c->K, c->img8_dev, c->undist_map, c->undist_img[0]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->undist_img[0], Pn * sizeof(float), hipMemcpyDeviceToHost, c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_det));
  return 0;
}

int rebvio_hip_front_end_px(rebvio_hip_ctx* c, const void* img, size_t pitch_bytes, int fmt, float* out) {
  int rc = check_px(c, "front_end_px", img, fmt, true, pitch_bytes);
  if (rc) return rc;
  if (!out) return fail_msg("front_end_px: null output", -3);
  HIPCHK(hipSetDevice(c->device));
  if (!c->undist_map) return fail_msg("front_end_px: no distortion model set (rebvio_hip_set_undistort)", -3);
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  const size_t rowb = (size_t)c->P.cols * px::bytes_per_pixel(fmt);
  uint8_t* stage = static_cast<uint8_t*>(u8_staging(c, fmt));
  HIPCHK(hipMemcpy2DAsync(stage, rowb, img, pitch_bytes ? pitch_bytes : rowb, rowb, (size_t)c->P.rows, hipMemcpyHostToDevice, c->s_det));
  launch_front_end_px(c->s_det, c->K, stage, fmt, c->undist_map, c->undist_img[0]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->undist_img[0], Pn * sizeof(float), hipMemcpyDeviceToHost, c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_det));
  return 0;
}

int rebvio_hip_detector_state(rebvio_hip_ctx* c, float* threshold, float* auto_threshold, int* count) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_key));
  DetState d;
  HIPCHK(hipMemcpy(&d, c->det + (c->frame_index % kDetRing), sizeof(d), hipMemcpyDeviceToHost));
  float at = d.auto_threshold;
  if (c->last_detected) {  // tuneThreshold of the last frame (edge_detector.cpp:184), same fp32 formula as the kernels
    MapState st;
    HIPCHK(hipMemcpy(&st, c->last_detected->d.st, sizeof(st), hipMemcpyDeviceToHost));
    if (st.n > 0) {
      float mx, mn;
      std::memcpy(&mx, &st.gmax_bits, 4);
      std::memcpy(&mn, &st.gmin_bits, 4);
      at = mx - float(kNumBins * (mx - mn)) / float(kNumBins);
    }
  }
  if (threshold) *threshold = d.threshold;
  if (auto_threshold) *auto_threshold = at;
  if (count) *count = d.count;
  return 0;
}

int rebvio_hip_map_size(rebvio_hip_map* m) {
  const Alive alive(m);
  if (alive.dead()) return -10;
  if (ensure_size(m)) return -1;
  return m->n_host;
}
float rebvio_hip_map_threshold(rebvio_hip_map* m) {
  const Alive alive(m);
  if (alive.dead()) return std::numeric_limits<float>::quiet_NaN();
  if (ensure_size(m)) return std::numeric_limits<float>::quiet_NaN();
  return m->thr_host;
}
uint64_t rebvio_hip_map_ts(rebvio_hip_map* m) { return m->ts; }

int rebvio_hip_map_download(rebvio_hip_map* m, rebvio_hip_keyline* keylines, int* mask) {
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_size(m);
  if (rc) return rc;
  // one packing buffer per context (callbacks and the fusion thread may both mirror maps); the same mutex orders the
  // "has the tracker touched this map" decision below against the tracker's first use of it (trk_wait_ready)
  std::lock_guard<std::mutex> dl(c->dl_mu);
  // The mirror reflects everything enqueued so far that concerns THIS map: its detection and distance field (`ready`,
  // recorded behind them; ensure_size has waited for them to be enqueued) and, once the tracker has used the
  // map, the track stream. A map fresh from detect() (edge-image callbacks, ros_rebvio.cpp:32-50) does not wait for the
  // tracker - which may be a pair ahead, or hold a second half parked until the fusion thread releases it.
  if (m->trk_touched.load(std::memory_order_acquire) || !c->owns_streams) {
    HIPCHK(hipStreamSynchronize(c->s_det));
    HIPCHK(hipStreamSynchronize(c->s_key));
    HIPCHK(hipStreamSynchronize(c->s_key));
    { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  } else {
    wait_enqueued(m);
    HIPCHK(hipEventSynchronize(m->ready));
  }
  if (keylines && m->n_host > 0) {
    launch_map_pack(c->s_key, c->K, m->d, c->aos_dev);
    HIPCHK(hipMemcpyAsync(keylines, c->aos_dev, (size_t)m->n_host * sizeof(rebvio_hip_keyline), hipMemcpyDeviceToHost, c->s_key));
  }
  if (mask)
    HIPCHK(hipMemcpyAsync(mask, m->d.mask, (size_t)c->P.rows * c->P.cols * sizeof(int), hipMemcpyDeviceToHost, c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_key));
  return 0;
}

int rebvio_hip_render_edge_image(rebvio_hip_map* m, const uint8_t* gray, uint8_t* rgb_out) {
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> dl(c->dl_mu);
  HIPCHK(hipStreamSynchronize(c->s_det));  // the staging frame and the scratch are shared with the detect path
  HIPCHK(hipStreamSynchronize(c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_key));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  uint8_t* rgb = reinterpret_cast<uint8_t*>(c->scratch_i);  // 8 bytes/pixel available, 3 used
  if (gray) HIPCHK(hipMemcpyAsync(c->img8_dev, gray, Pn, hipMemcpyHostToDevice, c->s_key));
  launch_render_edge_image(c->s_key, c->K, m->d, gray ? c->img8_dev : nullptr, rgb);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(rgb_out, rgb, 3 * Pn, hipMemcpyDeviceToHost, c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_key));
  return 0;
}

}  // extern "C"

namespace {
int check_cloud_args(const char* who, const rebvio_hip_cloud_filter* f, const rebvio_hip_cloud_pose* pose) {
  if (f) {
    if (std::isnan(f->max_rel_sigma) || std::isnan(f->rho_min) || std::isnan(f->rho_max))
      return fail_msg((std::string(who) + ": NaN in the filter").c_str(), -3);
    if (!(f->rho_min > 0.0f)) return fail_msg((std::string(who) + ": filter rho_min must be > 0").c_str(), -3);
    if (f->rho_min > f->rho_max) return fail_msg((std::string(who) + ": filter rho_min > rho_max").c_str(), -3);
    if (f->max_rel_sigma < 0.0f) return fail_msg((std::string(who) + ": filter max_rel_sigma must be >= 0").c_str(), -3);
  }
  if (pose) {
    bool nan = std::isnan(pose->scale);
    for (float v : pose->R) nan = nan || std::isnan(v);
    for (float v : pose->t) nan = nan || std::isnan(v);
    if (nan) return fail_msg((std::string(who) + ": NaN in the pose").c_str(), -3);
  }
  return 0;
}

// ---- statements the on-demand entries share. `who` is the entry's name as its messages begin; every entry calls
// them in the order it has always tested things in: that order decides which refusal wins when several apply. ----
// -3: a handle (`what`: "map", "left map", "snapshot") that belongs to another live context than the one it is used with
int other_context(const char* who, const char* what, const char* than = "") {
  return fail_msg((std::string(who) + ": " + what + " of another context" + than).c_str(), -3);
}
// A snapshot or database handed in next to a live map m is of m's context: else -10 with the handle's own sentence when its
// context is gone, -3 (other_context) when that is another live one.
template <class Handle>
int of_map_context(const char* who, const Handle* h, const rebvio_hip_map* m, const char* what, const char* than = "") {
  if (h->life == m->life) return 0;
  if (h->life->dead.load(std::memory_order_acquire)) return fail_msg(gone_text(h), -10);
  return other_context(who, what, than);
}
int snapshot_of(const char* who, const rebvio_hip_kf_snapshot* sn, const rebvio_hip_map* m) { return of_map_context(who, sn, m, "snapshot"); }
// -7: the entries that look keylines up in m's distance field need the one detection built, over keylines in detection's order
int needs_detection_field(const char* who, const rebvio_hip_map* m) {
  if (m->df_built && m->raster_order) return 0;
  return fail_msg((std::string(who) + ": the map's distance field is not detection's (none was built, or its keylines were uploaded)").c_str(), -7);
}
// -3: a pose's nine and three doubles are finite. may_be_null: a guess (R0, t0), where null stands for identity / zero.
int check_rt(const char* who, const double* R, const double* t, bool may_be_null) {
  bool fin = true;
  for (int i = 0; R && i < 9; ++i) fin = fin && std::isfinite(R[i]);
  for (int i = 0; t && i < 3; ++i) fin = fin && std::isfinite(t[i]);
  if (!fin) return fail_msg((std::string(who) + (may_be_null ? ": non-finite R0 or t0" : ": non-finite R or t")).c_str(), -3);
  return 0;
}
// -3: the association options of the entries that look keylines up in a distance field
int check_assoc_opts(const char* who, double min_cos, int max_dist, int search_range) {
  if (!(min_cos >= -1.0 && min_cos <= 1.0)) return fail_msg((std::string(who) + ": min_cos outside [-1, 1]").c_str(), -3);
  if (max_dist < 0 || max_dist > search_range) return fail_msg((std::string(who) + ": max_dist outside 0..search_range").c_str(), -3);
  return 0;
}
// -3: the options of a scalar Kalman update of (rho, sigma_rho)
int check_gate_sigma(const char* who, double gate_sigma) {
  return gate_sigma > 0.0 ? 0 : fail_msg((std::string(who) + ": gate_sigma must be > 0").c_str(), -3);
}
int check_q_abs(const char* who, double q_abs) { return q_abs >= 0.0 ? 0 : fail_msg((std::string(who) + ": q_abs must be >= 0").c_str(), -3); }

// What rebvio_hip_kf_snapshot_fuse_depth and _handover_depth ask of their pose and options, in the order both test it in.
// pixel_sigma: null where the options have none (the hand-over).
int check_kf_depth_args(const char* who, const rebvio_hip_cloud_filter& flt, const double* pixel_sigma, double gate_sigma, double q_abs,
                        double min_cos, int max_dist, int reserved, int search_range, const double* R, const double* t) {
  if (!R || !t) return fail_msg((std::string(who) + ": null R or t").c_str(), -3);
  RCCHK(check_cloud_args(who, &flt, nullptr));
  RCCHK(check_rt(who, R, t, false));
  if (pixel_sigma && !(*pixel_sigma > 0.0)) return fail_msg((std::string(who) + ": pixel_sigma must be > 0").c_str(), -3);
  RCCHK(check_gate_sigma(who, gate_sigma));
  RCCHK(check_q_abs(who, q_abs));
  RCCHK(check_assoc_opts(who, min_cos, max_dist, search_range));
  if (reserved != 0) return fail_msg((std::string(who) + ": reserved must be 0").c_str(), -3);
  return 0;
}

// Behind the kernel of fuse_depth / handover_depth on the track stream: the result struct the kernel left in the count words, the
// association words when the caller wants them, ONE wait.
template <class Result>
int fetch_counted(rebvio_hip_ctx* c, const int* cnt, const int* assoc, int kf_size, Result* out, int* assoc_host) {
  Result res;
  HIPCHK(hipMemcpyAsync(&res, cnt, sizeof(res), hipMemcpyDeviceToHost, c->s_trk));
  if (assoc_host) HIPCHK(hipMemcpyAsync(assoc_host, assoc, (size_t)kf_size * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  const int rc = trk_sync(c);
  if (rc) return rc;
  *out = res;
  return 0;
}

// Behind enqueue_depth_prior / enqueue_stereo_prior, in two steps: the counts, then exactly the words per keyline that exist
// (the outcome; the stereo entries' winner too).
template <class Counts>
int fetch_prior(rebvio_hip_ctx* c, const scratch::Counted& s, Counts* counts, int* out_host, int* out2_host) {
  Counts res;
  HIPCHK(hipMemcpyAsync(&res, s.cnt, sizeof(res), hipMemcpyDeviceToHost, c->s_trk));
  int rc = trk_sync(c);
  if (rc) return rc;
  if ((out_host || out2_host) && res.candidates > 0) {
    const size_t bytes = (size_t)res.candidates * sizeof(int);
    if (out_host) HIPCHK(hipMemcpyAsync(out_host, s.out, bytes, hipMemcpyDeviceToHost, c->s_trk));
    if (out2_host) HIPCHK(hipMemcpyAsync(out2_host, s.out2, bytes, hipMemcpyDeviceToHost, c->s_trk));
    rc = trk_sync(c);
    if (rc) return rc;
  }
  *counts = res;
  return 0;
}

// Scratch of the keyframe correspondences (rebvio_hip_map_keyframe_matches, rebvio_hip_map_keyframe_pose), made at the first call
int kf_scratch(rebvio_hip_ctx* c) {
  if (c->kf.rec) return 0;
  RCCHK(ensure_scratch(c, c->kf, (size_t)c->P.keylines_max, (size_t)kMaxRecBlocks));
  HIPCHK(c->own.device(&c->kf.rec, (size_t)c->P.keylines_max));
  return 0;
}

static_assert(sizeof(rebvio_hip_cloud_point) == 32 && sizeof(CloudHdr) == 64, "a cloud record is two 16-byte stores behind a 64-byte head");

int alloc_cloud(rebvio_hip_ctx* c, rebvio_hip_cloud* cl) {
  const size_t bytes = sizeof(CloudHdr) + (size_t)c->P.keylines_max * sizeof(rebvio_hip_cloud_point);
  HIPCHK(cl->own.pinned_bytes(&cl->hdr, bytes, false));
  std::memset(cl->hdr, 0, sizeof(CloudHdr));
  HIPCHK(cl->own.device(&cl->dev_buf, bytes));
  cl->dev = cl->dev_buf + sizeof(CloudHdr);
  HIPCHK(cl->own.event(&cl->extracted));
  HIPCHK(cl->own.event(&cl->done));
  return 0;
}

// buffers and events of a cloud; the host struct stays (a handle the caller still holds is deleted by its release)
void free_cloud_device(rebvio_hip_cloud* cl) {
  cl->own.release();
  cl->hdr = nullptr;
  cl->dev_buf = nullptr;
  cl->dev = nullptr;
  cl->done = cl->extracted = hipEvent_t{};
  cl->ctx = nullptr;
}

void release_cloud(rebvio_hip_cloud* cl) {
  std::lock_guard<std::mutex> lk(cl->ctx->cloud_mu);
  cl->in_use = false;
}

// Filter, pose and capacity of one extraction as the kernels take them. cap < 0: the buffer's capacity.
CloudArgs cloud_args(const rebvio_hip_ctx* c, const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose, int cap) {
  rebvio_hip_cloud_filter f;
  if (filter) f = *filter; else rebvio_hip_default_cloud_filter(&f);
  CloudArgs a{};
  a.min_matches = f.min_matches;
  a.max_rel_sigma = f.max_rel_sigma;
  a.rho_min = f.rho_min;
  a.rho_max = f.rho_max;
  for (int i = 0; i < 9; ++i) a.R[i] = pose ? pose->R[i] : (i % 4 == 0 ? 1.0f : 0.0f);
  for (int i = 0; i < 3; ++i) a.t[i] = pose ? pose->t[i] : 0.0f;
  a.scale = pose ? pose->scale : 1.0f;
  a.cap = (cap < 0 || cap > c->P.keylines_max) ? c->P.keylines_max : cap;
  return a;
}

// A cloud's buffer for one extraction, of a map or of a snapshot (the caller holds cloud_mu): the scratch and the cloud stream at
// the context's first cloud, a free buffer of the pool or a new one, the wait the re-use rule asks for, and the stamp (into a and *out).
int cloud_take(const char* who, rebvio_hip_ctx* c, CloudArgs& a, rebvio_hip_cloud** out) {
  if (!c->cloud_scratch) {
    HIPCHK(c->own.device(&c->cloud_scratch, kMaxRecBlocks + 1, 0));
    HIPCHK(hipStreamSynchronize(nullptr));  // (hipMemset returns before the fill has run: alloc_map)
    HIPCHK(c->own.stream(&c->s_cloud, hipStreamNonBlocking));
  }
  rebvio_hip_cloud* cl = nullptr;
  for (auto* x : c->clouds)
    if (!x->in_use) cl = x;
  if (!cl) {
    if (c->clouds.size() >= 64) return fail_msg((std::string(who) + ": 64 clouds are out; release some (rebvio_hip_cloud_release)").c_str(), -2);
    cl = new rebvio_hip_cloud;
    cl->ctx = c;
    cl->life = c->life;
    const int rc = alloc_cloud(c, cl);
    if (rc) {  // nothing half-made stays in the pool
      free_cloud_device(cl);
      delete cl;
      return rc;
    }
    c->clouds.push_back(cl);
  }
  // a buffer released without having been waited for: its copy to the host may still be reading the device buffer
  if (cl->seq != 0 && hipEventQuery(cl->done) != hipSuccess) HIPCHK(hipStreamWaitEvent(c->s_trk, cl->done, 0));
  if (++c->cloud_seq == 0) ++c->cloud_seq;  // non-zero: a fresh buffer's head reads 0
  a.seq = cl->seq = c->cloud_seq;
  cl->cap = a.cap;
  *out = cl;
  return 0;
}

// Behind the extraction kernels just queued on the track stream (the caller holds cloud_mu): the copy to the host on the cloud
// stream, and the two events. The handle counts as out from here on.
int cloud_queue_copy(rebvio_hip_ctx* c, rebvio_hip_cloud* cl, const CloudArgs& a) {
  HIPCHK(hipGetLastError());
  void* hdr_host_dev = nullptr;  // the host-visible buffer as the device addresses it
  HIPCHK(hipHostGetDevicePointer(&hdr_host_dev, cl->hdr, 0));
  HIPCHK(hipEventRecord(cl->extracted, c->s_trk));
  HIPCHK(hipStreamWaitEvent(c->s_cloud, cl->extracted, 0));
  launch_point_cloud_copy(c->s_cloud, c->K, cl->dev, reinterpret_cast<const int*>(cl->dev_buf), a,
                          reinterpret_cast<unsigned*>(c->cloud_scratch + kMaxRecBlocks), reinterpret_cast<CloudHdr*>(hdr_host_dev),
                          reinterpret_cast<char*>(hdr_host_dev) + sizeof(CloudHdr));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(cl->done, c->s_cloud));
  cl->in_use = true;
  return 0;
}

// Queues one extraction on the track stream; the caller holds the map's life block. cap < 0: the buffer's capacity.
int enqueue_cloud(const char* who, rebvio_hip_map* m, const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose, int cap,
                  rebvio_hip_cloud** out) {
  rebvio_hip_ctx* c = m->ctx;
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg((std::string(who) + ": the map was handed to track_pair_finish_async with R_prior_next and is rotated for the next pair; "
                     "its cloud is available again once the next track_pair_begin has run").c_str(), -7);
  HIPCHK(hipSetDevice(c->device));
  CloudArgs a = cloud_args(c, filter, pose, cap);
  std::lock_guard<std::mutex> lk(c->cloud_mu);
  rebvio_hip_cloud* cl = nullptr;
  int rc = cloud_take(who, c, a, &cl);
  if (rc) return rc;
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  launch_point_cloud(c->s_trk, c->K, m->d, a, c->cloud_scratch, reinterpret_cast<int*>(cl->dev_buf), cl->dev);
  rc = cloud_queue_copy(c, cl, a);
  if (rc) return rc;
  *out = cl;
  return 0;
}

// The same for a snapshot (the caller holds its life block): the size is read on the device, so nothing is fetched or waited for.
int enqueue_kf_cloud(const char* who, rebvio_hip_kf_snapshot* sn, const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose,
                     int cap, rebvio_hip_cloud** out) {
  rebvio_hip_ctx* c = sn->ctx;
  HIPCHK(hipSetDevice(c->device));
  CloudArgs a = cloud_args(c, filter, pose, cap);
  std::lock_guard<std::mutex> lk(c->cloud_mu);
  rebvio_hip_cloud* cl = nullptr;
  int rc = cloud_take(who, c, a, &cl);
  if (rc) return rc;
  launch_kf_point_cloud(c->s_trk, c->K, sn->prs, sn->matches, sn->n_dev, a, c->cloud_scratch, reinterpret_cast<int*>(cl->dev_buf), cl->dev);
  rc = cloud_queue_copy(c, cl, a);
  if (rc) return rc;
  *out = cl;
  return 0;
}

// Waits for a queued extraction (polling, like trk_sync) and checks its stamp.
int wait_cloud(rebvio_hip_cloud* cl, int* count) {
  for (;;) {
    const hipError_t e = hipEventQuery(cl->done);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) HIPCHK(e);
    std::this_thread::yield();
  }
  const unsigned seq = __atomic_load_n(&cl->hdr->seq, __ATOMIC_ACQUIRE);
  if (seq != cl->seq) return fail_msg("a point cloud was read before the device had written it (sequence stamp mismatch)", kStaleRecord);
  *count = cl->hdr->count;
  return 0;
}
}  // namespace

extern "C" {

void rebvio_hip_default_cloud_filter(rebvio_hip_cloud_filter* f) {
  f->min_matches = 2;
  f->max_rel_sigma = 0.5f;
  f->rho_min = 1e-3f;  // types/keyline.hpp:17-18: the bounds rho is clamped to
  f->rho_max = 20.0f;
}

int rebvio_hip_map_point_cloud(rebvio_hip_map* m, const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose,
                               rebvio_hip_cloud_point* points, int cap, int* count) {
  if (!m) return fail_msg("map_point_cloud: null map", -3);
  if (!count) return fail_msg("map_point_cloud: null count", -3);
  if (cap < 0 || (cap > 0 && !points)) return fail_msg("map_point_cloud: cap records need a points buffer (cap >= 0)", -3);
  int rc = check_cloud_args("map_point_cloud", filter, pose);
  if (rc) return rc;
  const Alive alive(m);
  if (alive.dead()) return -10;
  *count = 0;
  rebvio_hip_cloud* cl = nullptr;
  rc = enqueue_cloud("map_point_cloud", m, filter, pose, cap, &cl);
  if (rc) return rc;
  rc = wait_cloud(cl, count);
  if (rc == 0) {
    const int k = *count < cl->cap ? *count : cl->cap;
    if (k > 0) std::memcpy(points, reinterpret_cast<const char*>(cl->hdr) + sizeof(CloudHdr), (size_t)k * sizeof(rebvio_hip_cloud_point));
  }
  release_cloud(cl);
  return rc;
}

int rebvio_hip_map_point_cloud_async(rebvio_hip_ctx* c, rebvio_hip_map* m, const rebvio_hip_cloud_filter* filter,
                                     const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud** out) {
  if (out) *out = nullptr;
  if (!c || !m || !out) return fail_msg("map_point_cloud_async: null context, map or output", -3);
  const int rc = check_cloud_args("map_point_cloud_async", filter, pose);
  if (rc) return rc;
  const Alive alive(m);
  if (alive.dead()) return -10;
  if (m->ctx != c) return other_context("map_point_cloud_async", "map");
  return enqueue_cloud("map_point_cloud_async", m, filter, pose, -1, out);
}

int rebvio_hip_cloud_wait(rebvio_hip_cloud* cl, const rebvio_hip_cloud_point** points, int* count, const void** device_points) {
  if (points) *points = nullptr;
  if (device_points) *device_points = nullptr;
  if (!cl || !count) return fail_msg("cloud_wait: null cloud or count", -3);
  *count = 0;
  const std::shared_ptr<LifeBlock> life = cl->life;
  std::shared_lock<std::shared_mutex> lk(life->mu);
  if (life->dead.load(std::memory_order_acquire)) return fail_msg("the cloud's context has been destroyed (rebvio_hip_destroy)", -10);
  HIPCHK(hipSetDevice(cl->ctx->device));
  const int rc = wait_cloud(cl, count);
  if (rc) return rc;
  if (points) *points = reinterpret_cast<const rebvio_hip_cloud_point*>(reinterpret_cast<const char*>(cl->hdr) + sizeof(CloudHdr));
  if (device_points) *device_points = cl->dev;
  return 0;
}

void rebvio_hip_cloud_release(rebvio_hip_cloud* cl) {
  if (!cl) return;
  const std::shared_ptr<LifeBlock> life = cl->life;
  std::shared_lock<std::shared_mutex> lk(life->mu);
  if (life->dead.load(std::memory_order_acquire)) {  // the context is gone (its buffers with it): drop the husk
    if (cl->in_use) delete cl;
    return;
  }
  release_cloud(cl);
}

int rebvio_hip_map_mark_keyframe(rebvio_hip_ctx* c, rebvio_hip_map* m) {
  if (!c || !m) return fail_msg("map_mark_keyframe: null context or map", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  if (m->ctx != c) return other_context("map_mark_keyframe", "map");
  HIPCHK(hipSetDevice(c->device));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  launch_mark_keyframe(c->s_trk, c->K, m->d);
  HIPCHK(hipGetLastError());
  return 0;
}

static_assert(sizeof(rebvio_hip_kf_match) == 32, "a correspondence record is two 16-byte stores");

int rebvio_hip_map_keyframe_matches(rebvio_hip_map* m, int kf_size, rebvio_hip_kf_match* out_host, int cap, int* count) {
  if (!m) return fail_msg("map_keyframe_matches: null map", -3);
  if (!count) return fail_msg("map_keyframe_matches: null count", -3);
  if (cap < 0 || (cap > 0 && !out_host)) return fail_msg("map_keyframe_matches: cap records need an output buffer (cap >= 0)", -3);
  if (kf_size < 0) return fail_msg("map_keyframe_matches: negative kf_size", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  if (kf_size > c->P.keylines_max) return fail_msg("map_keyframe_matches: kf_size above keylines_max", -3);
  *count = 0;
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg("map_keyframe_matches: the map was handed to track_pair_finish_async with R_prior_next and is rotated for the next pair; "
                    "its correspondences are available again once the next track_pair_begin has run", -7);
  if (kf_size == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  { const int rc_sc = kf_scratch(c); if (rc_sc) return rc_sc; }
  if (cap > c->P.keylines_max) cap = c->P.keylines_max;  // (no more slots than that can hold a claimant)
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  int* count_dev = c->kf.blk + kMaxRecBlocks;
  HIPCHK((hipError_t)launch_kf_matches(c->s_trk, c->K, m->d, kf_size, cap, c->kf.key, c->kf.claimants, c->kf.blk, count_dev, c->kf.rec));
  HIPCHK(hipGetLastError());
  // the count first; then one copy of exactly the records that exist
  int n = 0;
  HIPCHK(hipMemcpyAsync(&n, count_dev, sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  const int k = n < cap ? n : cap;
  if (k > 0) {
    HIPCHK(hipMemcpyAsync(out_host, c->kf.rec, (size_t)k * sizeof(rebvio_hip_kf_match), hipMemcpyDeviceToHost, c->s_trk));
    const int rc_ts = trk_sync(c);
    if (rc_ts) return rc_ts;
  }
  *count = n;
  return 0;
}

int rebvio_hip_map_keyframe_snapshot(rebvio_hip_ctx* c, rebvio_hip_map* m, rebvio_hip_kf_snapshot** out) {
  if (out) *out = nullptr;
  if (!c || !m || !out) return fail_msg("map_keyframe_snapshot: null context, map or output", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  if (m->ctx != c) return other_context("map_keyframe_snapshot", "map");
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg("map_keyframe_snapshot: the map was handed to track_pair_finish_async with R_prior_next and is rotated for the next pair; "
                    "take the snapshot before that call, or once the next track_pair_begin has run", -7);
  HIPCHK(hipSetDevice(c->device));
  auto* sn = new rebvio_hip_kf_snapshot;
  sn->ctx = c;
  sn->life = c->life;
  const size_t M = (size_t)div_up(c->P.keylines_max, 256) * 256;
  const hipError_t e = sn->own.device_bytes(&sn->buf, M * (sizeof(float4) + sizeof(unsigned)) + 16);
  if (e != hipSuccess) {
    delete sn;
    return fail("map_keyframe_snapshot: device buffer", e);
  }
  sn->prs = sn->buf;
  sn->matches = reinterpret_cast<unsigned*>(sn->buf + M * sizeof(float4));
  sn->n_dev = reinterpret_cast<int*>(sn->matches + M);
  {
    std::lock_guard<std::mutex> lk(c->snap_mu);
    c->snaps.push_back(sn);
  }
  *out = sn;  // (from here on the caller's release gives the buffer back, whatever fails below)
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  launch_kf_snapshot(c->s_trk, c->K, m->d, sn->prs, sn->matches, sn->n_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

void rebvio_hip_kf_snapshot_release(rebvio_hip_kf_snapshot* sn) { unlist_and_release(&rebvio_hip_ctx::snaps, &rebvio_hip_ctx::snap_mu, sn); }

namespace {
// the keyframe's size on the host: fetched once, behind the snapshot kernel in stream order
int snapshot_size(rebvio_hip_ctx* c, rebvio_hip_kf_snapshot* sn) {
  if (sn->n_host >= 0) return 0;
  int n = 0;
  HIPCHK(hipMemcpyAsync(&n, sn->n_dev, sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  const int rc = trk_sync(c);
  if (rc) return rc;
  sn->n_host = n;
  return 0;
}

int check_kf_pose_args(const char* who, const rebvio_hip_kf_pose_opts& o, const double* R0, const double* t0) {
  const int rc = check_cloud_args(who, &o.kf_filter, nullptr);
  if (rc) return rc;
  if (!(o.huber_px > 0.0)) return fail_msg((std::string(who) + ": huber_px must be > 0").c_str(), -3);
  if (o.max_iter < 0 || o.max_iter > 32) return fail_msg((std::string(who) + ": max_iter outside 0..32").c_str(), -3);
  if (o.min_used < 0 || o.min_used > 65536) return fail_msg((std::string(who) + ": min_used outside 0..65536").c_str(), -3);
  return check_rt(who, R0, t0, true);
}

// the result block before the first evaluation: the guess, everything else zero
void kf_pose_start(rebvio_hip_kf_pose* o, const double* R0, const double* t0) {
  std::memset(o, 0, sizeof(*o));
  for (int i = 0; i < 9; ++i) o->R[i] = R0 ? R0[i] : (i % 4 == 0 ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) o->t[i] = t0 ? t0[i] : 0.0;
}
}  // namespace

int rebvio_hip_kf_snapshot_download(rebvio_hip_kf_snapshot* sn, float* prs4, unsigned* matches, int cap, int* n) {
  if (!sn || !n) return fail_msg("kf_snapshot_download: null snapshot or n", -3);
  if (cap < 0 || (cap > 0 && (!prs4 || !matches))) return fail_msg("kf_snapshot_download: cap records need both output buffers (cap >= 0)", -3);
  *n = 0;
  const Alive alive(sn);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = sn->ctx;
  HIPCHK(hipSetDevice(c->device));
  int rc = snapshot_size(c, sn);
  if (rc) return rc;
  const int k = sn->n_host < cap ? sn->n_host : cap;
  if (k > 0) {
    HIPCHK(hipMemcpyAsync(prs4, sn->prs, (size_t)k * sizeof(float4), hipMemcpyDeviceToHost, c->s_trk));
    HIPCHK(hipMemcpyAsync(matches, sn->matches, (size_t)k * sizeof(unsigned), hipMemcpyDeviceToHost, c->s_trk));
    rc = trk_sync(c);
    if (rc) return rc;
  }
  *n = sn->n_host;
  return 0;
}

int rebvio_hip_kf_snapshot_point_cloud(rebvio_hip_kf_snapshot* sn, const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose,
                                       rebvio_hip_cloud_point* points, int cap, int* count) {
  if (!sn) return fail_msg("kf_snapshot_point_cloud: null snapshot", -3);
  if (!count) return fail_msg("kf_snapshot_point_cloud: null count", -3);
  if (cap < 0 || (cap > 0 && !points)) return fail_msg("kf_snapshot_point_cloud: cap records need a points buffer (cap >= 0)", -3);
  int rc = check_cloud_args("kf_snapshot_point_cloud", filter, pose);
  if (rc) return rc;
  *count = 0;
  const Alive alive(sn);
  if (alive.dead()) return -10;
  rebvio_hip_cloud* cl = nullptr;
  rc = enqueue_kf_cloud("kf_snapshot_point_cloud", sn, filter, pose, cap, &cl);
  if (rc) return rc;
  rc = wait_cloud(cl, count);
  if (rc == 0) {
    const int k = *count < cl->cap ? *count : cl->cap;
    if (k > 0) std::memcpy(points, reinterpret_cast<const char*>(cl->hdr) + sizeof(CloudHdr), (size_t)k * sizeof(rebvio_hip_cloud_point));
  }
  release_cloud(cl);
  return rc;
}

int rebvio_hip_kf_snapshot_point_cloud_async(rebvio_hip_kf_snapshot* sn, const rebvio_hip_cloud_filter* filter,
                                             const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud** out) {
  if (out) *out = nullptr;
  if (!sn || !out) return fail_msg("kf_snapshot_point_cloud_async: null snapshot or output", -3);
  const int rc = check_cloud_args("kf_snapshot_point_cloud_async", filter, pose);
  if (rc) return rc;
  const Alive alive(sn);
  if (alive.dead()) return -10;
  return enqueue_kf_cloud("kf_snapshot_point_cloud_async", sn, filter, pose, -1, out);
}

int rebvio_hip_test_kf_cloud_host(float fm, const float* snap_prs4, const unsigned* snap_matches, int kf_size,
                                  const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud_point* points,
                                  int cap, int* count) {
  if (!count || kf_size < 0 || (kf_size > 0 && (!snap_prs4 || !snap_matches)))
    return fail_msg("test_kf_cloud_host: null array or count, or a negative size", -3);
  if (cap < 0 || (cap > 0 && !points)) return fail_msg("test_kf_cloud_host: cap records need a points buffer (cap >= 0)", -3);
  const int rc = check_cloud_args("test_kf_cloud_host", filter, pose);
  if (rc) return rc;
  rebvio_hip_cloud_filter f;
  if (filter) f = *filter; else rebvio_hip_default_cloud_filter(&f);
  const float eye[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, zero[3] = {0.0f, 0.0f, 0.0f};
  kfc::extract_host(fm, snap_prs4, snap_matches, kf_size, f, pose ? pose->R : eye, pose ? pose->t : zero, pose ? pose->scale : 1.0f, points,
                    cap, count);
  return 0;
}

void rebvio_hip_default_kf_pose_opts(rebvio_hip_kf_pose_opts* o) {
  rebvio_hip_default_cloud_filter(&o->kf_filter);
  o->huber_px = 2.0;
  o->max_iter = 8;
  o->min_used = 12;
}

static_assert(sizeof(rebvio_hip_kf_pose) == 55 * 8 + 16, "the result block is copied as it is");

int rebvio_hip_map_keyframe_pose(rebvio_hip_map* m, rebvio_hip_kf_snapshot* sn, const rebvio_hip_kf_pose_opts* opts, const double* R0,
                                 const double* t0, rebvio_hip_kf_pose* out) {
  if (!m || !sn || !out) return fail_msg("map_keyframe_pose: null map, snapshot or output", -3);
  rebvio_hip_kf_pose_opts o;
  if (opts) o = *opts; else rebvio_hip_default_kf_pose_opts(&o);
  RCCHK(check_kf_pose_args("map_keyframe_pose", o, R0, t0));
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(snapshot_of("map_keyframe_pose", sn, m));
  rebvio_hip_ctx* c = m->ctx;
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg("map_keyframe_pose: the map was handed to track_pair_finish_async with R_prior_next and is rotated for the next pair; "
                    "its pose is available again once the next track_pair_begin has run", -7);
  HIPCHK(hipSetDevice(c->device));
  RCCHK(snapshot_size(c, sn));
  const int kf_size = sn->n_host;
  rebvio_hip_kf_pose start;
  kf_pose_start(&start, R0, t0);
  if (kf_size == 0) {  // no candidates: nothing is launched
    start.status = 3;
    *out = start;
    return 0;
  }
  // scratch of the correspondences and of the solve
  RCCHK(kf_scratch(c));
  RCCHK(ensure_scratch(c, c->kfp, (size_t)kMaxRecBlocks, (size_t)0));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  int* count_dev = c->kf.blk + kMaxRecBlocks;
  HIPCHK((hipError_t)launch_kf_matches(c->s_trk, c->K, m->d, kf_size, c->P.keylines_max, c->kf.key, c->kf.claimants, c->kf.blk, count_dev, c->kf.rec));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->kfp.state, &start, sizeof(start), hipMemcpyHostToDevice, c->s_trk));
  for (int it = 0; it <= o.max_iter; ++it)
    launch_kf_pose_eval(c->s_trk, c->K, m->d, kf_size, c->kf.rec, count_dev, sn->prs, sn->matches, o.kf_filter, o.huber_px, it == 0,
                        it == o.max_iter, o.min_used, c->kfp.state, c->kfp.part, c->kfp.used);
  HIPCHK(hipGetLastError());
  rebvio_hip_kf_pose res;
  HIPCHK(hipMemcpyAsync(&res, c->kfp.state, sizeof(res), hipMemcpyDeviceToHost, c->s_trk));
  RCCHK(trk_sync(c));
  *out = res;
  return 0;
}

int rebvio_hip_test_kf_pose_host(float fm, const float* snap_prs4, const unsigned* snap_matches, int kf_size, const float* cur_pos_img,
                                 const float* cur_gradient, int n_cur, const rebvio_hip_kf_match* records, int n_rec,
                                 const rebvio_hip_kf_pose_opts* opts, const double* R0, const double* t0, rebvio_hip_kf_pose* out) {
  if (!out || kf_size < 0 || n_cur < 0 || n_rec < 0 || (kf_size > 0 && (!snap_prs4 || !snap_matches)) ||
      (n_cur > 0 && (!cur_pos_img || !cur_gradient)) || (n_rec > 0 && !records))
    return fail_msg("test_kf_pose_host: null array or negative size", -3);
  rebvio_hip_kf_pose_opts o;
  if (opts) o = *opts; else rebvio_hip_default_kf_pose_opts(&o);
  const int rc = check_kf_pose_args("test_kf_pose_host", o, R0, t0);
  if (rc) return rc;
  for (int r = 0; r < n_rec; ++r)
    if (records[r].kf_keyline < 0 || records[r].kf_keyline >= kf_size || records[r].keyline < 0 || records[r].keyline >= n_cur)
      return fail_msg("test_kf_pose_host: a record's indices lie outside the arrays", -3);
  rebvio_hip_kf_pose res;
  kf_pose_start(&res, R0, t0);
  res.candidates = n_rec;
  if (kf_size == 0) res.status = 3;
  for (int it = 0; kf_size > 0 && it <= o.max_iter; ++it) {
    double S[kfp::kSums] = {}, v[kfp::kSums], ws[48];
    int used = 0;
    for (int r = 0; r < n_rec; ++r) {
      const int j = records[r].kf_keyline, i = records[r].keyline;
      const float* k4 = snap_prs4 + 4 * (size_t)j;
      if (!kfp::filter_pass(o.kf_filter, k4[2], k4[3], snap_matches[j])) continue;
      bool in;
      if (!kfp::term(fm, k4[0], k4[1], k4[2], cur_pos_img[2 * (size_t)i], cur_pos_img[2 * (size_t)i + 1], cur_gradient[2 * (size_t)i],
                     cur_gradient[2 * (size_t)i + 1], res.R, res.t, o.huber_px, v, &in))
        continue;
      for (int k = 0; k < kfp::kSums; ++k) S[k] = S[k] + v[k];
      ++used;
    }
    kfp::step(S, used, it == 0, it == o.max_iter, o.min_used, ws, &res);
  }
  *out = res;
  return 0;
}

int rebvio_hip_kf_snapshot_add_normals(rebvio_hip_kf_snapshot* sn, rebvio_hip_map* m) {
  if (!sn || !m) return fail_msg("kf_snapshot_add_normals: null snapshot or map", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(of_map_context("kf_snapshot_add_normals", sn, m, "map"));
  rebvio_hip_ctx* c = m->ctx;
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg("kf_snapshot_add_normals: the map was handed to track_pair_finish_async with R_prior_next and its gradients are rotated "
                    "for the next pair; add the normals where the snapshot is taken", -7);
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(sn->nor_mu);
  if (!sn->normals_buf) {
    char* b = nullptr;
    const hipError_t e = sn->own.device_bytes(&b, (size_t)div_up(c->P.keylines_max, 256) * 256 * sizeof(float2));
    if (e != hipSuccess) return fail("kf_snapshot_add_normals: device buffer", e);
    sn->normals_buf = b;
  }
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  launch_kf_snapshot_normals(c->s_trk, c->K, m->d, sn->n_dev, sn->normals_buf);
  HIPCHK(hipGetLastError());
  sn->normals = sn->normals_buf;  // (every slot is written by the kernel just queued, in front of any reader on the track stream)
  return 0;
}

int rebvio_hip_kf_snapshot_download_normals(rebvio_hip_kf_snapshot* sn, float* n2, int cap, int* n) {
  if (!sn || !n) return fail_msg("kf_snapshot_download_normals: null snapshot or n", -3);
  if (cap < 0 || (cap > 0 && !n2)) return fail_msg("kf_snapshot_download_normals: cap pairs need an output buffer (cap >= 0)", -3);
  *n = 0;
  const Alive alive(sn);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = sn->ctx;
  const void* normals;
  {
    std::lock_guard<std::mutex> nl(sn->nor_mu);
    normals = sn->normals;
  }
  if (!normals) return fail_msg("kf_snapshot_download_normals: no normals were added to this snapshot (rebvio_hip_kf_snapshot_add_normals)", -7);
  HIPCHK(hipSetDevice(c->device));
  int rc = snapshot_size(c, sn);
  if (rc) return rc;
  const int k = sn->n_host < cap ? sn->n_host : cap;
  if (k > 0) {
    HIPCHK(hipMemcpyAsync(n2, normals, (size_t)k * sizeof(float2), hipMemcpyDeviceToHost, c->s_trk));
    rc = trk_sync(c);
    if (rc) return rc;
  }
  *n = sn->n_host;
  return 0;
}

void rebvio_hip_default_kf_align_opts(rebvio_hip_ctx* c, rebvio_hip_kf_align_opts* o) {
  std::memset(o, 0, sizeof(*o));
  rebvio_hip_default_cloud_filter(&o->kf_filter);
  o->huber_px = 2.0;
  o->min_cos = 0.9;
  o->max_dist = c ? (int)c->P.search_range : 40;
  o->max_iter = 8;
  o->min_used = 12;
}

namespace {
int check_kf_align_args(const char* who, const rebvio_hip_kf_align_opts& o, int search_range, const double* R0, const double* t0) {
  rebvio_hip_kf_pose_opts po;
  po.kf_filter = o.kf_filter;
  po.huber_px = o.huber_px;
  po.max_iter = o.max_iter;
  po.min_used = o.min_used;
  const int rc = check_kf_pose_args(who, po, R0, t0);
  return rc ? rc : check_assoc_opts(who, o.min_cos, o.max_dist, search_range);
}
}  // namespace

static_assert(sizeof(rebvio_hip_kf_align_opts) == 48, "filter, two doubles, three ints, padding");

int rebvio_hip_map_keyframe_align(rebvio_hip_map* m, rebvio_hip_kf_snapshot* sn, const rebvio_hip_kf_align_opts* opts, const double* R0,
                                  const double* t0, rebvio_hip_kf_pose* out, int* assoc_host) {
  if (!m || !sn || !out) return fail_msg("map_keyframe_align: null map, snapshot or output", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(snapshot_of("map_keyframe_align", sn, m));
  rebvio_hip_ctx* c = m->ctx;
  rebvio_hip_kf_align_opts o;
  if (opts) o = *opts; else rebvio_hip_default_kf_align_opts(c, &o);
  RCCHK(check_kf_align_args("map_keyframe_align", o, (int)c->P.search_range, R0, t0));
  RCCHK(needs_detection_field("map_keyframe_align", m));
  HIPCHK(hipSetDevice(c->device));
  RCCHK(snapshot_size(c, sn));
  const int kf_size = sn->n_host;
  rebvio_hip_kf_pose start;
  kf_pose_start(&start, R0, t0);
  if (kf_size == 0) {  // nothing to align: nothing is launched
    start.status = 3;
    *out = start;
    return 0;
  }
  RCCHK(ensure_scratch(c, c->kfa, (size_t)kMaxRecBlocks, (size_t)c->P.keylines_max));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  HIPCHK(hipMemcpyAsync(c->kfa.state, &start, sizeof(start), hipMemcpyHostToDevice, c->s_trk));
  const void* normals;
  {
    std::lock_guard<std::mutex> lk(sn->nor_mu);
    normals = sn->normals;
  }
  for (int it = 0; it <= o.max_iter; ++it)
    launch_kf_align_eval(c->s_trk, c->K, m->d, kf_size, sn->n_dev, sn->prs, sn->matches, normals, o.kf_filter, o.huber_px, o.min_cos,
                         o.max_dist, it == 0, it == o.max_iter, o.min_used, c->kfa.state, c->kfa.part, c->kfa.used, c->kfa.assoc);
  HIPCHK(hipGetLastError());
  rebvio_hip_kf_pose res;
  HIPCHK(hipMemcpyAsync(&res, c->kfa.state, sizeof(res), hipMemcpyDeviceToHost, c->s_trk));
  if (assoc_host) HIPCHK(hipMemcpyAsync(assoc_host, c->kfa.assoc, (size_t)kf_size * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  RCCHK(trk_sync(c));
  *out = res;
  return 0;
}

int rebvio_hip_test_kf_align_host(float fm, float cx, float cy, int rows, int cols, int search_range, const float* snap_prs4,
                                  const unsigned* snap_matches, const float* snap_normals, int kf_size, const float* cur_pos,
                                  const float* cur_unit, int n_cur, const int* df_id, const int* df_dist,
                                  const rebvio_hip_kf_align_opts* opts, const double* R0, const double* t0, rebvio_hip_kf_pose* out,
                                  int* assoc) {
  if (!out || kf_size < 0 || n_cur < 0 || rows < 0 || cols < 0 || (kf_size > 0 && (!snap_prs4 || !snap_matches)) ||
      (n_cur > 0 && (!cur_pos || !cur_unit)) || ((size_t)rows * (size_t)cols > 0 && (!df_id || !df_dist)))
    return fail_msg("test_kf_align_host: null array or negative size", -3);
  rebvio_hip_kf_align_opts o;
  if (opts) {
    o = *opts;
  } else {
    rebvio_hip_default_kf_align_opts(nullptr, &o);
    o.max_dist = search_range;
  }
  const int rc = check_kf_align_args("test_kf_align_host", o, search_range, R0, t0);
  if (rc) return rc;
  const size_t Pn = (size_t)rows * (size_t)cols;
  for (size_t k = 0; k < Pn; ++k)
    if (df_id[k] >= n_cur) return fail_msg("test_kf_align_host: a field id lies outside the keyline arrays", -3);
  const kfp::AlignMap am = kfp::host_map(fm, cx, cy, rows, cols, df_id, df_dist, cur_pos, cur_unit, n_cur);
  kfm::align_host(am, snap_prs4, snap_matches, snap_normals, kf_size, o, R0, t0, out, assoc, nullptr);
  return 0;
}

static_assert(sizeof(rebvio_hip_kf_hypothesis) == 104 && offsetof(rebvio_hip_kf_hypothesis, R0) == 8 &&
                  offsetof(rebvio_hip_kf_hypothesis, t0) == 80,
              "a pointer, twelve doubles");
static_assert(sizeof(rebvio_hip_kf_hyp_result) == sizeof(rebvio_hip_kf_pose) + 8 && offsetof(rebvio_hip_kf_hyp_result, pose) == 0 &&
                  offsetof(rebvio_hip_kf_hyp_result, inliers) == sizeof(rebvio_hip_kf_pose) && sizeof(rebvio_hip_kf_pose) == 456,
              "the pose, two ints");

int rebvio_hip_map_keyframe_align_many(rebvio_hip_map* m, const rebvio_hip_kf_hypothesis* hyp, int n, const rebvio_hip_kf_align_opts* opts,
                                       rebvio_hip_kf_hyp_result* out) {
  if (!m || !hyp || !out) return fail_msg("map_keyframe_align_many: null map, hypothesis list or output", -3);
  if (n < 1 || n > REBVIO_HIP_KF_HYP_MAX) return fail_msg("map_keyframe_align_many: n outside 1..REBVIO_HIP_KF_HYP_MAX", -3);
  for (int h = 0; h < n; ++h)
    if (!hyp[h].snap) return fail_msg("map_keyframe_align_many: null snapshot in the list", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  for (int h = 0; h < n; ++h) RCCHK(snapshot_of("map_keyframe_align_many", hyp[h].snap, m));
  rebvio_hip_ctx* c = m->ctx;
  rebvio_hip_kf_align_opts o;
  if (opts) o = *opts; else rebvio_hip_default_kf_align_opts(c, &o);
  for (int h = 0; h < n; ++h) RCCHK(check_kf_align_args("map_keyframe_align_many", o, (int)c->P.search_range, hyp[h].R0, hyp[h].t0));
  RCCHK(needs_detection_field("map_keyframe_align_many", m));
  HIPCHK(hipSetDevice(c->device));
  // sizes and normals: each distinct snapshot is asked once (its mutex taken once, never inside another's)
  const void* normals[REBVIO_HIP_KF_HYP_MAX];
  int nb_max = 0;
  for (int h = 0; h < n; ++h) {
    rebvio_hip_kf_snapshot* sn = hyp[h].snap;
    int seen = -1;
    for (int k = 0; k < h && seen < 0; ++k)
      if (hyp[k].snap == sn) seen = k;
    if (seen >= 0) {
      normals[h] = normals[seen];
      continue;
    }
    RCCHK(snapshot_size(c, sn));
    if (sn->n_host > (int)c->P.keylines_max) return fail_msg("map_keyframe_align_many: a snapshot larger than keylines_max", -2);
    {
      std::lock_guard<std::mutex> lk(sn->nor_mu);
      normals[h] = sn->normals;
    }
    const int nb = div_up(sn->n_host, 256);
    if (nb > nb_max) nb_max = nb;
  }
  struct Stage {
    KfHypDesc desc[REBVIO_HIP_KF_HYP_MAX];
    rebvio_hip_kf_hyp_result res[REBVIO_HIP_KF_HYP_MAX];
  };
  static_assert(offsetof(Stage, res) == sizeof(KfHypDesc) * REBVIO_HIP_KF_HYP_MAX, "the results follow the table without a gap");
  std::unique_ptr<Stage> stage(new Stage);
  std::memset(stage.get(), 0, sizeof(Stage));
  for (int h = 0; h < n; ++h) {
    kf_pose_start(&stage->res[h].pose, hyp[h].R0, hyp[h].t0);
    if (hyp[h].snap->n_host == 0) stage->res[h].pose.status = 3;  // nothing to align: neither kernel touches it
  }
  if (nb_max == 0) {  // every snapshot is empty: nothing is launched
    for (int h = 0; h < n; ++h) out[h] = stage->res[h];
    return 0;
  }
  static_assert(sizeof(Stage) % 64 == 0, "the partials start on a 64-byte line");
  static_assert(sizeof(KfHypDesc) == 64 && sizeof(ChainDev) == 13 * sizeof(void*), "as their stand-ins in tests/cpp/scratch_layout_check.cpp");
  RCCHK(ensure_scratch(c, c->kfm, (size_t)kMaxRecBlocks));
  for (int h = 0; h < n; ++h) {
    const rebvio_hip_kf_snapshot* sn = hyp[h].snap;
    KfHypDesc& d = stage->desc[h];
    d.prs = sn->prs;
    d.matches = sn->matches;
    d.normals = normals[h];
    d.res = c->kfm.res + h;
    d.part = c->kfm.part + (size_t)h * kMaxRecBlocks * kfp::kSums;
    d.part_used = c->kfm.used + (size_t)h * kMaxRecBlocks;
    d.part_inl = c->kfm.inl + (size_t)h * kMaxRecBlocks;
    d.size = sn->n_host;
  }
  wait_enqueued(m);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  // ONE upload: the whole table and the first n result blocks lie next to each other
  HIPCHK(hipMemcpyAsync(c->kfm.desc, stage.get(), offsetof(Stage, res) + (size_t)n * sizeof(rebvio_hip_kf_hyp_result), hipMemcpyHostToDevice,
                        c->s_trk));
  for (int it = 0; it <= o.max_iter; ++it)
    launch_kf_align_many_eval(c->s_trk, c->K, m->d, c->kfm.desc, n, nb_max, o.kf_filter, o.huber_px, o.min_cos, o.max_dist, it == 0,
                              it == o.max_iter, o.min_used);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(stage->res, c->kfm.res, (size_t)n * sizeof(rebvio_hip_kf_hyp_result), hipMemcpyDeviceToHost, c->s_trk));
  RCCHK(trk_sync(c));
  for (int h = 0; h < n; ++h) out[h] = stage->res[h];
  return 0;
}

int rebvio_hip_kf_align_best(const rebvio_hip_kf_hyp_result* res, int n, int min_inliers) {
  if (!res || n < 1) return fail_msg("kf_align_best: null array or n < 1", -3);
  return kfm::best(res, n, min_inliers);
}

int rebvio_hip_kf_hypotheses_around(rebvio_hip_kf_snapshot* snap, const double* R, const double* t, double rot_step, double trans_step,
                                    rebvio_hip_kf_hypothesis* out) {
  if (!R || !t || !out) return fail_msg("kf_hypotheses_around: null R, t or output", -3);
  bool fin = std::isfinite(rot_step) && std::isfinite(trans_step);
  for (int i = 0; i < 9; ++i) fin = fin && std::isfinite(R[i]);
  for (int i = 0; i < 3; ++i) fin = fin && std::isfinite(t[i]);
  if (!fin) return fail_msg("kf_hypotheses_around: non-finite R, t or step", -3);
  if (rot_step < 0.0 || trans_step < 0.0) return fail_msg("kf_hypotheses_around: negative step", -3);
  kfm::around(snap, R, t, rot_step, trans_step, out);
  return 0;
}

int rebvio_hip_test_kf_align_many_host(float fm, float cx, float cy, int rows, int cols, int search_range, const float* snap_prs4,
                                       const unsigned* snap_matches, const float* snap_normals, int kf_size, const float* cur_pos,
                                       const float* cur_unit, int n_cur, const int* df_id, const int* df_dist,
                                       const rebvio_hip_kf_align_opts* opts, const double* R0s, const double* t0s, int n,
                                       rebvio_hip_kf_hyp_result* out) {
  if (!out || !R0s || !t0s || kf_size < 0 || n_cur < 0 || rows < 0 || cols < 0 || (kf_size > 0 && (!snap_prs4 || !snap_matches)) ||
      (n_cur > 0 && (!cur_pos || !cur_unit)) || ((size_t)rows * (size_t)cols > 0 && (!df_id || !df_dist)))
    return fail_msg("test_kf_align_many_host: null array or negative size", -3);
  if (n < 1 || n > REBVIO_HIP_KF_HYP_MAX) return fail_msg("test_kf_align_many_host: n outside 1..REBVIO_HIP_KF_HYP_MAX", -3);
  rebvio_hip_kf_align_opts o;
  if (opts) {
    o = *opts;
  } else {
    rebvio_hip_default_kf_align_opts(nullptr, &o);
    o.max_dist = search_range;
  }
  for (int h = 0; h < n; ++h) {
    const int rc = check_kf_align_args("test_kf_align_many_host", o, search_range, R0s + 9 * (size_t)h, t0s + 3 * (size_t)h);
    if (rc) return rc;
  }
  const size_t Pn = (size_t)rows * (size_t)cols;
  for (size_t k = 0; k < Pn; ++k)
    if (df_id[k] >= n_cur) return fail_msg("test_kf_align_many_host: a field id lies outside the keyline arrays", -3);
  const kfp::AlignMap am = kfp::host_map(fm, cx, cy, rows, cols, df_id, df_dist, cur_pos, cur_unit, n_cur);
  for (int h = 0; h < n; ++h) {
    std::memset(&out[h], 0, sizeof(out[h]));
    kfm::align_host(am, snap_prs4, snap_matches, snap_normals, kf_size, o, R0s + 9 * (size_t)h, t0s + 3 * (size_t)h, &out[h].pose, nullptr,
                    &out[h].inliers);
  }
  return 0;
}

void rebvio_hip_default_kf_fuse_opts(rebvio_hip_ctx* c, rebvio_hip_kf_fuse_opts* o) {
  std::memset(o, 0, sizeof(*o));
  rebvio_hip_default_cloud_filter(&o->kf_filter);
  o->min_cos = 0.9;
  o->pixel_sigma = c ? (double)c->P.pixel_uncertainty : 1.0;
  o->gate_sigma = 3.0;
  o->q_abs = 0.0;
  o->max_dist = c ? (int)c->P.search_range : 40;
}

namespace {
int check_kf_fuse_args(const char* who, const rebvio_hip_kf_fuse_opts& o, int search_range, const double* R, const double* t) {
  return check_kf_depth_args(who, o.kf_filter, &o.pixel_sigma, o.gate_sigma, o.q_abs, o.min_cos, o.max_dist, o.reserved, search_range, R, t);
}
}  // namespace

static_assert(sizeof(rebvio_hip_kf_fuse_opts) == 56, "filter, four doubles, two ints");
static_assert(sizeof(rebvio_hip_kf_fuse) == 24, "six ints");

int rebvio_hip_kf_snapshot_fuse_depth(rebvio_hip_kf_snapshot* sn, rebvio_hip_map* m, const rebvio_hip_kf_fuse_opts* opts, const double* R,
                                      const double* t, rebvio_hip_kf_fuse* out, int* assoc_host) {
  if (!sn || !m || !out) return fail_msg("kf_snapshot_fuse_depth: null snapshot, map or output", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(snapshot_of("kf_snapshot_fuse_depth", sn, m));
  rebvio_hip_ctx* c = m->ctx;
  rebvio_hip_kf_fuse_opts o;
  if (opts) o = *opts; else rebvio_hip_default_kf_fuse_opts(c, &o);
  RCCHK(check_kf_fuse_args("kf_snapshot_fuse_depth", o, (int)c->P.search_range, R, t));
  RCCHK(needs_detection_field("kf_snapshot_fuse_depth", m));
  HIPCHK(hipSetDevice(c->device));
  RCCHK(snapshot_size(c, sn));
  const int kf_size = sn->n_host;
  std::memset(out, 0, sizeof(*out));
  if (kf_size == 0) return 0;  // nothing to fuse: nothing is launched
  RCCHK(ensure_scratch(c, c->kff, (size_t)c->P.keylines_max, 1));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  {
    std::lock_guard<std::mutex> lk(sn->nor_mu);  // (the snapshot is this call's from the clear to the kernel, as in add_normals)
    HIPCHK(hipMemsetAsync(c->kff.cnt, 0, 8 * sizeof(int), c->s_trk));
    launch_kf_fuse_depth(c->s_trk, c->K, m->d, kf_size, sn->n_dev, sn->prs, sn->matches, sn->normals, o, R, t, c->kff.cnt, c->kff.out);
    HIPCHK(hipGetLastError());
  }
  return fetch_counted(c, c->kff.cnt, c->kff.out, kf_size, out, assoc_host);
}

int rebvio_hip_test_kf_fuse_host(float fm, float cx, float cy, int rows, int cols, int search_range, float* snap_prs4, unsigned* snap_matches,
                                 const float* snap_normals, int kf_size, const float* cur_pos, const float* cur_unit, int n_cur,
                                 const int* df_id, const int* df_dist, const rebvio_hip_kf_fuse_opts* opts, const double* R, const double* t,
                                 rebvio_hip_kf_fuse* out, int* assoc) {
  if (!out || kf_size < 0 || n_cur < 0 || rows < 0 || cols < 0 || (kf_size > 0 && (!snap_prs4 || !snap_matches)) ||
      (n_cur > 0 && (!cur_pos || !cur_unit)) || ((size_t)rows * (size_t)cols > 0 && (!df_id || !df_dist)))
    return fail_msg("test_kf_fuse_host: null array or negative size", -3);
  rebvio_hip_kf_fuse_opts o;
  if (opts) {
    o = *opts;
  } else {
    rebvio_hip_default_kf_fuse_opts(nullptr, &o);
    o.max_dist = search_range;
  }
  const int rc = check_kf_fuse_args("test_kf_fuse_host", o, search_range, R, t);
  if (rc) return rc;
  const size_t Pn = (size_t)rows * (size_t)cols;
  for (size_t k = 0; k < Pn; ++k)
    if (df_id[k] >= n_cur) return fail_msg("test_kf_fuse_host: a field id lies outside the keyline arrays", -3);
  const kfp::AlignMap am = kfp::host_map(fm, cx, cy, rows, cols, df_id, df_dist, cur_pos, cur_unit, n_cur);
  rebvio_hip_kf_fuse res;
  std::memset(&res, 0, sizeof(res));
  res.candidates = kf_size;
  for (int j = 0; j < kf_size; ++j) {
    float* k4 = snap_prs4 + 4 * (size_t)j;
    int outcome = kfp::kFuseNone, i = 0;
    float rho_n = 0.f, sig_n = 0.f;
    bool clamped = false;
    if (kfp::filter_pass(o.kf_filter, k4[2], k4[3], snap_matches[j]))
      outcome = kfp::fuse_term(am, k4[0], k4[1], k4[2], k4[3], snap_normals != nullptr, snap_normals ? snap_normals[2 * (size_t)j] : 0.0f,
                               snap_normals ? snap_normals[2 * (size_t)j + 1] : 0.0f, o.min_cos, o.max_dist, R, t, o.pixel_sigma,
                               o.gate_sigma, o.q_abs, &i, &rho_n, &sig_n, &clamped);
    if (assoc) assoc[j] = outcome == kfp::kFuseNone ? std::numeric_limits<int>::min() : outcome == kfp::kFuseFused ? i : -1 - i;
    if (outcome == kfp::kFuseNone) continue;
    ++res.associated;
    if (outcome == kfp::kFuseGated) ++res.gated;
    if (outcome == kfp::kFuseFlat) ++res.flat;
    if (outcome != kfp::kFuseFused) continue;
    ++res.fused;
    if (clamped) ++res.clamped;
    k4[2] = rho_n;
    k4[3] = sig_n;
    if (snap_matches[j] != 0xFFFFFFFFu) ++snap_matches[j];
  }
  *out = res;
  return 0;
}

// ---- depth prior from a registered depth image (include/rebvio_hip.h is the definition; depth_prior.hpp the statement) ----------
void rebvio_hip_default_depth_prior_opts(rebvio_hip_depth_prior_opts* o) {
  std::memset(o, 0, sizeof(*o));
  o->tap_px = 2.0;
  o->jump_rel = 0.1;
  o->z_min = 0.1;
  o->z_max = 20.0;
  o->sigma_z0 = 1e-3;
  o->sigma_z2 = 2e-3;
  o->gate_sigma = 3.0;
  o->q_abs = 0.0;
  o->unit = 0.001;
}

namespace {
static_assert(sizeof(rebvio_hip_depth_prior_opts) == 80, "nine doubles, one int, padding");
static_assert(sizeof(rebvio_hip_depth_prior_counts) == 24, "six ints");

inline size_t depth_tap_bytes(int fmt) { return fmt == REBVIO_HIP_DEPTH_U16 ? 2 : 4; }

// Everything that is refused before the device is touched: the format, the image's pitch and alignment, the options.
// *pitch is replaced by the dense pitch where it is 0.
int check_depth_prior_args(const char* who, const void* depth, size_t* pitch, int fmt, int cols, const rebvio_hip_depth_prior_opts& o) {
  const std::string w(who);
  if (!depth) return fail_msg((w + ": null depth image").c_str(), -3);
  if (fmt != REBVIO_HIP_DEPTH_U16 && fmt != REBVIO_HIP_DEPTH_F32)
    return fail_msg((w + ": unknown depth format (REBVIO_HIP_DEPTH_U16, REBVIO_HIP_DEPTH_F32)").c_str(), -3);
  const size_t tb = depth_tap_bytes(fmt), rowb = (size_t)cols * tb;
  if (*pitch == 0) *pitch = rowb;
  if (*pitch < rowb || *pitch % tb != 0) return fail_msg((w + ": pitch_bytes below a row's bytes or no multiple of a tap's size").c_str(), -3);
  if (reinterpret_cast<uintptr_t>(depth) % tb != 0) return fail_msg((w + ": the depth image is not aligned to a tap's size").c_str(), -3);
  if (!(o.tap_px >= 0.0 && o.tap_px < HUGE_VAL)) return fail_msg((w + ": tap_px must be >= 0 and finite").c_str(), -3);
  if (!(o.jump_rel >= 0.0)) return fail_msg((w + ": jump_rel must be >= 0").c_str(), -3);
  if (!(o.z_min > 0.0)) return fail_msg((w + ": z_min must be > 0").c_str(), -3);
  if (!(o.z_max >= o.z_min)) return fail_msg((w + ": z_max must be >= z_min").c_str(), -3);
  if (!(o.sigma_z0 >= 0.0)) return fail_msg((w + ": sigma_z0 must be >= 0").c_str(), -3);
  if (!(o.sigma_z2 >= 0.0)) return fail_msg((w + ": sigma_z2 must be >= 0").c_str(), -3);
  if (!(o.sigma_z0 + o.sigma_z2 > 0.0)) return fail_msg((w + ": sigma_z0 + sigma_z2 must be > 0").c_str(), -3);
  RCCHK(check_gate_sigma(who, o.gate_sigma));
  RCCHK(check_q_abs(who, o.q_abs));
  if (!(o.unit > 0.0)) return fail_msg((w + ": unit must be > 0").c_str(), -3);
  if (o.reserved != 0) return fail_msg((w + ": reserved must be 0").c_str(), -3);
  return 0;
}

// The state rule, the scratch and the waits, then the clear and the kernel on the track stream. The caller holds the map's life
// block and has checked the arguments. img = the image as the device addresses it.
int depth_prior_state_rule(const char* who, const rebvio_hip_map* m) {
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg((std::string(who) + ": the map was handed to track_pair_finish_async with R_prior_next and is rotated for the next pair").c_str(), -7);
  if (m->served_old)
    return fail_msg((std::string(who) + ": the map has served as a pair's old map; its depths live in a newer frame").c_str(), -7);
  return 0;
}

int enqueue_depth_prior(const char* who, rebvio_hip_map* m, const void* img, size_t pitch, int fmt, const rebvio_hip_depth_prior_opts& o) {
  rebvio_hip_ctx* c = m->ctx;
  const int rc_state = depth_prior_state_rule(who, m);
  if (rc_state) return rc_state;
  RCCHK(ensure_scratch(c, c->dpr, (size_t)c->P.keylines_max, 1));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  HIPCHK(hipMemsetAsync(c->dpr.cnt, 0, 8 * sizeof(int), c->s_trk));
  launch_depth_prior(c->s_trk, c->K, m->d, dpr::make_args(img, pitch, c->P.rows, c->P.cols, fmt, o), c->dpr.cnt, c->dpr.out);
  HIPCHK(hipGetLastError());
  c->dpr_queued = true;
  return 0;
}

int fetch_depth_prior(rebvio_hip_ctx* c, rebvio_hip_depth_prior_counts* counts, int* outcome_host) {
  return fetch_prior(c, c->dpr, counts, outcome_host, nullptr);
}

int fuse_depth_image_sync(const char* who, rebvio_hip_map* m, const void* depth, size_t pitch, int fmt, const rebvio_hip_depth_prior_opts* opts,
                          rebvio_hip_depth_prior_counts* counts, int* outcome_host, bool host_image) {
  const std::string w(who);
  if (!m) return fail_msg((w + ": null map").c_str(), -3);
  if (!counts) return fail_msg((w + ": null counts").c_str(), -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  rebvio_hip_depth_prior_opts o;
  if (opts) o = *opts; else rebvio_hip_default_depth_prior_opts(&o);
  int rc = check_depth_prior_args(who, depth, &pitch, fmt, c->P.cols, o);
  if (rc) return rc;
  std::memset(counts, 0, sizeof(*counts));
  HIPCHK(hipSetDevice(c->device));
  const void* img = depth;
  if (host_image) {
    rc = depth_prior_state_rule(who, m);  // (before the staging frame is written or made)
    if (rc) return rc;
    const size_t rowb = (size_t)c->P.cols * depth_tap_bytes(fmt);
    if (!c->dpr_pin) HIPCHK(c->own.pinned_bytes(&c->dpr_pin, (size_t)c->P.rows * c->P.cols * sizeof(float), false));
    // (the previous call that used the frame was synchronous: nothing reads it any more)
    const char* src = static_cast<const char*>(depth);
    for (int r = 0; r < c->P.rows; ++r) std::memcpy(c->dpr_pin + (size_t)r * rowb, src + (size_t)r * pitch, rowb);
    void* dev_view = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dev_view, c->dpr_pin, 0));
    img = dev_view;
    pitch = rowb;
  }
  rc = enqueue_depth_prior(who, m, img, pitch, fmt, o);
  if (rc) return rc;
  return fetch_depth_prior(c, counts, outcome_host);
}
}  // namespace

int rebvio_hip_map_fuse_depth_image(rebvio_hip_map* m, const void* depth_host, size_t pitch_bytes, int fmt, const rebvio_hip_depth_prior_opts* opts,
                                    rebvio_hip_depth_prior_counts* counts, int* outcome_host) {
  return fuse_depth_image_sync("map_fuse_depth_image", m, depth_host, pitch_bytes, fmt, opts, counts, outcome_host, true);
}

int rebvio_hip_map_fuse_depth_image_device(rebvio_hip_map* m, const void* depth_dev, size_t pitch_bytes, int fmt,
                                           const rebvio_hip_depth_prior_opts* opts, rebvio_hip_depth_prior_counts* counts, int* outcome_host) {
  return fuse_depth_image_sync("map_fuse_depth_image_device", m, depth_dev, pitch_bytes, fmt, opts, counts, outcome_host, false);
}

int rebvio_hip_map_fuse_depth_image_async(rebvio_hip_ctx* c, rebvio_hip_map* m, const void* depth_dev, size_t pitch_bytes, int fmt,
                                          const rebvio_hip_depth_prior_opts* opts) {
  if (!c || !m) return fail_msg("map_fuse_depth_image_async: null context or map", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  if (m->ctx != c) return other_context("map_fuse_depth_image_async", "map");
  rebvio_hip_depth_prior_opts o;
  if (opts) o = *opts; else rebvio_hip_default_depth_prior_opts(&o);
  const int rc = check_depth_prior_args("map_fuse_depth_image_async", depth_dev, &pitch_bytes, fmt, c->P.cols, o);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  return enqueue_depth_prior("map_fuse_depth_image_async", m, depth_dev, pitch_bytes, fmt, o);
}

int rebvio_hip_depth_prior_last_counts(rebvio_hip_ctx* c, rebvio_hip_depth_prior_counts* counts) {
  if (!c || !counts) return fail_msg("depth_prior_last_counts: null context or counts", -3);
  std::memset(counts, 0, sizeof(*counts));
  if (!c->dpr_queued) return 0;
  HIPCHK(hipSetDevice(c->device));
  return fetch_depth_prior(c, counts, nullptr);
}

int rebvio_hip_test_depth_prior_host(int rows, int cols, rebvio_hip_keyline* keylines, int n, const void* depth, size_t pitch_bytes, int fmt,
                                     const rebvio_hip_depth_prior_opts* opts, rebvio_hip_depth_prior_counts* counts, int* outcome) {
  if (!counts || n < 0 || rows < 0 || cols < 0 || (n > 0 && !keylines))
    return fail_msg("test_depth_prior_host: null array or negative size", -3);
  rebvio_hip_depth_prior_opts o;
  if (opts) o = *opts; else rebvio_hip_default_depth_prior_opts(&o);
  const int rc = check_depth_prior_args("test_depth_prior_host", depth, &pitch_bytes, fmt, cols, o);
  if (rc) return rc;
  const dpr::Args a = dpr::make_args(depth, pitch_bytes, rows, cols, fmt, o);
  rebvio_hip_depth_prior_counts res;
  std::memset(&res, 0, sizeof(res));
  res.candidates = n;
  for (int i = 0; i < n; ++i) {
    rebvio_hip_keyline& k = keylines[i];
    float rho_n = 0.f, sig_n = 0.f;
    const int oc = dpr::term(a, k.pos[0], k.pos[1], k.gradient[0], k.gradient[1], k.gradient_norm, k.rho, k.sigma_rho, &rho_n, &sig_n);
    if (outcome) outcome[i] = oc;
    if (oc == dpr::kNone) continue;
    ++res.sampled;
    if (oc & dpr::kJumpBit) ++res.jumps;
    if ((oc & 3) == dpr::kGated) ++res.gated;
    if ((oc & 3) != dpr::kFused) continue;
    ++res.fused;
    if (oc & dpr::kClampedBit) ++res.clamped;
    k.rho = rho_n;
    k.sigma_rho = sig_n;
  }
  *counts = res;
  return 0;
}

// ---- depth prior from a rectified stereo partner's edge map (include/rebvio_hip.h is the definition; stereo_prior.hpp the statements)
void rebvio_hip_default_stereo_prior_opts(rebvio_hip_ctx* c, rebvio_hip_stereo_prior_opts* o) {
  std::memset(o, 0, sizeof(*o));
  o->d_min = 0.0;
  o->d_max = 64.0;
  o->min_ux = 0.5;
  o->row_tol = 1;
  o->sigma_px = 0.5;
  o->gate_sigma = 3.0;
  o->ambig_px = 2.0;
  o->cos_min = c ? (double)c->K.cang_min_edge : (double)(float)std::cos(45.0 * M_PI / 180.0);  // (as create leaves it in KParams)
  o->norm_tol = c ? (double)c->K.match_threshold_norm : 1.0;
  o->q_abs = 0.0;
}

namespace {
static_assert(sizeof(rebvio_hip_stereo_prior_opts) == 96, "four doubles, an int, six doubles, an int, padding");
static_assert(sizeof(rebvio_hip_stereo_prior_counts) == 32, "eight ints");

// The options, refused before the device is touched.
int check_stereo_prior_opts(const char* who, int cols, const rebvio_hip_stereo_prior_opts& o) {
  const std::string w(who);
  if (!(o.baseline > 0.0 && o.baseline < HUGE_VAL)) return fail_msg((w + ": baseline must be > 0 and finite").c_str(), -3);
  if (!(o.d_min >= 0.0 && o.d_min <= o.d_max && o.d_max <= (double)cols))
    return fail_msg((w + ": 0 <= d_min <= d_max <= cols does not hold").c_str(), -3);
  if (!(o.min_ux > 0.0 && o.min_ux <= 1.0)) return fail_msg((w + ": min_ux must be in (0, 1]").c_str(), -3);
  if (o.row_tol != 0 && o.row_tol != 1) return fail_msg((w + ": row_tol must be 0 or 1").c_str(), -3);
  if (!(o.sigma_px > 0.0 && o.sigma_px < HUGE_VAL)) return fail_msg((w + ": sigma_px must be > 0 and finite").c_str(), -3);
  RCCHK(check_gate_sigma(who, o.gate_sigma));
  if (!(o.ambig_px >= 0.0)) return fail_msg((w + ": ambig_px must be >= 0").c_str(), -3);
  if (!(o.cos_min >= -1.0 && o.cos_min <= 1.0)) return fail_msg((w + ": cos_min must be in [-1, 1]").c_str(), -3);
  if (!(o.norm_tol >= 0.0)) return fail_msg((w + ": norm_tol must be >= 0").c_str(), -3);
  RCCHK(check_q_abs(who, o.q_abs));
  if (o.reserved != 0) return fail_msg((w + ": reserved must be 0").c_str(), -3);
  return 0;
}

// Holds the life blocks of a left and a right map for an entry's duration: one block once when both maps are of one context (a
// shared_mutex is not taken twice by one thread), else both, in the order of their addresses.
class PairAlive {
 public:
  PairAlive(const rebvio_hip_map* l, const rebvio_hip_map* r) {
    const bool same = l->life.get() == r->life.get();
    const bool l_first = same || std::less<const LifeBlock*>()(l->life.get(), r->life.get());
    if (l_first) a_.emplace(l); else a_.emplace(r);
    if (!same) {
      if (l_first) b_.emplace(r); else b_.emplace(l);
    }
    dead_ = a_->dead() || (b_ && b_->dead());
  }
  bool dead() const { return dead_; }

 private:
  std::optional<Alive> a_, b_;
  bool dead_;
};

// Everything between the null checks and the launch that both entries share. The caller holds the life blocks. -3 for a right map
// that does not fit and for the options, before the device is touched; then the left map's state rule, the scratch, the host wait
// for the right map's detection, the clear and the kernel on the left context's track stream.
int enqueue_stereo_prior(const char* who, rebvio_hip_map* m, rebvio_hip_map* r, const rebvio_hip_stereo_prior_opts* opts) {
  const std::string w(who);
  rebvio_hip_ctx* c = m->ctx;
  const rebvio_hip_ctx* rc = r->ctx;
  if (rc->P.rows != c->P.rows || rc->P.cols != c->P.cols) return fail_msg((w + ": the right map has another rows x cols").c_str(), -3);
  if (rc->device != c->device) return fail_msg((w + ": the right map lives on another device").c_str(), -3);
  rebvio_hip_stereo_prior_opts o;
  if (opts) o = *opts; else rebvio_hip_default_stereo_prior_opts(c, &o);
  int rv = check_stereo_prior_opts(who, c->P.cols, o);
  if (rv) return rv;
  rv = depth_prior_state_rule(who, m);
  if (rv) return rv;
  HIPCHK(hipSetDevice(c->device));
  RCCHK(ensure_scratch(c, c->spr, (size_t)c->P.keylines_max, 2));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  if (r != m) {
    // the right map's own detection (+ distance field), on the host: no event of another context enters this stream
    wait_enqueued(r);
    HIPCHK(hipEventSynchronize(r->ready));
  }
  HIPCHK(hipMemsetAsync(c->spr.cnt, 0, 8 * sizeof(int), c->s_trk));
  launch_stereo_prior(c->s_trk, c->K, m->d, r->d, rc->P.keylines_max, spr::make_args(c->P.rows, c->P.cols, c->P.fm, o), c->spr.cnt,
                      c->spr.out, c->spr.out2);
  HIPCHK(hipGetLastError());
  c->spr_queued = true;
  return 0;
}

int fetch_stereo_prior(rebvio_hip_ctx* c, rebvio_hip_stereo_prior_counts* counts, int* outcome_host, int* winner_host) {
  return fetch_prior(c, c->spr, counts, outcome_host, winner_host);
}
}  // namespace

int rebvio_hip_map_fuse_stereo(rebvio_hip_map* m, rebvio_hip_map* r, const rebvio_hip_stereo_prior_opts* opts,
                               rebvio_hip_stereo_prior_counts* counts, int* outcome_host, int* winner_host) {
  if (!m) return fail_msg("map_fuse_stereo: null left map", -3);
  if (!r) return fail_msg("map_fuse_stereo: null right map", -3);
  if (!counts) return fail_msg("map_fuse_stereo: null counts", -3);
  const PairAlive alive(m, r);
  if (alive.dead()) return -10;
  std::memset(counts, 0, sizeof(*counts));
  const int rc = enqueue_stereo_prior("map_fuse_stereo", m, r, opts);
  if (rc) return rc;
  return fetch_stereo_prior(m->ctx, counts, outcome_host, winner_host);
}

int rebvio_hip_map_fuse_stereo_async(rebvio_hip_ctx* c, rebvio_hip_map* m, rebvio_hip_map* r, const rebvio_hip_stereo_prior_opts* opts) {
  if (!c || !m) return fail_msg("map_fuse_stereo_async: null context or left map", -3);
  if (!r) return fail_msg("map_fuse_stereo_async: null right map", -3);
  const PairAlive alive(m, r);
  if (alive.dead()) return -10;
  if (m->ctx != c) return other_context("map_fuse_stereo_async", "left map");
  return enqueue_stereo_prior("map_fuse_stereo_async", m, r, opts);
}

int rebvio_hip_stereo_prior_last_counts(rebvio_hip_ctx* c, rebvio_hip_stereo_prior_counts* counts) {
  if (!c || !counts) return fail_msg("stereo_prior_last_counts: null context or counts", -3);
  std::memset(counts, 0, sizeof(*counts));
  if (!c->spr_queued) return 0;
  HIPCHK(hipSetDevice(c->device));
  return fetch_stereo_prior(c, counts, nullptr, nullptr);
}

int rebvio_hip_test_stereo_prior_host(int rows, int cols, float fm, rebvio_hip_keyline* left, int n, const rebvio_hip_keyline* right, int nr,
                                      const int* right_mask, const rebvio_hip_stereo_prior_opts* opts, rebvio_hip_stereo_prior_counts* counts,
                                      int* outcome, int* winner) {
  if (!counts || n < 0 || nr < 0 || rows < 0 || cols < 0 || (n > 0 && !left) || (nr > 0 && !right) || ((size_t)rows * cols > 0 && !right_mask))
    return fail_msg("test_stereo_prior_host: null array or negative size", -3);
  rebvio_hip_stereo_prior_opts o;
  if (opts) o = *opts; else rebvio_hip_default_stereo_prior_opts(nullptr, &o);
  const int rc = check_stereo_prior_opts("test_stereo_prior_host", cols, o);
  if (rc) return rc;
  const spr::Args a = spr::make_args(rows, cols, fm, o);
  rebvio_hip_stereo_prior_counts res;
  std::memset(&res, 0, sizeof(res));
  res.candidates = n;
  for (int i = 0; i < n; ++i) {
    rebvio_hip_keyline& k = left[i];
    spr::Left L;
    int oc = spr::left_setup(a, k.pos[0], k.pos[1], k.gradient[0], k.gradient[1], k.gradient_norm, k.rho, k.sigma_rho, &L);
    int win = -1;
    if (oc != spr::kUnusable) ++res.usable;
    if (oc < 0) {
      spr::Fold f;
      spr::fold_clear(&f);
      for (int t = 0; t < (a.row_tol ? 3 : 1); ++t) {
        const int y = L.yi + (t == 0 ? 0 : (t == 1 ? -1 : 1));
        if (y < 0 || y >= rows) continue;
        const int* row = right_mask + (size_t)y * cols;
        for (int x = L.x0; x <= L.x1; ++x) {
          const int j = row[x];
          if (j < 0 || j >= nr) continue;
          const rebvio_hip_keyline& q = right[j];
          spr::fold_candidate(a, L, j, q.pos[0], q.pos[1], q.gradient[0], q.gradient[1], q.gradient_norm, &f);
        }
      }
      if (f.seen & 1) ++res.seen;
      oc = spr::decide(a, f);
      if (oc < 0) {
        float rho_n = 0.f, sig_n = 0.f;
        oc = spr::update(a, L, f.d_win, &rho_n, &sig_n);
        if ((oc & 7) == spr::kFused) {
          win = f.j;
          k.rho = rho_n;
          k.sigma_rho = sig_n;
        }
      }
    }
    if ((oc & 7) == spr::kFused) ++res.fused;
    if ((oc & 7) == spr::kGated) ++res.gated;
    if ((oc & 7) == spr::kAmbiguous) ++res.ambiguous;
    if (oc & spr::kClampedBit) ++res.clamped;
    if (outcome) outcome[i] = oc;
    if (winner) winner[i] = win;
  }
  *counts = res;
  return 0;
}

// ---- place recognition (include/rebvio_hip.h is the definition; place.hpp the statements) -------------------------------------------
namespace {
static_assert(sizeof(rebvio_hip_place_match) == 16, "copied from the device as it is");
constexpr size_t kPlcRowBytes = plc::kWords * sizeof(uint16_t);
constexpr size_t kPlcResHead = 16;  // the count, in front of the records

const char* const kPlcPromised = ": the map was handed to track_pair_finish_async with R_prior_next and its gradients are rotated for the "
                                 "next pair; take the signature where the snapshot is taken, or once the next track_pair_begin has run";

// the context's scratch, made at the first signature
int place_scratch(rebvio_hip_ctx* c) { return ensure_scratch(c, c->plc); }

// One clear and the two signature kernels on the track stream (the caller holds the life block and has done its checks).
int enqueue_place_signature(rebvio_hip_ctx* c, rebvio_hip_map* m, uint16_t* sig_dev, int* counted_dev) {
  RCCHK(place_scratch(c));
  if (!sig_dev) {  // the context's own query row
    sig_dev = c->plc.query;
    counted_dev = c->plc.counted;
  }
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  HIPCHK(hipMemsetAsync(c->plc.hist, 0, (plc::kWords + 1) * sizeof(unsigned), c->s_trk));
  launch_place_signature(c->s_trk, c->K, m->d, c->plc.hist, sig_dev, counted_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// The two query kernels over the first `eligible` (> 0) rows, the copy of the count and k records, the tags.
int run_place_query(rebvio_hip_place_db* db, const uint16_t* query_dev, int eligible, int k, rebvio_hip_place_match* out, int* count) {
  rebvio_hip_ctx* c = db->ctx;
  launch_place_query(c->s_trk, db->rows, eligible, query_dev, k, db->dist, db->res);
  HIPCHK(hipGetLastError());
  alignas(16) char host[kPlcResHead + REBVIO_HIP_PLACE_TOPK_MAX * sizeof(rebvio_hip_place_match)];
  HIPCHK(hipMemcpyAsync(host, db->res, kPlcResHead + (size_t)k * sizeof(rebvio_hip_place_match), hipMemcpyDeviceToHost, c->s_trk));
  const int rc = trk_sync(c);
  if (rc) return rc;
  int n = 0;
  std::memcpy(&n, host, sizeof(int));
  if (n < 0 || n > k || n > eligible) return fail_msg("place_db_query: the device returned an impossible count", -2);
  for (int r = 0; r < n; ++r) {
    rebvio_hip_place_match rec;
    std::memcpy(&rec, host + kPlcResHead + (size_t)r * sizeof(rec), sizeof(rec));
    if (rec.index < 0 || rec.index >= eligible) return fail_msg("place_db_query: the device returned an index outside the eligible rows", -2);
    rec.tag = db->tags[(size_t)rec.index];
    out[r] = rec;
  }
  *count = n;
  return 0;
}

int check_place_query_args(const char* who, int k, int exclude_last) {
  if (k < 1 || k > REBVIO_HIP_PLACE_TOPK_MAX) return fail_msg((std::string(who) + ": k outside 1..16").c_str(), -3);
  if (exclude_last < 0) return fail_msg((std::string(who) + ": negative exclude_last").c_str(), -3);
  return 0;
}
}  // namespace

int rebvio_hip_map_place_signature(rebvio_hip_map* m, uint16_t* sig, int* counted) {
  if (!m || !sig || !counted) return fail_msg("map_place_signature: null map, signature or counted", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  if (m->promised.load(std::memory_order_acquire)) return fail_msg((std::string("map_place_signature") + kPlcPromised).c_str(), -7);
  HIPCHK(hipSetDevice(c->device));
  int rc = enqueue_place_signature(c, m, nullptr, nullptr);
  if (rc) return rc;
  // (the row and its counted word lie next to each other: one copy)
  alignas(4) char host[kPlcRowBytes + sizeof(int)];
  HIPCHK(hipMemcpyAsync(host, c->plc.query, sizeof(host), hipMemcpyDeviceToHost, c->s_trk));
  rc = trk_sync(c);
  if (rc) return rc;
  std::memcpy(sig, host, kPlcRowBytes);
  std::memcpy(counted, host + kPlcRowBytes, sizeof(int));
  return 0;
}

int rebvio_hip_place_db_create(rebvio_hip_ctx* c, int cap, rebvio_hip_place_db** out) {
  if (out) *out = nullptr;
  if (!c || !out) return fail_msg("place_db_create: null context or output", -3);
  if (cap < 1 || cap > 65536) return fail_msg("place_db_create: cap outside 1..65536", -3);
  HIPCHK(hipSetDevice(c->device));
  auto* db = new rebvio_hip_place_db;
  db->ctx = c;
  db->life = c->life;
  db->cap = cap;
  char* rows = nullptr;
  char* aux = nullptr;
  hipError_t e = db->own.device_bytes(&rows, (size_t)cap * kPlcRowBytes);
  const size_t words = ((size_t)cap + 3) / 4 * 4;  // (keeps the result block 16-byte aligned)
  if (e == hipSuccess) e = db->own.device_bytes(&aux, words * (sizeof(unsigned) + sizeof(int)) + kPlcResHead +
                                                          REBVIO_HIP_PLACE_TOPK_MAX * sizeof(rebvio_hip_place_match));
  if (e != hipSuccess) {
    delete db;
    return fail("place_db_create: device buffers", e);
  }
  db->rows = reinterpret_cast<uint16_t*>(rows);
  db->dist = reinterpret_cast<unsigned*>(aux);
  db->counted = reinterpret_cast<int*>(aux + words * sizeof(unsigned));
  db->res = aux + words * (sizeof(unsigned) + sizeof(int));
  try {
    db->tags.reserve((size_t)cap);
    std::lock_guard<std::mutex> lk(c->place_mu);
    c->place_dbs.push_back(db);
  } catch (...) {
    delete db;
    return fail_msg("place_db_create: out of host memory", -2);
  }
  *out = db;
  return 0;
}

void rebvio_hip_place_db_release(rebvio_hip_place_db* db) {
  unlist_and_release(&rebvio_hip_ctx::place_dbs, &rebvio_hip_ctx::place_mu, db);
}

int rebvio_hip_place_db_clear(rebvio_hip_place_db* db) {
  if (!db) return fail_msg("place_db_clear: null database", -3);
  const Alive alive(db);
  if (alive.dead()) return -10;
  db->size = 0;
  db->tags.clear();
  return 0;
}

int rebvio_hip_place_db_size(rebvio_hip_place_db* db) {
  if (!db) return fail_msg("place_db_size: null database", -3);
  const Alive alive(db);
  if (alive.dead()) return -10;
  return db->size;
}

int rebvio_hip_place_db_add(rebvio_hip_place_db* db, rebvio_hip_map* m, uint64_t tag, int* index) {
  if (!db || !m) return fail_msg("place_db_add: null database or map", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(of_map_context("place_db_add", db, m, "map", " than the database's"));
  rebvio_hip_ctx* c = db->ctx;
  if (m->promised.load(std::memory_order_acquire)) return fail_msg((std::string("place_db_add") + kPlcPromised).c_str(), -7);
  if (db->size >= db->cap) return fail_msg("place_db_add: the database is full", -7);
  HIPCHK(hipSetDevice(c->device));
  const int i = db->size;
  const int rc = enqueue_place_signature(c, m, db->rows + (size_t)i * plc::kWords, db->counted + i);
  if (rc) return rc;
  db->tags.push_back(tag);  // (room reserved at create)
  db->size = i + 1;
  if (index) *index = i;
  return 0;
}

int rebvio_hip_place_db_add_signature(rebvio_hip_place_db* db, const uint16_t* sig, int counted, uint64_t tag, int* index) {
  if (!db || !sig) return fail_msg("place_db_add_signature: null database or signature", -3);
  if (counted < 0) return fail_msg("place_db_add_signature: negative counted", -3);
  const Alive alive(db);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = db->ctx;
  if (db->size >= db->cap) return fail_msg("place_db_add_signature: the database is full", -7);
  HIPCHK(hipSetDevice(c->device));
  const int i = db->size;
  HIPCHK(hipMemcpyAsync(db->rows + (size_t)i * plc::kWords, sig, kPlcRowBytes, hipMemcpyHostToDevice, c->s_trk));
  HIPCHK(hipMemcpyAsync(db->counted + i, &counted, sizeof(int), hipMemcpyHostToDevice, c->s_trk));
  const int rc = trk_sync(c);
  if (rc) return rc;
  db->tags.push_back(tag);
  db->size = i + 1;
  if (index) *index = i;
  return 0;
}

int rebvio_hip_place_db_entry(rebvio_hip_place_db* db, int index, uint16_t* sig, int* counted, uint64_t* tag) {
  if (!db) return fail_msg("place_db_entry: null database", -3);
  const Alive alive(db);
  if (alive.dead()) return -10;
  if (index < 0 || index >= db->size) return fail_msg("place_db_entry: index outside [0, size)", -3);
  rebvio_hip_ctx* c = db->ctx;
  HIPCHK(hipSetDevice(c->device));
  int n = 0;
  if (sig) HIPCHK(hipMemcpyAsync(sig, db->rows + (size_t)index * plc::kWords, kPlcRowBytes, hipMemcpyDeviceToHost, c->s_trk));
  if (counted) HIPCHK(hipMemcpyAsync(&n, db->counted + index, sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  const int rc = trk_sync(c);
  if (rc) return rc;
  if (counted) *counted = n;
  if (tag) *tag = db->tags[(size_t)index];
  return 0;
}

int rebvio_hip_place_db_query(rebvio_hip_place_db* db, rebvio_hip_map* m, int k, int exclude_last, rebvio_hip_place_match* out, int* count) {
  if (count) *count = 0;
  if (!db || !m || !out || !count) return fail_msg("place_db_query: null database, map, output or count", -3);
  int rc = check_place_query_args("place_db_query", k, exclude_last);
  if (rc) return rc;
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(of_map_context("place_db_query", db, m, "map", " than the database's"));
  rebvio_hip_ctx* c = db->ctx;
  if (m->promised.load(std::memory_order_acquire)) return fail_msg((std::string("place_db_query") + kPlcPromised).c_str(), -7);
  const int eligible = db->size - exclude_last;
  if (eligible <= 0) return 0;  // nothing is launched
  HIPCHK(hipSetDevice(c->device));
  rc = enqueue_place_signature(c, m, nullptr, nullptr);
  if (rc) return rc;
  return run_place_query(db, c->plc.query, eligible, k, out, count);
}

int rebvio_hip_place_db_query_signature(rebvio_hip_place_db* db, const uint16_t* sig, int k, int exclude_last, rebvio_hip_place_match* out,
                                        int* count) {
  if (count) *count = 0;
  if (!db || !sig || !out || !count) return fail_msg("place_db_query_signature: null database, signature, output or count", -3);
  int rc = check_place_query_args("place_db_query_signature", k, exclude_last);
  if (rc) return rc;
  const Alive alive(db);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = db->ctx;
  const int eligible = db->size - exclude_last;
  if (eligible <= 0) return 0;  // nothing is launched
  HIPCHK(hipSetDevice(c->device));
  RCCHK(place_scratch(c));
  HIPCHK(hipMemcpyAsync(c->plc.query, sig, kPlcRowBytes, hipMemcpyHostToDevice, c->s_trk));
  return run_place_query(db, c->plc.query, eligible, k, out, count);
}

int rebvio_hip_test_place_signature_host(int rows, int cols, const rebvio_hip_keyline* keylines, int n, uint16_t* sig, int* counted) {
  if (!sig || !counted || n < 0 || (n > 0 && !keylines)) return fail_msg("test_place_signature_host: null array or negative size", -3);
  if (rows < 1 || cols < 1) return fail_msg("test_place_signature_host: rows or cols < 1", -3);
  plc::signature_host(rows, cols, keylines, n, sig, counted);
  return 0;
}

int rebvio_hip_test_place_query_host(const uint16_t* rows384, int size, const uint16_t* sig, int k, int exclude_last,
                                     rebvio_hip_place_match* out, int* count) {
  if (count) *count = 0;
  if (!sig || !out || !count || size < 0 || (size > 0 && !rows384)) return fail_msg("test_place_query_host: null array or negative size", -3);
  const int rc = check_place_query_args("test_place_query_host", k, exclude_last);
  if (rc) return rc;
  plc::query_host(rows384, size, sig, k, exclude_last, out, count);
  return 0;
}

void rebvio_hip_default_kf_handover_opts(rebvio_hip_ctx* c, rebvio_hip_kf_handover_opts* o) {
  std::memset(o, 0, sizeof(*o));
  rebvio_hip_default_cloud_filter(&o->kf_filter);
  o->min_cos = 0.9;
  o->gate_sigma = 3.0;
  o->q_abs = 0.0;
  o->max_dist = c ? (int)c->P.search_range : 40;
}

namespace {
int check_kf_handover_args(const char* who, const rebvio_hip_kf_handover_opts& o, int search_range, const double* R, const double* t) {
  return check_kf_depth_args(who, o.kf_filter, nullptr, o.gate_sigma, o.q_abs, o.min_cos, o.max_dist, o.reserved, search_range, R, t);
}
}  // namespace

static_assert(sizeof(rebvio_hip_kf_handover_opts) == 48, "filter, three doubles, two ints");
static_assert(sizeof(rebvio_hip_kf_handover) == 28, "seven ints");
static_assert(sizeof(kfp::HandoverStage) == 8, "one 8-byte store");

int rebvio_hip_kf_snapshot_handover_depth(rebvio_hip_kf_snapshot* dst, rebvio_hip_kf_snapshot* src, rebvio_hip_map* m,
                                          const rebvio_hip_kf_handover_opts* opts, const double* R, const double* t,
                                          rebvio_hip_kf_handover* out, int* assoc_host) {
  if (!dst || !src || !m || !out) return fail_msg("kf_snapshot_handover_depth: null snapshot, map or output", -3);
  if (dst == src) return fail_msg("kf_snapshot_handover_depth: dst and src are the same snapshot", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  RCCHK(snapshot_of("kf_snapshot_handover_depth", dst, m));
  RCCHK(snapshot_of("kf_snapshot_handover_depth", src, m));
  rebvio_hip_ctx* c = m->ctx;
  rebvio_hip_kf_handover_opts o;
  if (opts) o = *opts; else rebvio_hip_default_kf_handover_opts(c, &o);
  RCCHK(check_kf_handover_args("kf_snapshot_handover_depth", o, (int)c->P.search_range, R, t));
  RCCHK(needs_detection_field("kf_snapshot_handover_depth", m));
  HIPCHK(hipSetDevice(c->device));
  RCCHK(snapshot_size(c, src));
  const int kf_size = src->n_host;
  std::memset(out, 0, sizeof(*out));
  if (kf_size == 0) return 0;  // nothing to hand over: nothing is launched
  RCCHK(snapshot_size(c, dst));
  const int dst_size = dst->n_host;
  RCCHK(ensure_scratch(c, c->kfh, (size_t)c->P.keylines_max));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  {
    // both snapshots are this call's from the clears to the kernels; in address order: std::mutex is not recursive (dst != src) and
    // two threads may name the pair in opposite roles
    std::mutex* first = &dst->nor_mu;
    std::mutex* second = &src->nor_mu;
    if (std::less<std::mutex*>()(second, first)) std::swap(first, second);
    std::lock_guard<std::mutex> l1(*first);
    std::lock_guard<std::mutex> l2(*second);
    if (dst_size > 0) HIPCHK(hipMemsetAsync(c->kfh.key, 0xFF, (size_t)dst_size * sizeof(unsigned long long), c->s_trk));
    HIPCHK(hipMemsetAsync(c->kfh.cnt, 0, 8 * sizeof(int), c->s_trk));
    launch_kf_handover(c->s_trk, c->K, m->d, kf_size, src->n_dev, dst_size, dst->n_dev, src->prs, src->matches, src->normals, dst->prs,
                       dst->matches, o, R, t, c->kfh.key, c->kfh.stage, c->kfh.cnt, c->kfh.assoc);
    HIPCHK(hipGetLastError());
  }
  return fetch_counted(c, c->kfh.cnt, c->kfh.assoc, kf_size, out, assoc_host);
}

int rebvio_hip_test_kf_handover_host(float fm, float cx, float cy, int rows, int cols, int search_range, const float* src_prs4,
                                     const unsigned* src_matches, const float* src_normals, int kf_size, const float* cur_pos,
                                     const float* cur_unit, int n_cur, const int* df_id, const int* df_dist, float* dst_prs4,
                                     unsigned* dst_matches, int dst_size, const rebvio_hip_kf_handover_opts* opts, const double* R,
                                     const double* t, rebvio_hip_kf_handover* out, int* assoc) {
  if (!out || kf_size < 0 || n_cur < 0 || dst_size < 0 || rows < 0 || cols < 0 || (kf_size > 0 && (!src_prs4 || !src_matches)) ||
      (dst_size > 0 && (!dst_prs4 || !dst_matches)) || (n_cur > 0 && (!cur_pos || !cur_unit)) ||
      ((size_t)rows * (size_t)cols > 0 && (!df_id || !df_dist)))
    return fail_msg("test_kf_handover_host: null array or negative size", -3);
  rebvio_hip_kf_handover_opts o;
  if (opts) {
    o = *opts;
  } else {
    rebvio_hip_default_kf_handover_opts(nullptr, &o);
    o.max_dist = search_range;
  }
  const int rc = check_kf_handover_args("test_kf_handover_host", o, search_range, R, t);
  if (rc) return rc;
  const size_t Pn = (size_t)rows * (size_t)cols;
  for (size_t k = 0; k < Pn; ++k)
    if (df_id[k] >= n_cur) return fail_msg("test_kf_handover_host: a field id lies outside the keyline arrays", -3);
  const kfp::AlignMap am = kfp::host_map(fm, cx, cy, rows, cols, df_id, df_dist, cur_pos, cur_unit, n_cur);
  rebvio_hip_kf_handover res;
  std::vector<unsigned long long> key((size_t)dst_size);
  std::vector<kfp::HandoverStage> stage((size_t)kf_size);
  std::vector<int> as((size_t)kf_size);
  kfp::handover_host(am, src_prs4, src_matches, src_normals, kf_size, dst_prs4, dst_matches, dst_size, o, R, t, key.data(), stage.data(),
                     as.data(), &res);
  if (assoc)
    for (int j = 0; j < kf_size; ++j) assoc[j] = as[(size_t)j];
  *out = res;
  return 0;
}

}  // extern "C"

namespace {
static_assert(sizeof(rebvio_hip_chain_ref) == 16 && sizeof(rebvio_hip_polyline) == 16 && sizeof(ech::ChainNode) == 16,
              "16-byte records: one load, one store");
static_assert(sizeof(rebvio_hip_polyline_opts) == 24, "filter, two ints");

// What both entries do up to their launches: the state rule, the scratch, the waits. The caller holds the map's life block.
int ech_begin(const char* who, rebvio_hip_map* m) {
  rebvio_hip_ctx* c = m->ctx;
  if (m->promised.load(std::memory_order_acquire))
    return fail_msg((std::string(who) + ": the map was handed to track_pair_finish_async with R_prior_next and is rotated for the next pair; "
                     "it is available again once the next track_pair_begin has run").c_str(), -7);
  HIPCHK(hipSetDevice(c->device));
  RCCHK(ensure_scratch(c, c->ech, (size_t)c->P.keylines_max, (size_t)kMaxRecBlocks, (size_t)kChainWords));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  return 0;
}

int check_polyline_args(const char* who, const rebvio_hip_polyline_opts* o, const rebvio_hip_cloud_pose* pose, const void* points,
                        int cap_points, const void* lines, int cap_lines, const int* n_points, const int* n_lines) {
  if (!n_points || !n_lines) return fail_msg((std::string(who) + ": null n_points or n_lines").c_str(), -3);
  if (cap_points < 0 || (cap_points > 0 && !points))
    return fail_msg((std::string(who) + ": cap_points records need a points buffer (cap_points >= 0)").c_str(), -3);
  if (cap_lines < 0 || (cap_lines > 0 && !lines))
    return fail_msg((std::string(who) + ": cap_lines records need a lines buffer (cap_lines >= 0)").c_str(), -3);
  if (o && o->min_chain_length < 1) return fail_msg((std::string(who) + ": min_chain_length must be >= 1").c_str(), -3);
  return check_cloud_args(who, o ? &o->filter : nullptr, pose);
}
}  // namespace

extern "C" {

int rebvio_hip_map_edge_chains(rebvio_hip_map* m, rebvio_hip_chain_ref* refs_host, int cap_keylines, int* order_host, int* starts_host,
                               int cap_chains, int* n_keylines, int* n_chains) {
  if (!m) return fail_msg("map_edge_chains: null map", -3);
  if (cap_keylines < 0 || cap_chains < 0) return fail_msg("map_edge_chains: negative cap", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  if (n_keylines) *n_keylines = 0;
  if (n_chains) *n_chains = 0;
  int rc = ech_begin("map_edge_chains", m);
  if (rc) return rc;
  launch_edge_chains(c->s_trk, c->K, m->d, c->ech, ech::chain_rounds(c->P.keylines_max));
  HIPCHK(hipGetLastError());
  // the counts first; then copies of exactly what exists
  int w[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(w, c->ech.words, sizeof(w), hipMemcpyDeviceToHost, c->s_trk));
  rc = trk_sync(c);
  if (rc) return rc;
  const int n = w[0], nc = w[1];
  const size_t kn = (size_t)(n < cap_keylines ? n : cap_keylines), ks = (size_t)(nc + 1 < cap_chains ? nc + 1 : cap_chains);
  if (refs_host && kn) HIPCHK(hipMemcpyAsync(refs_host, c->ech.refs, kn * sizeof(rebvio_hip_chain_ref), hipMemcpyDeviceToHost, c->s_trk));
  if (order_host && kn) HIPCHK(hipMemcpyAsync(order_host, c->ech.order, kn * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  if (starts_host && ks) HIPCHK(hipMemcpyAsync(starts_host, c->ech.starts, ks * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  rc = trk_sync(c);
  if (rc) return rc;
  if (n_keylines) *n_keylines = n;
  if (n_chains) *n_chains = nc;
  return 0;
}

void rebvio_hip_default_polyline_opts(rebvio_hip_polyline_opts* o) {
  rebvio_hip_default_cloud_filter(&o->filter);
  o->min_chain_length = 8;
  o->reserved = 0;
}

int rebvio_hip_map_edge_polylines(rebvio_hip_map* m, const rebvio_hip_polyline_opts* opts, const rebvio_hip_cloud_pose* pose,
                                  rebvio_hip_cloud_point* points_host, int* refs2_host, int cap_points, rebvio_hip_polyline* lines_host,
                                  int cap_lines, int* n_points, int* n_lines) {
  if (!m) return fail_msg("map_edge_polylines: null map", -3);
  int rc = check_polyline_args("map_edge_polylines", opts, pose, points_host, cap_points, lines_host, cap_lines, n_points, n_lines);
  if (rc) return rc;
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  *n_points = *n_lines = 0;
  rc = ech_begin("map_edge_polylines", m);
  if (rc) return rc;
  rebvio_hip_polyline_opts o;
  if (opts) o = *opts; else rebvio_hip_default_polyline_opts(&o);
  const CloudArgs a = cloud_args(c, &o.filter, pose, cap_points);
  if (cap_lines > c->P.keylines_max) cap_lines = c->P.keylines_max;  // (no more lines than keylines)
  launch_edge_chains(c->s_trk, c->K, m->d, c->ech, ech::chain_rounds(c->P.keylines_max));
  launch_edge_polylines(c->s_trk, c->K, m->d, c->ech, a, o.min_chain_length, cap_lines);
  HIPCHK(hipGetLastError());
  int w[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(w, c->ech.words, sizeof(w), hipMemcpyDeviceToHost, c->s_trk));
  rc = trk_sync(c);
  if (rc) return rc;
  const int np = w[2], nl = w[3];
  const size_t kp = (size_t)(np < a.cap ? np : a.cap), kl = (size_t)(nl < cap_lines ? nl : cap_lines);
  if (kp) HIPCHK(hipMemcpyAsync(points_host, c->ech.points, kp * sizeof(rebvio_hip_cloud_point), hipMemcpyDeviceToHost, c->s_trk));
  if (kp && refs2_host) HIPCHK(hipMemcpyAsync(refs2_host, c->ech.refs2, kp * sizeof(int2), hipMemcpyDeviceToHost, c->s_trk));
  if (kl) HIPCHK(hipMemcpyAsync(lines_host, c->ech.lines, kl * sizeof(rebvio_hip_polyline), hipMemcpyDeviceToHost, c->s_trk));
  rc = trk_sync(c);
  if (rc) return rc;
  *n_points = np;
  *n_lines = nl;
  return 0;
}

int rebvio_hip_test_edge_chains_host(const int* id_prev, const int* id_next, int n, rebvio_hip_chain_ref* refs, int cap_keylines, int* order,
                                     int* starts, int cap_chains, int* n_keylines, int* n_chains) {
  if (n < 0 || (n > 0 && (!id_prev || !id_next))) return fail_msg("test_edge_chains_host: negative n or null links", -3);
  if (cap_keylines < 0 || cap_chains < 0) return fail_msg("test_edge_chains_host: negative cap", -3);
  const size_t N = (size_t)n;
  std::vector<ech::ChainNode> a(N), b(N);
  std::vector<int> succ(N), len(N), start_of(N), ord(N), st(N + 1);
  std::vector<rebvio_hip_chain_ref> rf(N);
  int nc = 0;
  ech::chains_host(id_prev, id_next, n, a.data(), b.data(), succ.data(), len.data(), start_of.data(), rf.data(), ord.data(), st.data(), &nc);
  const size_t kn = (size_t)(n < cap_keylines ? n : cap_keylines), ks = (size_t)(nc + 1 < cap_chains ? nc + 1 : cap_chains);
  if (refs && kn) std::memcpy(refs, rf.data(), kn * sizeof(rebvio_hip_chain_ref));
  if (order && kn) std::memcpy(order, ord.data(), kn * sizeof(int));
  if (starts && ks) std::memcpy(starts, st.data(), ks * sizeof(int));
  if (n_keylines) *n_keylines = n;
  if (n_chains) *n_chains = nc;
  return 0;
}

int rebvio_hip_test_edge_polylines_host(float fm, const rebvio_hip_keyline* keylines, int n, const rebvio_hip_polyline_opts* opts,
                                        const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud_point* points, int* refs2, int cap_points,
                                        rebvio_hip_polyline* lines, int cap_lines, int* n_points, int* n_lines) {
  if (n < 0 || (n > 0 && !keylines)) return fail_msg("test_edge_polylines_host: negative n or null keylines", -3);
  const int rc = check_polyline_args("test_edge_polylines_host", opts, pose, points, cap_points, lines, cap_lines, n_points, n_lines);
  if (rc) return rc;
  rebvio_hip_polyline_opts o;
  if (opts) o = *opts; else rebvio_hip_default_polyline_opts(&o);
  const size_t N = (size_t)n;
  std::vector<int> idp(N), idn(N), succ(N), len(N), start_of(N), ord(N), st(N + 1);
  std::vector<float> pos_img(2 * N), rs(2 * N), gn(N);
  std::vector<unsigned> mt(N);
  for (size_t i = 0; i < N; ++i) {
    const rebvio_hip_keyline& k = keylines[i];
    idp[i] = k.id_prev; idn[i] = k.id_next;
    pos_img[2 * i] = k.pos_img[0]; pos_img[2 * i + 1] = k.pos_img[1];
    rs[2 * i] = k.rho; rs[2 * i + 1] = k.sigma_rho;
    gn[i] = k.gradient_norm;
    mt[i] = k.matches;
  }
  std::vector<ech::ChainNode> a(N), b(N);
  std::vector<rebvio_hip_chain_ref> rf(N);
  int nc = 0;
  ech::chains_host(idp.data(), idn.data(), n, a.data(), b.data(), succ.data(), len.data(), start_of.data(), rf.data(), ord.data(), st.data(), &nc);
  float R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = pose ? pose->R[i] : (i % 4 == 0 ? 1.0f : 0.0f);
  for (int i = 0; i < 3; ++i) t[i] = pose ? pose->t[i] : 0.0f;
  ech::polylines_host(fm, pos_img.data(), rs.data(), gn.data(), mt.data(), n, rf.data(), ord.data(), o, R, t, pose ? pose->scale : 1.0f, points,
                      refs2, cap_points, lines, cap_lines, n_points, n_lines);
  return 0;
}

}  // extern "C"

namespace {
static_assert(sizeof(rebvio_hip_line_segment) == 80 && sizeof(esg::SegPoint) == 16 && sizeof(esg::SegSpan) == 8,
              "an 80-byte record: five 16-byte stores; a point: one load");
static_assert(sizeof(rebvio_hip_segment_opts) == 40 && sizeof(rebvio_hip_segment_counts) == 32, "the polyline options and four words; eight ints");

int check_segment_args(const char* who, const rebvio_hip_segment_opts* o, const rebvio_hip_cloud_pose* pose, const void* segs, int cap,
                       const rebvio_hip_segment_counts* counts) {
  if (!counts) return fail_msg((std::string(who) + ": null counts").c_str(), -3);
  if (cap < 0 || (cap > 0 && !segs)) return fail_msg((std::string(who) + ": cap_segments records need a segs buffer (cap_segments >= 0)").c_str(), -3);
  if (o) {
    if (!(o->tol >= 0.0f) || !(o->min_length >= 0.0f)) return fail_msg((std::string(who) + ": tol and min_length must be >= 0").c_str(), -3);
    if (o->min_points < 2) return fail_msg((std::string(who) + ": min_points must be >= 2").c_str(), -3);
    if (o->max_rounds < 1 || o->max_rounds > esg::kMaxRounds) return fail_msg((std::string(who) + ": max_rounds must be in 1..32").c_str(), -3);
    if (o->poly.min_chain_length < 1) return fail_msg((std::string(who) + ": min_chain_length must be >= 1").c_str(), -3);
  }
  return check_cloud_args(who, o ? &o->poly.filter : nullptr, pose);
}
}  // namespace

extern "C" {

void rebvio_hip_default_segment_opts(rebvio_hip_segment_opts* o) {
  rebvio_hip_default_polyline_opts(&o->poly);
  o->tol = 1.0f;
  o->min_length = 4.0f;
  o->min_points = 8;
  o->max_rounds = 16;
}

int rebvio_hip_map_edge_segments(rebvio_hip_map* m, const rebvio_hip_segment_opts* opts, const rebvio_hip_cloud_pose* pose,
                                 rebvio_hip_line_segment* segs_host, int cap_segments, rebvio_hip_segment_counts* counts) {
  if (!m) return fail_msg("map_edge_segments: null map", -3);
  int rc = check_segment_args("map_edge_segments", opts, pose, segs_host, cap_segments, counts);
  if (rc) return rc;
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  std::memset(counts, 0, sizeof(*counts));
  rc = ech_begin("map_edge_segments", m);
  if (rc) return rc;
  RCCHK(ensure_scratch(c, c->esg, (size_t)c->P.keylines_max, (size_t)kMaxRecBlocks, (size_t)esg::kSegWords));
  rebvio_hip_segment_opts o;
  if (opts) o = *opts; else rebvio_hip_default_segment_opts(&o);
  // every point and line stays on the device: the polylines run with both caps at keylines_max
  const CloudArgs a = cloud_args(c, &o.poly.filter, pose, -1);
  const SegArgs sa{o.tol * o.tol, o.min_length * o.min_length, o.min_points, o.max_rounds};
  launch_edge_chains(c->s_trk, c->K, m->d, c->ech, ech::chain_rounds(c->P.keylines_max));
  launch_edge_polylines(c->s_trk, c->K, m->d, c->ech, a, o.poly.min_chain_length, c->P.keylines_max);
  launch_edge_segments(c->s_trk, c->K, m->d, c->ech, c->esg, a, sa);
  HIPCHK(hipGetLastError());
  int w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(w, c->esg.words, sizeof(w), hipMemcpyDeviceToHost, c->s_trk));
  rc = trk_sync(c);
  if (rc) return rc;
  const size_t ks = (size_t)(w[3] < cap_segments ? w[3] : cap_segments);
  if (ks) {
    HIPCHK(hipMemcpyAsync(segs_host, c->esg.recs, ks * sizeof(rebvio_hip_line_segment), hipMemcpyDeviceToHost, c->s_trk));
    rc = trk_sync(c);
    if (rc) return rc;
  }
  *counts = rebvio_hip_segment_counts{w[2], w[3], w[4], w[5], w[6], w[0], w[1], 0};
  return 0;
}

int rebvio_hip_test_edge_segments_host(float fm, const rebvio_hip_keyline* keylines, int n, const rebvio_hip_segment_opts* opts,
                                       const rebvio_hip_cloud_pose* pose, rebvio_hip_line_segment* segs, int cap_segments,
                                       rebvio_hip_segment_counts* counts) {
  if (n < 0 || (n > 0 && !keylines)) return fail_msg("test_edge_segments_host: negative n or null keylines", -3);
  int rc = check_segment_args("test_edge_segments_host", opts, pose, segs, cap_segments, counts);
  if (rc) return rc;
  rebvio_hip_segment_opts o;
  if (opts) o = *opts; else rebvio_hip_default_segment_opts(&o);
  const size_t N = (size_t)n;
  std::vector<rebvio_hip_cloud_point> pts(N);
  std::vector<rebvio_hip_polyline> lines(N);
  int np = 0, nl = 0;
  rc = rebvio_hip_test_edge_polylines_host(fm, keylines, n, &o.poly, pose, pts.data(), nullptr, n, lines.data(), n, &np, &nl);
  if (rc) return rc;
  std::vector<esg::SegPoint> q((size_t)np);
  for (int p = 0; p < np; ++p) {
    const rebvio_hip_keyline& k = keylines[pts[(size_t)p].keyline];
    q[(size_t)p] = esg::SegPoint{k.pos_img[0], k.pos_img[1], k.rho, k.sigma_rho};
  }
  std::vector<esg::SegSpan> span((size_t)np);
  std::vector<int> nxt((size_t)np), line_of((size_t)np);
  std::vector<unsigned long long> far((size_t)np);
  float R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = pose ? pose->R[i] : (i % 4 == 0 ? 1.0f : 0.0f);
  for (int i = 0; i < 3; ++i) t[i] = pose ? pose->t[i] : 0.0f;
  esg::segments_host(fm, q.data(), np, lines.data(), nl, o, R, t, pose ? pose->scale : 1.0f, span.data(), nxt.data(), line_of.data(), far.data(),
                     segs, cap_segments, counts);
  return 0;
}

}  // extern "C"

extern "C" {

int rebvio_hip_map_upload(rebvio_hip_map* m, const rebvio_hip_keyline* keylines, int n) {
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_size(m);
  if (rc) return rc;
  if (n != m->n_host) return fail_msg("map_upload: count differs from map size", -6);
  std::lock_guard<std::mutex> dl(c->dl_mu);
  HIPCHK(hipStreamSynchronize(c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_key));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(c->aos_dev, keylines, (size_t)n * sizeof(rebvio_hip_keyline), hipMemcpyHostToDevice, c->s_key));
    launch_map_unpack(c->s_key, c->K, m->d, c->aos_dev, n);
  }
  HIPCHK(hipStreamSynchronize(c->s_key));
  m->df_built = false;
  m->raster_order = false;  // arbitrary keylines: the rebuild goes through the scatter kernel
  return 0;
}

int rebvio_hip_test_map_set_mask(rebvio_hip_map* m, const int* mask) {
  if (!m || !mask) return fail_msg("test_map_set_mask: null map or mask", -3);
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_size(m);
  if (rc) return rc;
  for (size_t k = 0; k < Pn; ++k)
    if (mask[k] < -1 || mask[k] >= m->n_host) return fail_msg("test_map_set_mask: a word outside [-1, size)", -3);
  std::lock_guard<std::mutex> dl(c->dl_mu);
  HIPCHK(hipStreamSynchronize(c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_key));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  HIPCHK(hipMemcpyAsync(m->d.mask, mask, Pn * sizeof(int), hipMemcpyHostToDevice, c->s_key));
  HIPCHK(hipStreamSynchronize(c->s_key));
  m->df_built = false;
  return 0;
}

void rebvio_hip_map_release(rebvio_hip_map* m) {
  if (!m) return;
  const std::shared_ptr<LifeBlock> life = m->life;
  std::shared_lock<std::shared_mutex> lk(life->mu);  // (against destroy; the pool's own state is under the context's pool_mu)
  if (life->dead.load(std::memory_order_acquire)) {  // the context is gone (its memory with it): drop the husk
    if (m->in_use) delete m;
    return;
  }
  (void)hipSetDevice(m->ctx->device);
  release_map(m);
}

}  // extern "C"

namespace {
// Stream-ordered return of a map to its pool (the library's own releases call this directly; the C-ABI entry adds the
// lifetime check and selects the device).
// done_ref: an event already recorded behind the map's last consumer. Null: one is recorded here on the track stream, unless
// record_done is false (a batch releases a step's maps at one point of the track stream, and only its last lane's is marked:
// the detect stage waits for that one event).
// done_token: no event; the map is idle once its context's pair queue has proven that many steps complete (PairQueue::proven).
void release_map(rebvio_hip_map* m, hipEvent_t done_ref, bool record_done, uint64_t done_token) {
  if (!m || !m->in_use) return;
  rebvio_hip_ctx* c = m->ctx;
  wait_enqueued(m);
  // a pair's counters still waiting in this map's state record (track_pair_finish_async without its _result yet): copy them
  // out in stream order before the map can be handed to another frame
  if (c->h_bf && c->bf_res >= 0 && c->bf_map[c->bf_res] == m && !c->bf_have[c->bf_res] && !c->bf_copy_queued[c->bf_res]) {
    const int r = c->bf_res;
    if (hipMemcpyAsync(&c->h_bf[r], m->d.st, sizeof(MapState), hipMemcpyDeviceToHost, c->s_trk) == hipSuccess &&
        hipEventRecord(c->bf_done[r], c->s_trk) == hipSuccess)
      c->bf_copy_queued[r] = true;
  }
  std::lock_guard<std::mutex> pool_lk(c->pool_mu);
  m->done_ref = done_token ? nullptr : done_ref;
  m->done_token = done_token;
  if (done_ref || done_token) {
    m->has_done = true;
  } else if (record_done) {
    (void)record_counted(c, kOnTrk, c->s_trk, m->done);
    m->has_done = true;
  }
  if (c->df_map == m) c->df_map = nullptr;
  m->release_seq = ++c->release_counter;
  m->kf_flag = false;  // (a flagged frame dropped untracked must not hand its request to the frame that reuses the map)
  m->in_use = false;  // (c->last_detected may keep pointing at it: only its MapState is read, stream-ordered)
}
}  // namespace

extern "C" {

int rebvio_hip_build_distance_field(rebvio_hip_ctx* c, rebvio_hip_map* m) {
  HIPCHK(hipSetDevice(c->device));
  wait_enqueued(m);
  HIPCHK(trk_wait_ready_once(c, m));
  if (!m->df_built) {
    if (!m->raster_order) HIPCHK(hipMemsetAsync(m->d.df, 0xFF, (size_t)c->P.rows * c->P.cols * sizeof(unsigned), c->s_trk));
    launch_df_build(c->s_trk, c->K, m->d, c->det + (c->frame_index % kDetRing), m->raster_order);  // keylines may have been uploaded
    HIPCHK(hipGetLastError());
    m->df_built = true;
  }
  c->df_map = m;
  return 0;
}

int rebvio_hip_distance_field(rebvio_hip_ctx* c, int* id_out, int* dist_out) {
  HIPCHK(hipSetDevice(c->device));
  if (!c->df_map) return fail_msg("no distance field built", -7);
  std::lock_guard<std::mutex> dl(c->dl_mu);
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  launch_df_decode(c->s_trk, c->K, c->df_map->d, c->scratch_i, c->scratch_i + Pn);
  HIPCHK(hipGetLastError());
  if (id_out) HIPCHK(hipMemcpyAsync(id_out, c->scratch_i, Pn * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, c->scratch_i + Pn, Pn * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  return 0;
}

int rebvio_hip_map_distance_field(rebvio_hip_map* m, int* id_out, int* dist_out) {
  const Alive alive(m);
  if (alive.dead()) return -10;
  rebvio_hip_ctx* c = m->ctx;
  HIPCHK(hipSetDevice(c->device));
  if (!m->df_built) return fail_msg("map_distance_field: no distance field has been built from this map", -7);
  wait_enqueued(m);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  std::lock_guard<std::mutex> dl(c->dl_mu);
  const size_t Pn = (size_t)c->P.rows * c->P.cols;
  launch_df_decode(c->s_trk, c->K, m->d, c->scratch_i, c->scratch_i + Pn);
  HIPCHK(hipGetLastError());
  if (id_out) HIPCHK(hipMemcpyAsync(id_out, c->scratch_i, Pn * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, c->scratch_i + Pn, Pn * sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  return 0;
}

int rebvio_hip_search_match(rebvio_hip_ctx* c, rebvio_hip_map* searched, const rebvio_hip_keyline* query, const float vel[3],
                            const float Rvel[9], const float Rback[9], float max_radius, int* idx_out) {
  HIPCHK(hipSetDevice(c->device));
  if (!(query->gradient_norm > 0.0f)) return fail_msg("search_match: the query keyline needs a positive gradient_norm", -3);
  wait_enqueued(searched);
  HIPCHK(trk_wait_ready(c->s_trk, searched));
  int* out_dev = reinterpret_cast<int*>(c->fscratch) + 32;
  launch_search_match_one(c->s_trk, c->K, searched->d, *query, vel, Rvel, Rback, max_radius, out_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_f + 32, out_dev, sizeof(int), hipMemcpyDeviceToHost, c->s_trk));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  std::memcpy(idx_out, c->h_f + 32, sizeof(int));
  return 0;
}

int rebvio_hip_smooth_n(rebvio_hip_ctx* c, const float* img, const int* widths, int n, float* out) {
  HIPCHK(hipSetDevice(c->device));
  if (n < 1 || n > 16) return fail_msg("smooth: 1..16 box passes", -3);
  for (int k = 0; k < n; ++k)
    if (widths[k] < 3 || widths[k] > 11 || (widths[k] & 1) == 0) return fail_msg("smooth: box widths must be odd and in 3..11", -3);
  const size_t nb = (size_t)c->P.rows * c->P.cols * sizeof(float);
  if (!c->diag0) {
    HIPCHK(c->own.device_bytes(&c->diag0, nb));
    HIPCHK(c->own.device_bytes(&c->diag1, nb));
  }
  HIPCHK(hipStreamSynchronize(c->s_key));  // the scratch DoG / gradient buffers below belong to frames in flight
  HIPCHK(hipMemcpyAsync(c->img_dev, img, nb, hipMemcpyHostToDevice, c->s_det));
  ScaleBufs sb = c->sb;
  sb.scale0 = c->diag0;
  sb.scale1 = c->diag1;
  launch_smooth_n(c->s_det, c->K, c->img_dev, sb, widths, n, c->db.rowcount);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->diag0, nb, hipMemcpyDeviceToHost, c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_det));
  return 0;
}

int rebvio_hip_smooth(rebvio_hip_ctx* c, const float* img, const int widths3[3], float* out) { return rebvio_hip_smooth_n(c, img, widths3, 3, out); }

int rebvio_hip_rotate(rebvio_hip_ctx* c, rebvio_hip_map* m, const float R[9]) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(trk_wait_ready(c->s_trk, m));
  launch_rotate(c->s_trk, c->K, m->d, R, nullptr, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

int rebvio_hip_quantile(rebvio_hip_ctx* c, rebvio_hip_map* m, float percentile, int num_bins, float* out) {
  HIPCHK(hipSetDevice(c->device));
  if (num_bins < 1 || num_bins > 128) return fail_msg("num_bins must be in 1..128", -3);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  launch_quantile(c->s_trk, c->K, m->d, c->hist, percentile, num_bins, c->fscratch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_f, c->fscratch, sizeof(float), hipMemcpyDeviceToHost, c->s_trk));
  HIPCHK(hipMemsetAsync(c->hist, 0, 128 * sizeof(int), c->s_trk));  // invariant: the histogram is zero between uses
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  *out = c->h_f[0];
  return 0;
}

int rebvio_hip_try_vel(rebvio_hip_ctx* c, rebvio_hip_map* m, const float vel[3], float sigma_rho_min, float* residuals,
                       float out10[10]) {
  HIPCHK(hipSetDevice(c->device));
  if (!c->df_map) return fail_msg("try_vel needs a distance field", -7);
  int rc = ensure_size(m);
  if (rc) return rc;
  const int n = m->n_host;
  HIPCHK(trk_wait_ready(c->s_trk, m));
  if (n > 0) HIPCHK(hipMemcpyAsync(m->d.residual, residuals, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->s_trk));
  LmState st;
  std::memset(&st, 0, sizeof(st));
  for (int i = 0; i < 3; ++i) st.Vnew[i] = st.vel[i] = vel[i];
  st.sigma_rho_min = sigma_rho_min;
  c->h_lm[1] = st;
  HIPCHK(hipMemcpyAsync(c->lm, &c->h_lm[1], sizeof(LmState), hipMemcpyHostToDevice, c->s_trk));
  launch_try_vel(c->s_trk, c->K, m->d, c->df_map->d, 0, 0, 0, c->lm, c->lm + 1, c->part, c->part, c->hist, 0);
  HIPCHK(hipGetLastError());
  const int nb = std::max(1, div_up(n, 256));
  HIPCHK(hipMemcpyAsync(c->h_part, c->part, (size_t)nb * kPartStride * sizeof(float), hipMemcpyDeviceToHost, c->s_trk));
  if (n > 0) HIPCHK(hipMemcpyAsync(residuals, m->d.residual, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->s_trk));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  for (int k = 0; k < 10; ++k) {
    // the order of the device-side reducer (track.hip reduce_staged_records): record b goes to lane b % 16, a lane adds its
    // records in ascending order from 0, the sixteen lanes are scanned with shifts 1, 2, 4, 8 (zero fill) - the sums a
    // stand-alone tryVel reports are bit for bit the ones minimizeVel's kernels work with
    float part[16];
    const int nblk = div_up(n, 256);
    for (int j = 0; j < 16; ++j) {
      float acc = 0.f;
      for (int b = j; b < nblk; b += 16) acc += c->h_part[(size_t)b * kPartStride + k];
      part[j] = acc;
    }
    for (int d = 1; d < 16; d <<= 1)
      for (int i = 15; i >= 0; --i) part[i] = part[i] + (i >= d ? part[i - d] : 0.0f);
    out10[k] = part[15];
  }
  // resolve cross-workgroup carry markers (a later device call would do this in its prologue)
  float carry = 0.f;
  for (int b = 0; b < div_up(n, 256); ++b) {
    const int lo = b * 256, hi = std::min(n, lo + 256);
    for (int i = lo; i < hi; ++i)
      if (residuals[i] == kResidualCarry) residuals[i] = std::fabs(carry);
    if (c->h_part[(size_t)b * kPartStride + 10] != 0.f) carry = c->h_part[(size_t)b * kPartStride + 11];
  }
  return 0;
}

int rebvio_hip_minimize_vel(rebvio_hip_ctx* c, rebvio_hip_map* m, float vel[3], float Rvel[9], float* F, int* accept_mask,
                            float* sigma_rho_min) {
  HIPCHK(hipSetDevice(c->device));
  if (!c->df_map) return fail_msg("minimize_vel needs a distance field", -7);
  HIPCHK(trk_wait_ready(c->s_trk, m));
  HIPCHK(hipMemsetAsync(m->d.residual, 0, (size_t)c->P.keylines_max * sizeof(float), c->s_trk));
  HIPCHK(hipMemsetAsync(c->hist, 0, 128 * sizeof(int), c->s_trk));
  // histogram of sigma_rho for estimateQuantile (core.cpp:153)
  launch_quantile(c->s_trk, c->K, m->d, c->hist, c->P.quantile_cutoff, c->P.quantile_num_bins, c->fscratch);
  enqueue_lm_chain(c, m, c->df_map, vel);
  const int calls = (int)c->P.iterations + 1;
  launch_lm_final(c->s_trk, m->d, calls, c->lm + calls, c->lm + calls + 1,
                  c->part + (size_t)(calls - 1) * part_call_stride(c));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&c->h_lm[0], c->lm + calls + 1, sizeof(LmState), hipMemcpyDeviceToHost, c->s_trk));
  HIPCHK(hipMemsetAsync(c->hist, 0, 128 * sizeof(int), c->s_trk));  // invariant: the histogram is zero between uses
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  lm_to_out(c->h_lm[0], vel, Rvel, F, accept_mask, sigma_rho_min);
  return 0;
}

int rebvio_hip_forward_match(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(trk_wait_ready(c->s_trk, om));
  HIPCHK(trk_wait_ready(c->s_trk, nm));
  // the winners follow from match_id_forward as it stands now (edge_map.cpp:78-81): keys that an earlier minimize_vel or
  // forward_match into this map has left are not part of it (covers [0, n): n <= keylines_max)
  HIPCHK(hipMemsetAsync(nm->d.fwd_key, 0, (size_t)c->P.keylines_max * sizeof(unsigned long long), c->s_trk));
  launch_forward_keys(c->s_trk, c->K, om->d, nm->d);
  const float v0[3] = {0, 0, 0};
  launch_ext_rot_vel(c->s_trk, c->K, om->d, nm->d, 1, 0, 0, c->lm, c->lm, c->part, c->xrv_part, v0, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

int rebvio_hip_ext_rot_vel(rebvio_hip_ctx* c, const float vel[3], float Wx[36], float JtF[6], float X[6], int* ok) {
  HIPCHK(hipSetDevice(c->device));
  if (!c->df_map) return fail_msg("ext_rot_vel needs a distance field", -7);
  rebvio_hip_map* nm = c->df_map;
  int rc = ensure_size(nm);
  if (rc) return rc;
  launch_ext_rot_vel(c->s_trk, c->K, nm->d, nm->d, 0, 0, 0, c->lm, c->lm, c->part, c->xrv_part, vel, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  const int nb = std::max(1, div_up(nm->n_host, 256));
  HIPCHK(hipMemcpyAsync(c->h_xrv, c->xrv_part, (size_t)nb * kXrvStride * sizeof(float), hipMemcpyDeviceToHost, c->s_trk));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  float jtf[6];
  sum_xrv(c->h_xrv, div_up(nm->n_host, 256), Wx, jtf, nullptr);
  if (JtF) std::memcpy(JtF, jtf, sizeof(jtf));
  hm::sym6_pinv_solve(Wx, jtf, X);
  int good = 1;
  for (int i = 0; i < 6; ++i)
    if (std::isnan(X[i])) good = 0;
  if (ok) *ok = good;
  return 0;
}

int rebvio_hip_directed_match(rebvio_hip_ctx* c, rebvio_hip_map* nm, rebvio_hip_map* om, const float vel[3],
                              const float Rvel[9], const float Rback[9], float max_radius, int* matches, int* kf_matches) {
  HIPCHK(hipSetDevice(c->device));
  // (a probe's slot index 2 * step + side takes 10 bits of a candidate-list entry of k_directed_match_c; rebvio_hip_create bounds
  // search_range the same way)
  if (!(max_radius >= 0.f) || max_radius > 255.f) return fail_msg("directed_match: max_radius outside 0..255", -3);
  // (a long search walks up to max_radius + 2 * pixel_uncertainty_match steps: the bound of rebvio_hip_create on search_range)
  if (max_radius + 2.0f * c->P.pixel_uncertainty_match + 2.0f > 260.0f)
    return fail_msg("directed_match: max_radius + 2 * pixel_uncertainty_match must be at most 258 (probe sequence buffer)", -3);
  HIPCHK(trk_wait_ready(c->s_trk, om));
  HIPCHK(trk_wait_ready(c->s_trk, nm));
  float vel_r[3], Rvel_r[9];
  rotate_inputs(c, vel, Rvel, Rback, vel_r, Rvel_r);
  HIPCHK(hipMemsetAsync(&nm->d.st->dm_matches, 0, 4 * sizeof(int), c->s_trk));  // dm_matches, dm_kf, reg_count, dm_queued
  launch_directed_match(c->s_trk, c->K, nm->d, om->d, vel_r, Rvel_r, Rback, max_radius, nullptr, c->dm_head_form);
  HIPCHK(hipGetLastError());
  MapState st;
  int rc = fetch_map_state(nm, &st, c->s_trk);
  if (rc) return rc;
  if (matches) *matches = st.dm_matches;
  if (kf_matches) *kf_matches = st.dm_kf;
  return 0;
}

int rebvio_hip_regularize(rebvio_hip_ctx* c, rebvio_hip_map* m, int* count) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(trk_wait_ready(c->s_trk, m));
  HIPCHK(hipMemsetAsync(&m->d.st->reg_count, 0, sizeof(int), c->s_trk));
  launch_regularize(c->s_trk, c->K, m->d, 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(m->d.rs, m->d.rs_tmp, (size_t)c->P.keylines_max * sizeof(float2), hipMemcpyDeviceToDevice, c->s_trk));
  MapState st;
  int rc = fetch_map_state(m, &st, c->s_trk);
  if (rc) return rc;
  if (count) *count = st.reg_count;
  return 0;
}

int rebvio_hip_update_inverse_depth(rebvio_hip_ctx* c, const float vel[3]) {
  HIPCHK(hipSetDevice(c->device));
  if (!c->df_map) return fail_msg("update_inverse_depth needs a distance field", -7);
  launch_depth_ekf(c->s_trk, c->K, c->df_map->d, vel, 0, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

namespace {
// Host glue between extRotVel and directedMatch (rebvio.cpp:177-233, accelerometer/SAB branch excluded) for the per-pair
// API: the shared core of glue.hpp (the streaming and batch drivers run the same statements on the device). R is the prior
// rotation used for the first rotateKeylines.
struct GlueOut {
  float R0a[9], Rgva[9], V[3], P_V[9];
  bool nan_v;
};
GlueParams glue_params(const rebvio_hip_ctx* c, float frame_dt) {
  GlueParams gp;
  gp.frame_dt = frame_dt;
  gp.gyro_std_dev = c->P.gyro_std_dev;
  gp.gyro_bias_std_dev = c->P.gyro_bias_std_dev;
  gp.has_pre = 0;
  std::memset(gp.pre, 0, sizeof(gp.pre));
  gp.has_next = 1;  // no gyro rotation known for the next pair: the identity (glue_params_next)
  hm::store3(hm::identity3(), gp.R_next);
  return gp;
}
// Streaming and batch drivers: what the glue of a pair needs of the pair AFTER it - the gyro rotation `next` was pushed with (the
// frame behind the pair's new map). next == null: not pushed yet. A stream without rotations goes on with the identity; on one
// that carries rotations the pair runs without the next rotation (GlueParams::has_next). Returns has_next.
bool glue_params_next(const rebvio_hip_ctx* c, const rebvio_hip_map* next, GlueParams* gp) {
  gp->has_next = (next || !c->gyro_stream) ? 1 : 0;
  if (next && next->gyro_set) std::memcpy(gp->R_next, next->gyro_R, sizeof(gp->R_next));
  return gp->has_next != 0;
}
// Streaming driver: the pair's gyroBiasCorrection matrices from the host's shadow of the device's W_Bg (GlueParams::pre); the
// shadow advances with every pair queued. Not valid (after rebvio_hip_set_gyro_state, before the first pair of a stream has
// uploaded the host's state): the device forms them itself.
void glue_params_pre(rebvio_hip_ctx* c, GlueParams* gp) {
  if (!c->gyro_pre_on || !c->wbg_shadow_valid) return;
  const float s_b = gp->gyro_bias_std_dev * gp->gyro_bias_std_dev * gp->frame_dt * gp->frame_dt;  // (rebvio.cpp:186-191, as the glue forms them)
  const float s_g = gp->gyro_std_dev * gp->gyro_std_dev * gp->frame_dt * gp->frame_dt;
  hm::gyro_pre(c->wbg_shadow, s_g, s_b, gp->pre);
  gp->has_pre = 1;
  c->wbg_shadow = hm::load3(gp->pre[2]);
}
GlueOut pair_glue(rebvio_hip_ctx* c, const LmState& lm, const float* xrv, int n_new, float frame_dt, hm::M3 R,
                  rebvio_hip_pair_out* out) {
  GlueState st;
  for (int i = 0; i < 3; ++i) st.Bg[i] = c->Bg[i];
  hm::store3(c->W_Bg, st.W_Bg);
  hm::store3(R, st.R);
  st.pad = 0.f;
  GlueDev gl;
  hm::pair_glue_core(lm, xrv, n_new, glue_params(c, frame_dt), st, gl, *out);
  for (int i = 0; i < 3; ++i) c->Bg[i] = st.Bg[i];
  c->W_Bg = hm::load3(st.W_Bg);
  note_accept_mask(c, out->lm_accept_mask);
  GlueOut g;
  std::memcpy(g.R0a, gl.R0a, sizeof(g.R0a));
  std::memcpy(g.Rgva, gl.Rgva, sizeof(g.Rgva));
  std::memcpy(g.V, gl.V, sizeof(g.V));
  std::memcpy(g.P_V, out->P_V, sizeof(g.P_V));
  g.nan_v = gl.nan_v != 0;
  return g;
}

// rotate by R0, directedMatch, regularize1Iter, updateInverseDepth (rebvio.cpp:232-259) on the track stream:
// three launches - the rotation of the old map is applied on the fly inside directedMatch (the old map is dead
// afterwards), regularize + depth EKF are one kernel. RT_next (streaming driver only) additionally applies the next
// pair's first rotateKeylines to the new map and bins its sigma_rho histogram.
void enqueue_b_chain(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const GlueOut& g, const float* RT_next) {
  hipStream_t s = c->s_trk;
  if (g.nan_v) {  // rebvio.cpp:236: no matching / depth update
    if (RT_next) {
      launch_rotate(s, c->K, nm->d, RT_next, c->hist, 0);
      nm->pre_rotated = true;
    }
    return;
  }
  float vel_r[3], Rvel_r[9];
  rotate_inputs(c, g.V, g.P_V, g.Rgva, vel_r, Rvel_r);
  launch_directed_match(s, c->K, nm->d, om->d, vel_r, Rvel_r, g.Rgva, c->P.search_range, g.R0a, c->dm_head_form);
  const int gate = (int)c->P.global_min_matches_threshold;
  launch_regularize_ekf(s, c->K, nm->d, g.V, gate > 0 ? gate : 0, RT_next, c->hist);  // rebvio.cpp:256-259
  std::swap(nm->d.rs, nm->d.rs_tmp);
  if (RT_next) {
    std::swap(nm->d.grad, nm->d.grad_tmp);
    nm->pre_rotated = true;
  }
}

hm::M3 prior_rotation(rebvio_hip_ctx* c, const float* R_prior) {
  // R = imu.R(); R.T() = SO3(Bg) * R.T()  (rebvio.cpp:163-164)
  return hm::prior_rotation(c->Bg, R_prior ? hm::load3(R_prior) : hm::identity3());
}

// The match counters of a finished pair from its new map's state record; too few matches: status 2 (rebvio.cpp:247-252).
void match_counters(rebvio_hip_pair_out* o, const MapState& st, const rebvio_hip_params& P) {
  o->klm_num = st.dm_matches;
  o->kf_matches = st.dm_kf;
  o->reg_num = st.reg_count;
  if ((unsigned)o->klm_num < P.global_min_matches_threshold) o->status = 2;
}
}  // namespace

int rebvio_hip_track_pair(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const float* R_prior, float frame_dt,
                          rebvio_hip_pair_out* out) {
  HIPCHK(hipSetDevice(c->device));
  std::memset(out, 0, sizeof(*out));
  hipStream_t s = c->s_trk;
  om->served_old = true;
  HIPCHK(trk_wait_ready(s, om));
  HIPCHK(trk_wait_ready(s, nm));
  int rc = rebvio_hip_build_distance_field(c, nm);  // rebvio.cpp:142 (no-op when detect already built it)
  if (rc) return rc;
  const hm::M3 R = prior_rotation(c, R_prior);
  float RT[9];
  hm::store3(hm::transpose(R), RT);
  launch_rotate(s, c->K, om->d, RT, c->hist, 0);  // rebvio.cpp:165 (+ histogram for estimateQuantile; hist is zero here)
  const float v0[3] = {0, 0, 0};                  // imu_state_.Vg = Zeros (rebvio.cpp:167)
  // minimizeVel, forwardMatch + extRotVel (rebvio.cpp:169-177); results land in slot 0
  PairSlot* slot = c->slot[0];
  rc = enqueue_pair_lm(c, om, nm, v0, slot, slot->xrv, GlueArgs{});
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  if (slot->seq != c->last_stamp) return fail_msg(kStaleRecordMsg, kStaleRecord);
  nm->n_host = slot->new_st.n;
  nm->thr_host = slot->new_st.threshold;
  const GlueOut g = pair_glue(c, slot->lm, slot->xrv, nm->n_host, frame_dt, R, out);
  enqueue_b_chain(c, om, nm, g, nullptr);
  HIPCHK(hipGetLastError());
  if (g.nan_v) {
    out->status = 1;
    return 0;
  }
  HIPCHK(hipMemcpyAsync(&c->h_st[1], nm->d.st, sizeof(MapState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  match_counters(out, c->h_st[1], c->P);
  return 0;
}

int rebvio_hip_track_pair_begin(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const float* R_prior, float frame_dt,
                                rebvio_hip_pair_mid* mid) {
  HIPCHK(hipSetDevice(c->device));
  const auto tb0 = std::chrono::steady_clock::now();
  std::memset(mid, 0, sizeof(*mid));
  hipStream_t s = c->s_trk;
  if (!c->h_bf) {
    HIPCHK(c->own.pinned(&c->h_bf, 2, false));
    for (auto& e : c->bf_done) HIPCHK(c->own.event(&e));
  }
  c->bf_cur = (c->bf_res == 0) ? 1 : 0;  // the slot that does not hold an unfetched result
  // The previous pair's match counters (unfetched: result slot bf_res). If this pair continues from its new map they arrive
  // for free with this pair's slot (the first-half kernel copies its old map's state record into pinned memory); otherwise a
  // copy is queued here, AHEAD of this pair (and of its parked second half).
  const int pr = c->bf_res;
  const bool prev_from_slot = pr >= 0 && !c->bf_have[pr] && !c->bf_copy_queued[pr] && c->bf_map[pr] == om;
  if (pr >= 0 && !c->bf_have[pr] && !c->bf_copy_queued[pr] && !prev_from_slot) {
    HIPCHK(hipMemcpyAsync(&c->h_bf[pr], c->bf_map[pr]->d.st, sizeof(MapState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(c->bf_done[pr], s));
    c->bf_copy_queued[pr] = true;
  }
  om->served_old = true;
  wait_enqueued(om);
  wait_enqueued(nm);
  HIPCHK(trk_wait_ready_once(c, om));
  HIPCHK(trk_wait_ready_once(c, nm));
  int rc = rebvio_hip_build_distance_field(c, nm);
  if (rc) return rc;
  const hm::M3 R = prior_rotation(c, R_prior);
  if (om->pre_rotated) {
    // the previous pair's _finish_async applied this pair's first rotateKeylines (and binned the sigma histogram) inside its
    // last kernel; it was told the same prior
    if (std::memcmp(&om->pre_R, &R, sizeof(R)) != 0)
      return fail_msg("track_pair_begin: R_prior (or the gyro state) differs from the R_prior_next the previous finish_async applied", -7);
    om->promised.store(false, std::memory_order_release);  // consumed: the map is in the frame this pair asked for
  } else {
    float RT[9];
    hm::store3(hm::transpose(R), RT);
    launch_rotate(s, c->K, om->d, RT, c->hist, 0);
  }
  const float v0[3] = {0, 0, 0};
  PairSlot* slot = c->slot[0];
  rc = enqueue_pair_lm(c, om, nm, v0, slot, slot->xrv, GlueArgs{});
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  const auto tb1 = std::chrono::steady_clock::now();
  // No event behind the first half: a completion event is a packet of its own on the track stream (~5 us until its signal fires
  // on this runtime, plus the wake-up) between the LM kernel's end and this thread - the path the inertial fusion and the second
  // half's launch wait on. The records carry sequence stamps (slot: the LM kernel's last store; every extRotVel block record:
  // stored behind the record's own words), so the thread polls them in pinned memory instead.
  {
    const int prc = poll_pair_records(c, slot, c->last_stamp);
    if (prc) return prc;
  }
  const auto tb2 = std::chrono::steady_clock::now();
  c->t_begin_enq += std::chrono::duration<double, std::micro>(tb1 - tb0).count();
  c->t_begin_wait += std::chrono::duration<double, std::micro>(tb2 - tb1).count();
  c->t_begin_n++;
  if (slot->seq != c->last_stamp) return fail_msg(kStaleRecordMsg, kStaleRecord);
  if (prev_from_slot) {
    c->h_bf[pr] = slot->old_st;
    c->bf_have[pr] = true;
  }
  nm->n_host = slot->new_st.n;
  nm->thr_host = slot->new_st.threshold;
  lm_to_out(slot->lm, mid->Vg, mid->P_Vg, &mid->F, &mid->lm_accept_mask, &mid->sigma_rho_min);
  note_accept_mask(c, mid->lm_accept_mask);
  float JtF6[6];
  sum_xrv(slot->xrv, div_up(nm->n_host, 256), mid->W_Xv, JtF6, nullptr);
  hm::sym6_solve(mid->W_Xv, JtF6, mid->Xv);
  mid->ext_ok = 1;
  for (int i = 0; i < 6; ++i)
    if (std::isnan(mid->Xv[i])) mid->ext_ok = 0;
  std::memcpy(mid->Xgv, mid->Xv, sizeof(mid->Xv));
  std::memcpy(mid->W_Xgv, mid->W_Xv, sizeof(mid->W_Xv));
  const float s_b = c->P.gyro_bias_std_dev * c->P.gyro_bias_std_dev * frame_dt * frame_dt;
  const float s_g = c->P.gyro_std_dev * c->P.gyro_std_dev * frame_dt * frame_dt;
  c->RGBias = hm::diag3(s_b);
  c->RGyro = hm::diag3(s_g);
  float dg[3];
  hm::gyro_bias_correction(mid->Xgv, mid->W_Xgv, c->W_Bg, c->RGyro, c->RGBias, dg);
  for (int i = 0; i < 3; ++i) c->Bg[i] += dg[i];
  hm::store3(R, mid->R);
  return 0;
}

int rebvio_hip_track_pair_finish_async(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const float V[3], const float P_V[9],
                                       const float Rgva[9], const float R_second[9], const float* R_prior_next) {
  HIPCHK(hipSetDevice(c->device));
  GlueOut g;
  std::memcpy(g.V, V, sizeof(g.V));
  std::memcpy(g.P_V, P_V, sizeof(g.P_V));
  std::memcpy(g.Rgva, Rgva, sizeof(g.Rgva));
  std::memcpy(g.R0a, R_second, sizeof(g.R0a));
  g.nan_v = std::isnan(V[0]) || std::isnan(V[1]) || std::isnan(V[2]);
  if (!c->h_bf) return fail_msg("track_pair_finish without track_pair_begin", -7);
  if (c->bf_res >= 0) return fail_msg("track_pair_finish_async: fetch the previous pair's result first (rebvio_hip_track_pair_result)", -7);
  c->bf_nan[c->bf_cur] = g.nan_v;
  c->bf_res = c->bf_cur;
  c->bf_map[c->bf_cur] = nm;  // its state record will hold the counters: fetched by the next _begin or by _result
  c->bf_have[c->bf_cur] = false;
  c->bf_copy_queued[c->bf_cur] = false;
  float RT_next[9];
  if (R_prior_next) {  // the next pair's first rotateKeylines rides in this pair's last kernel (rebvio.cpp:163-165 of that pair)
    nm->pre_R = prior_rotation(c, R_prior_next);
    hm::store3(hm::transpose(nm->pre_R), RT_next);
    nm->promised.store(true, std::memory_order_release);
  }
  enqueue_b_chain(c, om, nm, g, R_prior_next ? RT_next : nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

int rebvio_hip_track_pair_hint_next(rebvio_hip_ctx* c, rebvio_hip_map* next_new_map) {
  if (!c || !next_new_map || next_new_map->ctx != c) return fail_msg("track_pair_hint_next: map of another context", -3);
  HIPCHK(hipSetDevice(c->device));
  wait_enqueued(next_new_map);
  HIPCHK(trk_wait_ready_once(c, next_new_map));
  return 0;
}

int rebvio_hip_track_pair_result(rebvio_hip_ctx* c, int* klm_num, int* kf_matches, int* reg_num, int* status) {
  HIPCHK(hipSetDevice(c->device));
  if (klm_num) *klm_num = 0;
  if (kf_matches) *kf_matches = 0;
  if (reg_num) *reg_num = 0;
  if (c->bf_res < 0) return fail_msg("track_pair_result: no finished pair to report", -7);
  const int r = c->bf_res;
  c->bf_res = -1;
  if (!c->bf_have[r]) {
    if (!c->bf_copy_queued[r]) {  // no later pair has been begun: fetch the record now (nothing is parked at this point)
      HIPCHK(hipMemcpyAsync(&c->h_bf[r], c->bf_map[r]->d.st, sizeof(MapState), hipMemcpyDeviceToHost, c->s_trk));
      HIPCHK(hipEventRecord(c->bf_done[r], c->s_trk));
    }
    HIPCHK(hipEventSynchronize(c->bf_done[r]));  // (a copy queued by _begin sits ahead of that pair's parked second half)
    c->bf_have[r] = true;
  }
  rebvio_hip_pair_out o{};
  if (c->bf_nan[r])
    o.status = 1;
  else
    match_counters(&o, c->h_bf[r], c->P);
  if (klm_num) *klm_num = o.klm_num;
  if (kf_matches) *kf_matches = o.kf_matches;
  if (reg_num) *reg_num = o.reg_num;
  if (status) *status = o.status;
  return 0;
}

int rebvio_hip_track_pair_finish(rebvio_hip_ctx* c, rebvio_hip_map* om, rebvio_hip_map* nm, const float V[3], const float P_V[9],
                                 const float Rgva[9], const float R_second[9], int* klm_num, int* kf_matches, int* reg_num,
                                 int* status) {
  const int rc = rebvio_hip_track_pair_finish_async(c, om, nm, V, P_V, Rgva, R_second, nullptr);
  if (rc) return rc;
  return rebvio_hip_track_pair_result(c, klm_num, kf_matches, reg_num, status);
}

namespace {
// ---- streaming driver -------------------------------------------------------------------------------------------------
// Per pair, on the track stream, four launches and nothing else (one event per GROUP of pairs, see stream_enqueue_group):
//   persistent minimizeVel / forwardMatch / extRotVel, with the pair's GLUE at its tail: every workgroup publishes its
//             extRotVel sums as tagged words, workgroup 0 collects them and evaluates glue.hpp (6x6 solve, gyroBiasCorrection,
//             SO3, Cholesky) on four waves (glue_dev.hpp); filter state in device memory (double-buffered by pair parity),
//             the second half's inputs in glue_dev[slot], the host's record in a pinned GlueRec
//   directedMatch head (reads glue_dev[slot]) -> directedMatch tail -> regularize / depth EKF / next pair's first rotation
// The host never stands between a pair's halves (round 2: kernel end -> event -> host glue -> flag -> wait kernel, 8-10 us
// of an ~80 us frame, and the reason the rate moved with the box's host): it queues pair k as soon as frame k + lead - 2 has
// been queued for detection and reads the pairs' records up to kSlots - 1 pairs later. A pair's match counters are
// read from the NEXT pair's slot (its first kernel copies its old map's state record), so pair k is reported once pair
// k + 1's event has fired; rebvio_hip_flush() fetches the last pair's counters itself.

// The lanes whose pairs a PairQueue holds: the streaming driver's context alone, or a batch's lanes. owner / who: the time-out
// error's residency report (the context or the batch) and its prefix.
struct LaneSet {
  rebvio_hip_ctx* const* c;
  int n;
  int device;
  const void* owner;
  const char* who;
};

// A step's records as the caller gets them, lane by lane: the device glue's output, the match counters from each lane's new map
// state record st[l], and the lane's host mirror of the filter state (rebvio_hip_get_gyro_state; authoritative again after a flush).
int finish_step(PairQueue& q, const LaneSet& L, const PairQueue::Step& a, const MapState* st) {
  for (int l = 0; l < L.n; ++l) {
    const GlueRec* r = L.c[l]->rec[a.slot];
    if (r->seq_out != a.seq || r->seq_gs != a.seq) return fail_msg(kStaleRecordMsg, kStaleRecord);
  }
  for (int l = 0; l < L.n; ++l) {
    rebvio_hip_ctx* c = L.c[l];
    const GlueRec* r = c->rec[a.slot];
    PairRec d;
    d.out = r->out;
    if (d.out.status != 1) match_counters(&d.out, st[l], c->P);
    d.keylines = st[l].n;
    for (int i = 0; i < 3; ++i) c->Bg[i] = r->gs.Bg[i];
    c->W_Bg = hm::load3(r->gs.W_Bg);
    c->gs_R = hm::load3(r->gs.R);
    note_accept_mask(c, d.out.lm_accept_mask);
    c->t_queued += (double)st[l].dm_queued;
    q.done.push_back(d);
  }
  return 0;
}

// Has step n, queued without an event, left its result slots? 1: every lane's slot carries n's stamp and adds up; 0: not yet
// (block == false). The stamp is stored by the last wave of n's directedMatch launch, which started only after the kernels of
// the step in front of n had ended: it proves that step complete, records and maps. block: polls the slots; the track stream is
// queried every few thousand polls, and once it is idle - n's kernels have run, nothing can arrive any more - the slots get one
// last look: the records, or -12 (a forged or lost stamp). The wait is bounded by the stream's own work, not by a time-out.
int step_stamped(PairQueue& q, const LaneSet& L, const PairQueue::Step& n, bool block) {
  auto all_lanes = [&]() -> bool {
    for (int l = 0; l < L.n; ++l)
      if (!slot_complete(L.c[l]->slot[n.slot], n.seq)) return false;
    return true;
  };
  if (!all_lanes()) {
    if (!block) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
      __builtin_ia32_pause();
      if (all_lanes()) break;
      if ((spins & 0xFFFu) != 0u) continue;
      const hipError_t e = hipStreamQuery(L.c[0]->s_trk);  // (the lanes of a batch share its track stream)
      if (e == hipErrorNotReady) continue;
      if (e != hipSuccess) return fail("track stream", e);
      if (all_lanes()) break;
      for (int l = 0; l < L.n; ++l) {
        const int rc = lm_timed_out(L.c[l], L.device, L.owner, L.who);
        if (rc) return rc;
      }
      return fail_msg(kStaleRecordMsg, kStaleRecord);
    }
    q.t_wait += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 1;
}

// Reports the steps whose successor has completed (a step's match counters ride in its successor's slots: the successor's first
// kernel copies its old maps' state records); `need` > 0: blocks until at least that many have been reported. The successor's
// completion is its group's event where it has one (batch driver, REBVIO_HIP_HANDOVER=events), else its record stamp (step_stamped).
int harvest(PairQueue& q, const LaneSet& L, int need) {
  MapState st[kMaxLanes];
  while (q.count >= 2) {
    const PairQueue::Step& a = q[0];
    const PairQueue::Step& n = q[1];
    if (n.ev_slot < 0) {
      const int w = step_stamped(q, L, n, need > 0);
      if (w < 0) return w;
      if (w == 0) break;
    } else if (need > 0) {
      const auto t0 = std::chrono::steady_clock::now();
      HIPCHK(hipEventSynchronize(q.slot_ev[n.ev_slot]));
      q.t_wait += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    } else {
      const hipError_t e = hipEventQuery(q.slot_ev[n.ev_slot]);
      if (e == hipErrorNotReady) break;
      HIPCHK(e);
    }
    for (int l = 0; l < L.n; ++l) {
      const rebvio_hip_ctx* c = L.c[l];
      const int rc = lm_timed_out(c, L.device, L.owner, L.who);
      if (rc) return rc;
      if (c->slot[n.slot]->seq != n.seq) return fail_msg(kStaleRecordMsg, kStaleRecord);
      st[l] = c->slot[n.slot]->old_st;
    }
    const int frc = finish_step(q, L, a, st);
    if (frc) return frc;
    q.pop_front();
    --need;
  }
  return 0;
}

// Everything queued completes; every step's records end in q.done. The last step has no successor to carry its counters: they
// are copied from its new maps.
int drain(PairQueue& q, const LaneSet& L) {
  int rc = harvest(q, L, q.count);
  if (rc) return rc;
  if (q.count == 1) {
    const PairQueue::Step& a = q[0];
    if (a.ev_slot >= 0)
      HIPCHK(hipEventSynchronize(q.slot_ev[a.ev_slot]));
    else
      HIPCHK(hipStreamSynchronize(L.c[0]->s_trk));
    for (int l = 0; l < L.n; ++l) {
      rebvio_hip_ctx* c = L.c[l];
      rc = lm_timed_out(c, L.device, L.owner, L.who);
      if (rc) return rc;
      if (c->slot[a.slot]->seq != a.seq) return fail_msg(kStaleRecordMsg, kStaleRecord);
      HIPCHK(hipMemcpyAsync(&c->h_st[1], a.nm[l]->d.st, sizeof(MapState), hipMemcpyDeviceToHost, c->s_trk));
    }
    HIPCHK(hipStreamSynchronize(L.c[0]->s_trk));  // (the lanes of a batch share its track stream)
    MapState st[kMaxLanes];
    for (int l = 0; l < L.n; ++l) st[l] = L.c[l]->h_st[1];
    rc = finish_step(q, L, a, st);
    if (rc) return rc;
    q.pop_front();
  }
  return 0;
}

// The oldest step's records, one per lane, to the caller; 0: none is waiting.
int pop_records(PairQueue& q, int lanes, rebvio_hip_pair_out* out, int* keylines) {
  if (q.done.empty()) return 0;
  for (int l = 0; l < lanes; ++l) {
    if (out) out[l] = q.done.front().out;
    if (keylines) keylines[l] = q.done.front().keylines;
    q.done.pop_front();
  }
  return 1;
}

// Pairs (batch: steps) to queue as one group now, with `queued` detected frames (steps) waiting and `inflight` steps queued. Full
// groups while the device has pairs queued (fewest stream operations per pair); as soon as it is about to run dry - a stream's
// start, or right after the caller synchronised - whatever can start is started at once, down to single pairs. Either way the
// newest map of a group was detected at least lead - 2 calls ago.
int group_size(int queued, int inflight, int lead, int group) {
  const bool shallow = inflight < group;
  return shallow ? std::min(group, queued - lead + 1) : (queued >= lead + group - 1 ? group : 0);
}

// First pair of a lane's stream (or after a flush): no second half has applied the prior rotation yet, and the filter state the
// device glue works on is the host's. It goes up into the state of pair parity gpar; then the old map's first rotateKeylines,
// for the gyro rotation the pair's newer frame nm was pushed with (rebvio.cpp:163-165).
int start_lane_stream(rebvio_hip_ctx* c, rebvio_hip_map* om, const rebvio_hip_map* nm, int gpar) {
  const hm::M3 R = prior_rotation(c, nm->gyro_set ? nm->gyro_R : nullptr);
  GlueState& gs = c->h_gstate[gpar];
  for (int i = 0; i < 3; ++i) gs.Bg[i] = c->Bg[i];
  hm::store3(c->W_Bg, gs.W_Bg);
  hm::store3(R, gs.R);
  gs.pad = 0.f;
  HIPCHK(hipMemcpyAsync(c->gstate + gpar, &gs, sizeof(GlueState), hipMemcpyHostToDevice, c->s_trk));
  float RT[9];
  hm::store3(hm::transpose(R), RT);
  launch_rotate(c->s_trk, c->K, om->d, RT, c->hist, 0);
  return 0;
}

// The streaming driver as one lane (the set points at the caller's own `c`: use it within that call)
LaneSet stream_lanes(rebvio_hip_ctx* const& c) { return LaneSet{&c, 1, c->device, c, ""}; }


// `npairs` consecutive pairs (frames[0..npairs]) as ONE group on the track stream. Every stream operation between two
// kernels is a packet of its own for the command processor, and with the kernels queued back to back those packets are what
// is left between them (measured with in-kernel stamps: ~6 us per event record / event wait on the pair-to-pair path). A group
// carries one of them whatever its size: the wait for the detection of its NEWEST map (the keyline stream is in order, so the
// maps before it are ready too; the runtime drops the wait where that detection has finished). With REBVIO_HIP_HANDOVER=events
// a second one: an event behind its last kernel, which stands for every pair's completion and for the release of every old map.
// Without it nothing is recorded: harvest learns a pair's completion from its successor's record stamp, and the old maps go back
// to the pool with the number of pairs the host has to have read by then.
int stream_enqueue_group(rebvio_hip_ctx* c, int npairs) {
  // the slot of pair k is reused by pair k + kSlots: its record (and its successor's) must have been read
  while (c->q.count + npairs > rebvio_hip_ctx::kSlots - 1) {
    const int rc = harvest(c->q, stream_lanes(c), 1);
    if (rc) return rc;
  }
  hipStream_t s = c->s_trk;
  if (!c->frames[0]->trk_waited) {  // first group of a stream
    wait_enqueued(c->frames[0]);
    c->ho.queued[kOnTrk].fetch_add(1, std::memory_order_relaxed);
    HIPCHK(trk_wait_ready(s, c->frames[0]));
    c->frames[0]->trk_waited = true;
  }
  {
    rebvio_hip_map* newest = c->frames[(size_t)npairs];
    wait_enqueued(newest);
    c->ho.queued[kOnTrk].fetch_add(1, std::memory_order_relaxed);
    HIPCHK(trk_wait_ready(s, newest));
    for (int g = 1; g <= npairs; ++g) {
      c->frames[(size_t)g]->trk_waited = true;
      if (g < npairs) {  // (as trk_wait_ready does for the map it is given)
        std::lock_guard<std::mutex> dl(c->dl_mu);
        c->frames[(size_t)g]->trk_touched.store(true, std::memory_order_release);
      }
    }
  }
  int last_slot = -1;
  for (int g = 0; g < npairs; ++g) {
    rebvio_hip_map *om = c->frames[(size_t)g], *nm = c->frames[(size_t)g + 1];
    c->df_map = nm;
    const int slot = (int)(c->pair_seq % rebvio_hip_ctx::kSlots);
    const int gpar = (int)(c->pair_seq & 1);
    if (om->kf_flag) {  // rebvio_hip_keyframe_next: behind the pair that ended at om (stream order), in front of this one
      launch_mark_keyframe(s, c->K, om->d);
      om->kf_flag = false;
    }
    if (!om->pre_rotated) {
      const int rc = start_lane_stream(c, om, nm, gpar);
      if (rc) return rc;
      c->wbg_shadow = c->W_Bg;  // what the device's filter state starts from
      c->wbg_shadow_valid = true;
    }
    const float v0[3] = {0, 0, 0};
    const float frame_dt = (float)((double)(float)(nm->ts - om->ts) / 1000000.0);  // rebvio.cpp:183
    const int calls = (int)c->P.iterations + 1;
    GlueArgs ga;
    ga.lm = c->lm + calls + 1;
    ga.xrv = c->xrv_part;
    ga.st_in = c->gstate + gpar;
    ga.st_out = c->gstate + (gpar ^ 1);
    ga.rec = c->rec[slot];
    ga.gd_copy = c->glue_dev + slot;
    ga.stage = c->glue_stage + slot;
    ga.gp = glue_params(c, frame_dt);
    glue_params_pre(c, &ga.gp);
    // the glue forms the NEXT pair's prior rotation: the rotation of the frame behind nm (queued already, but for a flush's last pair)
    const bool has_next = glue_params_next(c, (size_t)g + 2 < c->frames.size() ? c->frames[(size_t)g + 2] : nullptr, &ga.gp);
    int rc = enqueue_pair_lm(c, om, nm, v0, c->slot[slot], c->xrv_part, ga);  // rebvio.cpp:167-177 + the glue of rebvio.cpp:177-233
    if (rc) return rc;
    launch_directed_match_dev(s, c->K, nm->d, om->d, c->glue_dev + slot, c->glue_stage + slot, c->P.search_range, c->dm_head_form);
    const int gate = (int)c->P.global_min_matches_threshold;
    launch_regularize_ekf_dev(s, c->K, nm->d, c->glue_dev + slot, gate > 0 ? gate : 0, c->hist);  // rebvio.cpp:256-259
    std::swap(nm->d.rs, nm->d.rs_tmp);
    if (has_next) {  // (else the last kernel has left the new map in its own frame: the next pair starts through start_lane_stream)
      std::swap(nm->d.grad, nm->d.grad_tmp);
      nm->pre_rotated = true;
    }
    HIPCHK(hipGetLastError());
    PairQueue::Step f;
    f.nm[0] = nm;
    f.seq = c->last_stamp;
    f.slot = slot;
    c->q.push_back(f);
    last_slot = slot;
    c->pair_seq++;
  }
  if (c->handover_events) {
    HIPCHK(record_counted(c, kOnTrk, s, c->q.slot_ev[last_slot]));
    for (int g = 0; g < npairs; ++g) {
      c->q[c->q.count - 1 - g].ev_slot = last_slot;
      release_map(c->frames[(size_t)g], c->q.slot_ev[last_slot]);  // stream-ordered: reusable once the group has drained
    }
  } else {
    // No event: pair k's old map is idle once the host has read pair k's records (harvest: the stamp of pair k + 1), and whoever
    // reuses it earlier records an event then (detect_launch).
    for (int g = 0; g < npairs; ++g)
      release_map(c->frames[(size_t)g], nullptr, false, c->q[c->q.count - npairs + g].idx + 1);
  }
  c->frames.erase(c->frames.begin(), c->frames.begin() + npairs);
  return 0;
}

}  // namespace

namespace {
int push_frame(rebvio_hip_ctx* c, const uint8_t* frame_dev, const uint8_t* frame_host, size_t host_pitch, uint64_t ts_us, rebvio_hip_pair_out* out,
               int* keylines, int fmt = 0, const uint8_t* mask_frame = nullptr, const float* R_gyro = nullptr) {
  // Software pipeline over the three HIP streams of the context:
  //   scan / keyline streams : frame f (this call)
  //   track stream           : see the comment above stream_wait_maps
  // The returned record is the oldest COMPLETE pair not yet handed out, several frames behind f in steady state; status -1
  // while there is none.
  // Lead: pair (k-1, k) is started once frame k+lead-2 has been queued for detection. A frame's detection takes ~130 us
  // from enqueue to its distance field (scan chain, then keyline chain) while the tracker needs a new map every ~70-80 us: with
  // the minimum lead of 3 the kernel trace showed the LM kernel starting 11-12 us after the previous pair's last kernel,
  // waiting for that map; lead 5 keeps two more detections in flight. Costs latency of the returned records, not throughput;
  // flush() drops the frames no pair was started for.
  rebvio_hip_map* m = nullptr;
  const auto td0 = std::chrono::steady_clock::now();
  HIPCHK(hipSetDevice(c->device));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->status = -1;
  }
  if (keylines) *keylines = -1;
  c->min_pool = c->lead + 3 * c->group + 3;
  // Stamp hand-over: a map is reused without a wait only once the host has read its last pair's records, and the queue holds up
  // to kSlots - 1 pairs the host has not read. With kSlots free maps between a release and its reuse (oldest first) that pair has
  // always left the queue: no event and no wait in steady state. (Fewer maps work too, through the fall-back of detect_launch -
  // whose event stands behind EVERY pair queued by then, so the keyline stream waits longer than the map needs.)
  if (!c->handover_events) c->min_pool = std::max(c->min_pool, c->lead + c->group + rebvio_hip_ctx::kSlots + 1);
  int rc;
  if (frame_host) {
    const size_t rowb = (size_t)c->P.cols * px::bytes_per_pixel(fmt);
    rc = detect(c, u8_staging(c, fmt), 1, fmt, ts_us, &m, frame_host, host_pitch ? host_pitch : rowb, rowb);
  } else {
    rc = detect(c, frame_dev, 1, fmt, ts_us, &m, nullptr, 0, 0, mask_frame);
  }
  if (rc) return rc;
  const auto td1 = std::chrono::steady_clock::now();
  c->t_detect_enq += std::chrono::duration<double, std::micro>(td1 - td0).count();
  c->t_frames++;
  if (R_gyro) {  // (checked by the entry: finite)
    m->gyro_set = true;
    std::memcpy(m->gyro_R, R_gyro, sizeof(m->gyro_R));
    c->gyro_stream = true;
  }
  if (c->kf_pending) {  // rebvio_hip_keyframe_next
    m->kf_flag = true;
    c->kf_pending = false;
  }
  c->plain_flushed = false;
  if (c->carry) {  // a flushed stream with gyro rotations goes on from its newest map
    c->frames.push_back(c->carry);
    c->carry = nullptr;
  }
  c->frames.push_back(m);
  const int npairs = group_size((int)c->frames.size(), c->q.count, c->lead, c->group);
  if (npairs >= 1) {
    rc = stream_enqueue_group(c, npairs);
    if (rc) return rc;
  }
  c->t_enq += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - td1).count();
  rc = harvest(c->q, stream_lanes(c), 0);
  if (rc) return rc;
  (void)pop_records(c->q, 1, out, keylines);
  return 0;
}

}  // namespace

int rebvio_hip_push_frame_u8_device(rebvio_hip_ctx* c, const uint8_t* frame_dev, uint64_t ts_us, rebvio_hip_pair_out* out,
                                    int* keylines) {
  return push_frame(c, frame_dev, nullptr, 0, ts_us, out, keylines);
}

int rebvio_hip_push_frame_u8(rebvio_hip_ctx* c, const uint8_t* frame_host, size_t pitch_bytes, uint64_t ts_us, rebvio_hip_pair_out* out,
                             int* keylines) {
  if (!frame_host) return fail_msg("push_frame_u8: null frame", -3);
  return push_frame(c, nullptr, frame_host, pitch_bytes, ts_us, out, keylines);
}

int rebvio_hip_push_frame_px_device(rebvio_hip_ctx* c, const void* frame_dev, int fmt, uint64_t ts_us, rebvio_hip_pair_out* out,
                                    int* keylines) {
  const int rc = check_px(c, "push_frame_px_device", frame_dev, fmt, false, 0);
  if (rc) return rc;
  return push_frame(c, static_cast<const uint8_t*>(frame_dev), nullptr, 0, ts_us, out, keylines, fmt);
}

int rebvio_hip_push_frame_px(rebvio_hip_ctx* c, const void* frame_host, size_t pitch_bytes, int fmt, uint64_t ts_us, rebvio_hip_pair_out* out,
                             int* keylines) {
  const int rc = check_px(c, "push_frame_px", frame_host, fmt, true, pitch_bytes);
  if (rc) return rc;
  return push_frame(c, nullptr, static_cast<const uint8_t*>(frame_host), pitch_bytes, ts_us, out, keylines, fmt);
}

int rebvio_hip_push_frame_px_masked_device(rebvio_hip_ctx* c, const void* frame_dev, int fmt, const uint8_t* mask_dev, uint64_t ts_us,
                                           rebvio_hip_pair_out* out, int* keylines) {
  int rc = check_px(c, "push_frame_px_masked_device", frame_dev, fmt, false, 0);
  if (rc == 0 && !mask_dev) rc = fail_msg("push_frame_px_masked_device: null mask", -3);
  if (rc) return rc;
  return push_frame(c, static_cast<const uint8_t*>(frame_dev), nullptr, 0, ts_us, out, keylines, fmt, mask_dev);
}

namespace {
// Argument check of the *_gyro entries, before anything is queued: every entry of R_gyro finite (-3; no orthonormality check, as
// R_prior of rebvio_hip_track_pair has none), and a frame to measure the rotation from (-7, see rebvio_hip_ctx::plain_flushed).
int check_gyro(const rebvio_hip_ctx* c, const char* who, const float* R_gyro) {
  if (!R_gyro) return 0;
  char buf[256];
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(R_gyro[i])) {
      std::snprintf(buf, sizeof(buf), "%s: R_gyro[%d] is not finite", who, i);
      return fail_msg(buf, -3);
    }
  static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (c->plain_flushed && !c->gyro_stream && std::memcmp(R_gyro, I, sizeof(I)) != 0) {
    std::snprintf(buf, sizeof(buf), "%s: R_gyro is not the identity, but the stream before the flush carried no rotations: its newest map was "
                  "rotated for an identity measurement there and the stream ended. Push this frame with R_gyro = NULL (or the identity) "
                  "as the first frame of a new stream", who);
    return fail_msg(buf, -7);
  }
  return 0;
}
}  // namespace

int rebvio_hip_push_frame_px_gyro_device(rebvio_hip_ctx* c, const void* frame_dev, int fmt, const uint8_t* mask_dev, const float* R_gyro,
                                         uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines) {
  int rc = check_px(c, "push_frame_px_gyro_device", frame_dev, fmt, false, 0);
  if (rc == 0) rc = check_gyro(c, "push_frame_px_gyro_device", R_gyro);
  if (rc) return rc;
  return push_frame(c, static_cast<const uint8_t*>(frame_dev), nullptr, 0, ts_us, out, keylines, fmt, mask_dev, R_gyro);
}

int rebvio_hip_push_frame_px_gyro(rebvio_hip_ctx* c, const void* frame_host, size_t pitch_bytes, int fmt, const float* R_gyro, uint64_t ts_us,
                                  rebvio_hip_pair_out* out, int* keylines) {
  int rc = check_px(c, "push_frame_px_gyro", frame_host, fmt, true, pitch_bytes);
  if (rc == 0) rc = check_gyro(c, "push_frame_px_gyro", R_gyro);
  if (rc) return rc;
  return push_frame(c, nullptr, static_cast<const uint8_t*>(frame_host), pitch_bytes, ts_us, out, keylines, fmt, nullptr, R_gyro);
}

void rebvio_hip_gyro_integrate(float R[9], const float gyro_cam[3], float dt_s) {
  // R = R * SO3::exp(gyro * dt)  (types/imu.hpp:72), with the so3_exp every prior rotation of the library goes through
  const float w[3] = {gyro_cam[0] * dt_s, gyro_cam[1] * dt_s, gyro_cam[2] * dt_s};
  hm::store3(hm::mul(hm::load3(R), hm::so3_exp(w)), R);
}

uint64_t rebvio_hip_pairs_started(rebvio_hip_ctx* c) { return c->pair_seq; }

int rebvio_hip_keyframe_next(rebvio_hip_ctx* c) {
  if (!c) return fail_msg("keyframe_next: null context", -3);
  if (c->batch) return fail_msg("keyframe_next: the context is a lane of a batch; keyframes inside lock-step steps are not supported", -3);
  c->kf_pending = true;
  return 0;
}

// Test hook: the kernels of the NEXT pair this context queues (per-pair API or streaming driver) are handed a wrong sequence
// stamp, so its records look exactly like records read before the pair wrote them; the call that reads them must fail with -12.
int rebvio_hip_test_forge_record_stamp(rebvio_hip_ctx* c) {
  if (!c) return -3;
  c->forge_stamp = true;
  return 0;
}


// Test hook: the hand-over counters of the context's streams since it was created (rebvio_hip_ctx::ho).
int rebvio_hip_test_handover_counters(rebvio_hip_ctx* c, unsigned long long out[10]) {
  if (!c || !out) return -3;
  for (int i = 0; i < 3; ++i) {
    out[3 * i] = c->ho.queued[i].load(std::memory_order_relaxed);
    out[3 * i + 1] = c->ho.skipped[i].load(std::memory_order_relaxed);
    out[3 * i + 2] = c->ho.events[i].load(std::memory_order_relaxed);
  }
  out[9] = c->ho.reuse_fallbacks.load(std::memory_order_relaxed);
  return 0;
}

int rebvio_hip_next_record(rebvio_hip_ctx* c, rebvio_hip_pair_out* out, int* keylines) { return pop_records(c->q, 1, out, keylines); }

int rebvio_hip_flush(rebvio_hip_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  if (c->lm_stamps && c->lm_stamp_n && c->lm_stamp_spec) {
    const double* a = c->lm_stamp_acc;
    const double n = (double)c->lm_stamp_n;
    std::fprintf(stderr,
                 "[rebvio_hip] k_lm_chain_spec workgroup 0, mean us over %llu launches: eval0 %.2f  eval1 %.2f  collect+states %.2f  "
                 "speculative evals [project %.2f  issue gathers %.2f  match %.2f  neighbour round %.2f  weighted sums %.2f  publish %.2f]  "
                 "collect all %.2f  check %.2f  finish %.2f  forwardMatch+extRotVel %.2f  collect sums + device glue %.2f\n",
                 (unsigned long long)c->lm_stamp_n, a[2] / n, a[3] / n, a[4] / n, a[5] / n, a[6] / n, a[7] / n, a[8] / n, a[9] / n, a[10] / n,
                 a[11] / n, a[12] / n, a[13] / n, a[14] / n, a[15] / n);
    if (c->lm_stamps[41])
      std::fprintf(stderr, "[rebvio_hip] end of an LM launch -> start of the next (second half of the pair + stream operations), mean over %llu: %.2f us\n",
                   (unsigned long long)c->lm_stamps[41], (double)c->lm_stamps[40] * 0.01 / (double)c->lm_stamps[41]);
    if (c->lm_stamps[55]) {
      const double m = 0.01 / (double)c->lm_stamps[55];
      std::fprintf(stderr, "[rebvio_hip]   device glue: wait for + sum the extRotVel records %.2f  6x6 solve (wave 0) %.2f  until every wave is there %.2f  "
                   "X, SO3, covariance, records %.2f\n", (double)c->lm_stamps[51] * m, (double)c->lm_stamps[52] * m, (double)c->lm_stamps[53] * m,
                   (double)c->lm_stamps[54] * m);
    }
    if (c->lm_stamps[46]) {
      const double m = 0.01 / (double)c->lm_stamps[46];
      std::fprintf(stderr, "[rebvio_hip]   of which: LM end -> head start %.2f  head start -> tail start %.2f  tail start -> regularize/EKF start %.2f  "
                   "regularize/EKF start -> next LM start %.2f (of which the LM kernel's own prologue: keyline loads + sigma quantile %.2f)\n",
                   (double)c->lm_stamps[42] * m, (double)c->lm_stamps[43] * m, (double)c->lm_stamps[44] * m, (double)c->lm_stamps[45] * m,
                   (double)c->lm_stamps[56] * m);
    }
    if (c->dm_stats) {  // per-wave records of the LAST k_directed_match_c launch
      std::vector<unsigned long long> h(c->dm_stats_words);
      (void)hipMemcpy(h.data(), c->dm_stats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      const size_t nw = std::min((size_t)h[0], c->dm_stats_words / 16 - 1);
      double sum[14] = {0}, mx[14] = {0}, slow = 0;
      size_t with_open = 0;
      for (size_t w = 0; w < nw; ++w) {
        const unsigned long long* r = &h[16 * (w + 1)];
        double tot = 0;
        for (int i = 0; i < 14; ++i) {
          sum[i] += (double)r[i];
          mx[i] = std::max(mx[i], (double)r[i]);
          if (i < 7) tot += (double)r[i];
        }
        slow = std::max(slow, tot);
        with_open += r[11] ? 1 : 0;
      }
      if (nw) {
        static const char* const seg[7] = {"set-up + head probes issued", "mask loads back + scan", "head candidates tested", "chains walked",
                                           "long probes issued", "mask loads back + scan", "long candidates tested"};
        std::fprintf(stderr, "[rebvio_hip]   directedMatch (compact), last launch, %zu waves: keylines %.0f  t_steps > 4: %.0f  matched in the head %.0f  long "
                     "searches %.0f (max per wave %.0f, waves with any %zu)  head candidates %.0f (max %.0f)  long-search candidates %.0f (max %.0f)\n",
                     nw, sum[8], sum[9], sum[10], sum[11], mx[11], with_open, sum[12], mx[12], sum[13], mx[13]);
        std::fprintf(stderr, "[rebvio_hip]   per wave, us mean / max:");
        for (int i = 0; i < 7; ++i) std::fprintf(stderr, "  %s %.2f / %.2f", seg[i], sum[i] * 0.01 / (double)nw, mx[i] * 0.01);
        std::fprintf(stderr, "  | slowest wave %.2f\n", slow * 0.01);
      }
    }
  } else if (c->lm_stamps && c->lm_stamp_n) {
    const int calls = (int)c->P.iterations + 1;
    std::fprintf(stderr, "[rebvio_hip] k_lm_chain workgroup 0, mean us per segment over %llu launches\n", (unsigned long long)c->lm_stamp_n);
    std::fprintf(stderr, "  prologue %.2f\n", c->lm_stamp_acc[1] / c->lm_stamp_n);
    for (int k = 0; k < calls; ++k) {
      const double* a = c->lm_stamp_acc + 1 + k * 6;
      const double n = (double)c->lm_stamp_n;
      std::fprintf(stderr, "  eval %d: collect %.2f  lm_step %.2f  evaluate %.2f  wave-reduce %.2f  carry+publish %.2f  (loop edge %.2f)\n", k,
                   a[1] / n, a[2] / n, a[3] / n, a[4] / n, a[5] / n, k + 1 < calls ? a[6] / n : 0.0);
    }
    std::fprintf(stderr, "  final collect+lm_step %.2f  forwardMatch+extRotVel %.2f\n", c->lm_stamp_acc[1 + calls * 6] / c->lm_stamp_n,
                 c->lm_stamp_acc[2 + calls * 6] / c->lm_stamp_n);
  }
  if (std::getenv("REBVIO_HIP_DEBUG") && c->t_frames) {
    const double n = (double)c->t_frames;
    std::fprintf(stderr,
                 "[rebvio_hip] host time per frame (us): detect hand-over %.1f  pair enqueue %.1f  waiting for result slots %.1f | long "
                 "directedMatch searches per pair %.0f\n",
                 c->t_detect_enq / n, c->t_enq / n, c->q.t_wait / n, c->t_queued / n);
    if (c->t_det_n)
      std::fprintf(stderr, "[rebvio_hip] detect: %.1f us of launches per frame over %llu frames\n", c->t_det_launch / (double)c->t_det_n,
                   (unsigned long long)c->t_det_n);
    static const char* const on[3] = {"track", "scan", "keyline"};
    for (int i = 0; i < 3; ++i)
      std::fprintf(stderr, "[rebvio_hip] %s stream since create: waits queued %llu, skipped %llu, events recorded %llu%s", on[i],
                   (unsigned long long)c->ho.queued[i].load(), (unsigned long long)c->ho.skipped[i].load(),
                   (unsigned long long)c->ho.events[i].load(), i < 2 ? "\n" : "");
    std::fprintf(stderr, " | map reuse fall-backs %llu (hand-over: %s)\n", (unsigned long long)c->ho.reuse_fallbacks.load(),
                 c->handover_events ? "events" : "stamps");
    // (the counters start again: a caller that flushes between phases reads each phase on its own)
    c->t_detect_enq = c->t_enq = c->q.t_wait = c->t_queued = 0;
    c->t_frames = 0;
    c->t_det_launch = 0;
    c->t_det_n = 0;
  }
  int rc = 0;
  while (rc == 0 && c->frames.size() >= 2)  // the pairs no group was started for yet
    rc = stream_enqueue_group(c, std::min(c->group, (int)c->frames.size() - 1));
  if (rc == 0) rc = drain(c->q, stream_lanes(c));
  if (c->gyro_stream && rc == 0 && c->frames.size() == 1 && c->frames[0]->in_use && !c->frames[0]->pre_rotated) {
    // A stream that carries gyro rotations continues across the flush: the rotation of the next frame pushed spans the interval
    // from this map's frame, and the last pair has left the map un-rotated for it (GlueParams::has_next == 0).
    c->carry = c->frames[0];
    c->frames.clear();
  } else if (!c->frames.empty() && !c->gyro_stream) {
    c->plain_flushed = true;  // the stream ends here, its newest map rotated for an identity measurement that will not come
  }
  for (auto* m : c->frames)
    if (m->in_use) release_map(m, nullptr);
  c->frames.clear();
  // The last second half binned the sigma histogram for a pair that will not come (its next-rotation rides in the last
  // kernel): a stream that continues after the flush must not find those counts under its first pair's (they put the
  // quantile cut below every fresh keyline's sigma and the pair came back with status 1).
  HIPCHK(hipMemsetAsync(c->hist, 0, 128 * sizeof(int), c->s_trk));
  HIPCHK(hipStreamSynchronize(c->s_det));
  HIPCHK(hipStreamSynchronize(c->s_key));
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  return rc;
}

int rebvio_hip_test_glue(rebvio_hip_ctx* c, const float vel[3], const float JtJ6[6], float F, float sigma_rho_min, int accept_mask,
                         const float* xrv, int n_new, float frame_dt, const float Bg[3], const float W_Bg[9], const float R_prior[9],
                         rebvio_hip_pair_out* out_dev, float* state_dev, float* second_dev, rebvio_hip_pair_out* out_host, float* state_host,
                         float* second_host) {
  HIPCHK(hipSetDevice(c->device));
  if (n_new < 0 || n_new > c->P.keylines_max) return fail_msg("test_glue: n_new out of range", -3);
  static_assert(sizeof(GlueState) == 22 * sizeof(float) && sizeof(GlueDev) == 44 * sizeof(float), "record layouts of the test hook");
  LmState lm;
  std::memset(&lm, 0, sizeof(lm));
  for (int i = 0; i < 3; ++i) lm.vel[i] = vel[i];
  for (int i = 0; i < 6; ++i) lm.JtJ[i] = JtJ6[i];
  lm.F = F;
  lm.sigma_rho_min = sigma_rho_min;
  lm.accept_mask = accept_mask;
  GlueState st;
  for (int i = 0; i < 3; ++i) st.Bg[i] = Bg[i];
  std::memcpy(st.W_Bg, W_Bg, sizeof(st.W_Bg));
  std::memcpy(st.R, R_prior, sizeof(st.R));
  st.pad = 0.f;
  const int nb = div_up(n_new, 256);
  // host form (what rebvio_hip_track_pair runs)
  {
    GlueState sh = st;
    GlueDev gl;
    std::memset(&gl, 0, sizeof(gl));
    std::memset(out_host, 0, sizeof(*out_host));
    GlueParams gph = glue_params(c, frame_dt);
    gph.has_next = c->test_has_next;
    std::memcpy(gph.R_next, c->test_R_next, sizeof(gph.R_next));
    hm::pair_glue_core(lm, xrv, n_new, gph, sh, gl, *out_host);
    std::memcpy(state_host, &sh, sizeof(sh));
    std::memcpy(second_host, &gl, sizeof(gl));
  }
  // device form (what the streaming and batch drivers run), through the stand-alone glue kernel
  { const int rc_ts = trk_sync(c); if (rc_ts) return rc_ts; }
  char* buf = nullptr;
  const size_t xb = (size_t)std::max(nb, 1) * kXrvStride * sizeof(float);
  Owned scratch;
  HIPCHK(scratch.device(&buf, sizeof(LmState) + sizeof(MapState) + 2 * sizeof(GlueState) + sizeof(GlueDev) + sizeof(GlueRec) + xb));
  LmState* d_lm = reinterpret_cast<LmState*>(buf);
  MapState* d_ms = reinterpret_cast<MapState*>(d_lm + 1);
  GlueState* d_st = reinterpret_cast<GlueState*>(d_ms + 1);
  GlueDev* d_gl = reinterpret_cast<GlueDev*>(d_st + 2);
  GlueRec* d_rec = reinterpret_cast<GlueRec*>(d_gl + 1);
  float* d_xrv = reinterpret_cast<float*>(d_rec + 1);
  MapState ms;
  std::memset(&ms, 0, sizeof(ms));
  ms.n = n_new;
  HIPCHK(hipMemcpy(d_lm, &lm, sizeof(lm), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_ms, &ms, sizeof(ms), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_st, &st, sizeof(st), hipMemcpyHostToDevice));
  if (nb > 0) HIPCHK(hipMemcpy(d_xrv, xrv, (size_t)nb * kXrvStride * sizeof(float), hipMemcpyHostToDevice));
  MapDev fake{};
  fake.st = d_ms;
  GlueArgs ga;
  ga.lm = d_lm;
  ga.xrv = d_xrv;
  ga.st_in = d_st;
  ga.st_out = d_st + 1;
  ga.rec = d_rec;
  ga.gd_copy = d_gl;
  ga.stage = nullptr;
  ga.seq = 1u;
  ga.gp = glue_params(c, frame_dt);
  ga.gp.has_next = c->test_has_next;
  std::memcpy(ga.gp.R_next, c->test_R_next, sizeof(ga.gp.R_next));
  launch_pair_glue(c->s_trk, fake, ga);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->s_trk));
  GlueRec rec;
  GlueState sd;
  GlueDev gd;
  HIPCHK(hipMemcpy(&rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sd, d_st + 1, sizeof(sd), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&gd, d_gl, sizeof(gd), hipMemcpyDeviceToHost));
  *out_dev = rec.out;
  std::memcpy(state_dev, &sd, sizeof(sd));
  std::memcpy(second_dev, &gd, sizeof(gd));
  if (std::memcmp(&rec.gs, &sd, sizeof(sd)) != 0) return fail_msg("test_glue: the record's state copy differs from the state written", -5);
  return 0;
}

int rebvio_hip_test_glue_set_next(rebvio_hip_ctx* c, const float* R_next, int has_next) {
  if (!c) return -3;
  static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(c->test_R_next, R_next ? R_next : I, sizeof(c->test_R_next));
  c->test_has_next = R_next ? (has_next != 0) : 1;
  return 0;
}

int rebvio_hip_profile_enable(rebvio_hip_ctx* c, int on) {
  (void)c;
  std::lock_guard<std::mutex> g(g_prof.mu);
  g_prof.on = on != 0;
  g_prof.stride = on > 1 ? on : 1;  // on = N > 1: sample every N-th launch of each kernel
  if (g_prof.on && g_prof.free_events.size() < 256)
    for (int i = 0; i < 512; ++i) {
      hipEvent_t e;
      if (hipEventCreate(&e) == hipSuccess) g_prof.free_events.push_back(e);
    }
  return 0;
}

int rebvio_hip_profile_select(rebvio_hip_ctx* c, const char* only_kernel) {
  (void)c;
  std::lock_guard<std::mutex> g(g_prof.mu);
  g_prof.only = only_kernel ? only_kernel : "";
  return 0;
}

int rebvio_hip_profile_reset(rebvio_hip_ctx* c) {
  (void)c;
  std::lock_guard<std::mutex> g(g_prof.mu);
  g_prof.drain();
  g_prof.acc.clear();
  return 0;
}

int rebvio_hip_profile_read(rebvio_hip_ctx* c, char* names, size_t names_cap, double* avg_us, int* calls, int cap) {
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> g(g_prof.mu);
  g_prof.drain();
  std::string all;
  int k = 0;
  for (auto& kv : g_prof.acc) {
    if (k >= cap) break;
    const std::string& nm = g_prof.names[kv.first];
    if (all.size() + nm.size() + 2 > names_cap) break;
    all += nm;
    all += '\n';
    avg_us[k] = kv.second.second ? kv.second.first / kv.second.second : 0.0;
    calls[k] = kv.second.second;
    ++k;
  }
  if (names_cap) {
    std::strncpy(names, all.c_str(), names_cap - 1);
    names[names_cap - 1] = 0;
  }
  return k;
}

int rebvio_hip_device_alloc(rebvio_hip_ctx* c, size_t bytes, void** out) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMalloc(out, bytes));
  return 0;
}
int rebvio_hip_device_free(rebvio_hip_ctx* c, void* p) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipFree(p));
  return 0;
}
int rebvio_hip_device_upload(rebvio_hip_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

}  // extern "C"

// ---- batch of camera streams on one GPU (rebvio_hip_batch_*) ----------------------------------------------------------------------------------
// B independent rebvio pipelines (B instances of rebvio::Rebvio, each with its own detector, tracker and maps: rebvio.hpp:91-112)
// advanced in LOCK-STEP by batched launches: every kernel of the per-frame path runs once per step with lane = blockIdx.z.
// Why not B contexts side by side: measured on MI355X (tools/multi_ctx.py), several contexts per process do not overlap -
// with stream priorities two pipelines starve each other's low-priority stages (2 x 3.0k frames/s against 11.8k for one),
// without them they merely share the single-stream rate, and with more hardware queues every pipeline gets slower - while a
// single 640x480 stream keeps under a tenth of the chip busy because each of its kernels is a short latency chain. A batched
// launch costs about the same latency as a single one, so B lanes raise the frame rate almost B-fold until the chip fills.
// Each lane is a full rebvio_hip_ctx (its buffers, maps, glue state) that adopts the batch's three streams; per lane results
// are bit-identical to a stand-alone context fed the same frames (same kernel bodies, same per-lane reduction order).
struct rebvio_hip_batch {
  int B = 0;
  int device = 0;
  rebvio_hip_params P{};
  KParams K{};
  Owned own;  // the batch's buffers and events, and the three streams its lanes adopt
  SharedStreams st{};
  std::vector<rebvio_hip_ctx*> lane;
  LaneStatic* ls_dev = nullptr;
  std::vector<LaneStatic> ls_host;  // what ls_dev holds (re-uploaded when a lane's lens model changes)
  bool lens = false;                // every lane has a lens model: the batched front end runs ahead of the scans
  MapDev* maptab_dev = nullptr;
  hipEvent_t ev_scan[kDetPar]{}, ev_flag[kDetPar]{};
  bool ev_flag_used[kDetPar]{};
  static constexpr int kReadyRing = 16;
  hipEvent_t ev_ready[kReadyRing]{};  // keylines + distance fields of a step finished (keyline stream)
  uint64_t step = 0;
  struct Frame {
    std::vector<rebvio_hip_map*> m;  // one detected map per lane
    uint64_t step;
  };
  std::deque<Frame> frames;
  PairQueue q;  // steps in flight and records waiting for the caller
  uint64_t pair_seq = 0;
  uint32_t stamp_seq = 0;   // sequence stamps of the lanes' records, one value per step (rebvio_hip_ctx::stamp_seq)
  bool forge_stamp = false;
  int lead = 4;
  int group = 2;          // steps queued together (REBVIO_HIP_BATCH_GROUP 1..4, see stream_enqueue_group)
  int lm_lanes_per_launch = 1;  // lanes whose LM workgroups the device holds together (lm_chain_b_max_lanes)
  int lm_capacity_wgs = 0;      // ... and the workgroups that is (shared with the other registered users, see Residency)
  // REBVIO_HIP_DEBUG: host time per step of the detect worker's launches, of the caller's track enqueue and of its waits for
  // result slots (printed by rebvio_hip_batch_flush)
  bool dbg = false;
  std::atomic<uint64_t> t_det_ns{0};
  double t_trk_enq = 0;
  int dm_head_form = 0;   // REBVIO_HIP_BATCH_DM_HEAD: 0 by lane count and map size, 1 compact8, 2 compact4, 3 compact1
  bool poisoned = false;  // a step failed half way (some lanes prepared, others not): every later call is refused
  // detect-enqueue worker: launches the detect stage of a step while the caller thread launches the track stage (the
  // reference's data-acquisition thread, rebvio.cpp:28). A batch step's detect launches take long enough on the host for the
  // split to pay (the single stream measured it the other way round: DESIGN.md 6d).
  struct DetStep {
    LaneDynB dyn;
    int par;
    uint64_t step;
    hipEvent_t reuse_done;  // last consumer of the maps this step reuses (null: fresh maps)
    std::vector<rebvio_hip_map*> maps;
    bool lens;
    int fmt = 0;  // pixel format of every lane's frame
    bool masked = false;  // some lane has a detection mask: the masked candidate kernel, with `masks`
    LaneMasks masks{};
  };
  std::thread det_thread;
  std::mutex det_mu;
  std::condition_variable det_cv;
  std::deque<DetStep> det_jobs;
  std::atomic<uint64_t> det_done_steps{0};  // steps whose detect stage has been enqueued (their events are recorded)
  bool det_stop = false;
  std::string det_error;
};

namespace {
int batch_upload_map_entry(rebvio_hip_batch* b, int lane, rebvio_hip_map* m) {
  rebvio_hip_ctx* c = b->lane[lane];
  int idx = -1;
  for (size_t i = 0; i < c->pool.size(); ++i)
    if (c->pool[i] == m) idx = (int)i;
  if (idx < 0 || idx >= kLaneMaps) return fail_msg("batch: edge-map pool of a lane outgrew the lane's map table (release maps)", -2);
  m->tab_idx = idx;
  m->canon = m->d;
  HIPCHK(hipMemcpy(b->maptab_dev + (size_t)lane * kLaneMaps + idx, &m->canon, sizeof(MapDev), hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));  // (null-stream work is not ordered against the batch's non-blocking streams: see alloc_map)
  return 0;
}
inline unsigned map_swap_bits(const rebvio_hip_map* m) { return (m->d.rs != m->canon.rs ? 1u : 0u) | (m->d.grad != m->canon.grad ? 2u : 0u); }

int batch_detect_launch(rebvio_hip_batch* b, const rebvio_hip_batch::DetStep& j) {
  const int B = b->B, par = j.par;
  if (b->ev_flag_used[par]) HIPCHK(hipStreamWaitEvent(b->st.s_det, b->ev_flag[par], 0));
  // k_dog_mag_b + k_keyline_flag_b: the single stream's fused candidate kernel moves the last box pass from the scan stream to
  // the keyline stream, measured SLOWER for batches (8 lanes 42.4 k -> 39.7 k frames/s, 4 lanes 32.9 k -> 32.2 k), like the
  // single stream's other moves of scan work to the keyline stream
  launch_scale_space_b(b->st.s_det, b->K, 0, B, b->ls_dev, j.dyn, b->lane[0]->widths, j.lens, j.fmt);
  HIPCHK(hipEventRecord(b->ev_scan[par], b->st.s_det));
  HIPCHK(hipStreamWaitEvent(b->st.s_key, b->ev_scan[par], 0));
  if (j.reuse_done) HIPCHK(hipStreamWaitEvent(b->st.s_key, j.reuse_done, 0));
  launch_keylines_b(b->st.s_key, b->K, B, b->ls_dev, b->maptab_dev, j.dyn, j.masked ? &j.masks : nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(b->ev_flag[par], b->st.s_key));
  b->ev_flag_used[par] = true;
  launch_df_build_b(b->st.s_key, b->K, B, b->ls_dev, b->maptab_dev, j.dyn);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(b->ev_ready[j.step % rebvio_hip_batch::kReadyRing], b->st.s_key));
  for (int l = 0; l < B; ++l) {
    // The single-map entries (size, download, ...) wait on the map's own event. Letting the step's one event stand for every
    // lane's map (eight marker packets fewer on the keyline stream) was measured SLOWER, 42.5 k -> 41.9 k frames/s at 8 lanes,
    // three alternating runs: the packets space the keyline stream's kernels apart, to the benefit of the other two streams.
    HIPCHK(hipEventRecord(j.maps[l]->ready, b->st.s_key));
    j.maps[l]->enqueued.store(1, std::memory_order_release);
  }
  return 0;
}

void batch_det_worker(rebvio_hip_batch* b) {
  (void)hipSetDevice(b->device);
  for (;;) {
    rebvio_hip_batch::DetStep j;
    {
      std::unique_lock<std::mutex> lk(b->det_mu);
      b->det_cv.wait(lk, [&] { return b->det_stop || !b->det_jobs.empty(); });
      if (b->det_jobs.empty()) return;
      j = b->det_jobs.front();
      b->det_jobs.pop_front();
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int drc = batch_detect_launch(b, j);
    if (b->dbg) b->t_det_ns.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
    if (drc != 0) {
      std::lock_guard<std::mutex> lk(b->det_mu);
      b->det_error = g_err;
      for (auto* m : j.maps) m->enqueued.store(1, std::memory_order_release);
    }
    b->det_done_steps.store(j.step + 1, std::memory_order_release);
  }
}

LaneSet batch_lanes(const rebvio_hip_batch* b) { return LaneSet{b->lane.data(), b->B, b->device, b, "batch: "}; }

// `nsteps` consecutive steps' pairs, all lanes, as one group on the track stream (see stream_enqueue_group): per step [rotate +]
// LM kernel with every lane's glue at its end, directedMatch head, tail, regularize / EKF / next rotation; per group one wait
// for the newest step's detection and one event
int batch_enqueue_group(rebvio_hip_batch* b, int nsteps) {
  while (b->q.count + nsteps > rebvio_hip_ctx::kSlots - 1) {
    const int rc = harvest(b->q, batch_lanes(b), 1);
    if (rc) return rc;
  }
  hipStream_t s = b->st.s_trk;
  {
    const uint64_t newest = b->frames[(size_t)nsteps].step;
    while (b->det_done_steps.load(std::memory_order_acquire) <= newest) std::this_thread::yield();  // its event has been recorded
    HIPCHK(hipStreamWaitEvent(s, b->ev_ready[newest % rebvio_hip_batch::kReadyRing], 0));  // (earlier steps: same stream order)
  }
  const int calls = (int)b->P.iterations + 1;
  int last_slot = -1;
  std::vector<rebvio_hip_batch::Frame> olds;
  for (int g = 0; g < nsteps; ++g) {
    const rebvio_hip_batch::Frame of = b->frames[0], nf = b->frames[1];
    const int slot = (int)(b->pair_seq % rebvio_hip_ctx::kSlots);
    const int gpar = (int)(b->pair_seq & 1);
    const uint32_t step_seq = next_stamp(&b->stamp_seq);
    LaneDynB dyn{};
    // every lane's gyro rotation for its NEXT pair: what the step behind nf was pushed with (the identity for a lane pushed without
    // one, and for the last step in front of a flush: a batch's flush ends every lane's stream, whatever it carried)
    LaneGyroB gyro;
    for (int l = 0; l < kMaxLanes; ++l) hm::store3(hm::identity3(), gyro.R_next[l]);
    for (int l = 0; l < b->B; ++l) {
      rebvio_hip_ctx* c = b->lane[l];
      rebvio_hip_map *om = of.m[l], *nm = nf.m[l];
      if (b->frames.size() > 2 && b->frames[2].m[l]->gyro_set) std::memcpy(gyro.R_next[l], b->frames[2].m[l]->gyro_R, sizeof(gyro.R_next[l]));
      c->df_map = nm;
      dyn.v[l].seq = (b->forge_stamp && l == b->B - 1) ? (step_seq ^ 0x40000000u) : step_seq;
      if (!om->pre_rotated) {
        const int rc = start_lane_stream(c, om, nm, gpar);
        if (rc) return rc;
      }
      LaneDyn& d = dyn.v[l];
      d.nm = (short)nm->tab_idx;
      d.om = (short)om->tab_idx;
      d.nm_swap = (unsigned char)map_swap_bits(nm);
      d.om_swap = (unsigned char)map_swap_bits(om);
      d.slot = (unsigned char)slot;
      d.gpar = (unsigned char)gpar;
      d.tag_base = c->lm_tag_base;
      advance_lm_tags(c, calls);
    }
    // one launch for all lanes: the most cautious of the lanes' choices (1 sequential; otherwise the LATEST first speculative
    // evaluation any lane asks for)
    int spec_now = 2;
    for (auto* c : b->lane) {
      const int ch = lm_kernel_choice(c);
      if (ch == 1 || spec_now == 1)
        spec_now = 1;
      else
        spec_now = std::max(spec_now, ch);
    }
    const float frame_dt = (float)((double)(float)(nf.m[0]->ts - of.m[0]->ts) / 1000000.0);  // rebvio.cpp:183
    // this batch's share of the device: the capacity split evenly among the live users of the persistent kernels on this GPU
    const int users = std::max(1, residency_users(b->device));
    const int per_lane_wgs = (b->K.kmax + 511) / 512;
    const int lanes_now = users <= 1 ? b->lm_lanes_per_launch : std::max(1, std::min(b->lm_lanes_per_launch, b->lm_capacity_wgs / users / per_lane_wgs));
    launch_lm_chain_b(s, b->K, b->B, lanes_now, b->ls_dev, b->maptab_dev, dyn, calls, spec_now, glue_params(b->lane[0], frame_dt), gyro);
    const int gate = (int)b->P.global_min_matches_threshold;
    launch_b_chain_b(s, b->K, b->B, b->ls_dev, b->maptab_dev, dyn, b->P.search_range, gate > 0 ? gate : 0, b->dm_head_form);
    HIPCHK(hipGetLastError());
    for (int l = 0; l < b->B; ++l) {  // (a lane whose pair is skipped for a NaN velocity still gets its next rotation applied)
      rebvio_hip_map* nm = nf.m[l];
      std::swap(nm->d.rs, nm->d.rs_tmp);
      std::swap(nm->d.grad, nm->d.grad_tmp);
      nm->pre_rotated = true;
    }
    b->forge_stamp = false;
    PairQueue::Step f;
    for (int l = 0; l < b->B; ++l) f.nm[l] = nf.m[l];
    f.seq = step_seq;
    f.slot = slot;
    b->q.push_back(f);
    olds.push_back(of);
    b->frames.pop_front();
    b->pair_seq++;
    last_slot = slot;
  }
  HIPCHK(hipEventRecord(b->q.slot_ev[last_slot], s));
  for (int g = 0; g < nsteps; ++g) b->q[b->q.count - 1 - g].ev_slot = last_slot;
  for (auto& of : olds)
    for (auto* m : of.m) release_map(m, b->q.slot_ev[last_slot], false);  // the group's one event covers every old map
  return 0;
}

}  // namespace

extern "C" {

void rebvio_hip_batch_destroy(rebvio_hip_batch* b) {
  if (!b) return;
  residency_remove(b->device, b);
  (void)hipSetDevice(b->device);
  if (b->det_thread.joinable()) {
    {
      std::lock_guard<std::mutex> lk(b->det_mu);
      b->det_stop = true;
    }
    b->det_cv.notify_all();
    b->det_thread.join();
  }
  (void)hipDeviceSynchronize();
  // the maps of queued steps and of the pairs in flight are the batch's own, not handles a caller holds
  for (auto& f : b->frames)
    for (auto* m : f.m) m->in_use = false;
  for (int i = 0; i < b->q.count; ++i)
    for (int l = 0; l < b->B; ++l) b->q[i].nm[l]->in_use = false;
  for (auto* c : b->lane) rebvio_hip_destroy(c);
  b->own.release();
  delete b;
}

int rebvio_hip_batch_create(const rebvio_hip_params* p, int lanes, rebvio_hip_batch** out) {
  *out = nullptr;
  if (lanes < 1 || lanes > kMaxLanes) return fail_msg("batch: lanes must be in 1..16", -3);
  if (int rc = check_search_range(p)) return rc;
  if (int rc = check_detection_params(p)) return rc;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail_msg("no HIP device present: the gfx950 backend has no CPU fallback", -4);
  if (p->device_id < 0 || p->device_id >= ndev) return fail_msg("device_id out of range", -3);
  HIPCHK(hipSetDevice(p->device_id));
  int lm_lanes_per_launch = 1;
  {
    // The persistent LM kernel exchanges records among the workgroups of a lane, and every workgroup of a launch has to be
    // resident for that (no assumption about dispatch order): the batch driver launches it for as many lanes at a time as the
    // device holds together (lm_chain_b_max_lanes; 8 lanes of 16 k keylines on an MI355X). Not even one lane: refused here
    // instead of finding out from an exchange time-out (-9).
    lm_lanes_per_launch = lm_chain_b_max_lanes(p->device_id, p->keylines_max, (int)p->iterations + 1);
    if (lm_lanes_per_launch < 1) {
      char msg[200];
      std::snprintf(msg, sizeof(msg), "batch: the %d LM workgroups of one lane (%d keylines) do not fit this device together",
                    (p->keylines_max + 511) / 512, p->keylines_max);
      return fail_msg(msg, -3);
    }
  }
  rebvio_hip_batch* b = new rebvio_hip_batch;
  b->lm_lanes_per_launch = lm_lanes_per_launch;
  b->lm_capacity_wgs = lm_chain_b_capacity_wgs(p->device_id, p->keylines_max, (int)p->iterations + 1);
  b->dbg = std::getenv("REBVIO_HIP_DEBUG") != nullptr;
  struct Guard {
    rebvio_hip_batch* b;
    ~Guard() {
      if (b) rebvio_hip_batch_destroy(b);
    }
  } guard{b};
  b->B = lanes;
  b->device = p->device_id;
  residency_add(b->device, b, std::min(lanes, lm_lanes_per_launch) * ((p->keylines_max + 511) / 512));
  b->P = *p;
  // the three stages of a step overlap across steps like the stages of one stream do; one priority class for all
  // (see the comment on rebvio_hip_batch: priorities are what made pipelines starve each other)
  HIPCHK(b->own.stream(&b->st.s_det, hipStreamNonBlocking));
  HIPCHK(b->own.stream(&b->st.s_key, hipStreamNonBlocking));
  HIPCHK(b->own.stream(&b->st.s_trk, hipStreamNonBlocking));
  for (int l = 0; l < lanes; ++l) {
    rebvio_hip_ctx* c = nullptr;
    rebvio_hip_params pl = *p;
    if (pl.map_pool <= 0) pl.map_pool = 8;
    t_adopt_streams = &b->st;
    const int rc = rebvio_hip_create(&pl, &c);
    t_adopt_streams = nullptr;
    if (rc) return rc;
    c->batch = b;
    b->lane.push_back(c);
  }
  b->K = b->lane[0]->K;
  std::vector<LaneStatic> ls((size_t)lanes);
  HIPCHK(b->own.device(&b->maptab_dev, (size_t)lanes * kLaneMaps, 0));
  for (int l = 0; l < lanes; ++l) {
    rebvio_hip_ctx* c = b->lane[l];
    LaneStatic& L = ls[l];
    for (int f = 0; f < 2; ++f) {
      L.sa[f] = c->sb.a[f];
      L.sb[f] = c->sb.b[f];
    }
    for (int i = 0; i < kDetPar; ++i) {
      L.dog2[i] = c->dog2[i];
      L.mag2[i] = c->mag2[i];
      L.rowcount2[i] = c->rowcount2[i];
      L.undist_img[i] = c->undist_img[i];
    }
    L.stash = c->db.stash;
    L.bits = c->db.bits;
    L.det = c->det;
    L.lm = c->lm;
    L.lm_zero = c->lm_zero;
    L.lm_xch = c->lm_xch;
    L.lm_bar_err = c->lm_bar_err;
    L.hist = c->hist;
    for (int i = 0; i < rebvio_hip_ctx::kSlots; ++i) {
      L.slot[i] = c->slot[i];
      L.rec[i] = c->rec[i];
      L.glue_stage = c->glue_stage;
    }
    L.glue_dev = c->glue_dev;
    L.gstate = c->gstate;
    L.xrv_part = c->xrv_part;
    L.undist_map = c->undist_map;
    for (auto* m : c->pool) {
      const int rc = batch_upload_map_entry(b, l, m);
      if (rc) return rc;
    }
  }
  HIPCHK(b->own.device(&b->ls_dev, ls.size()));
  HIPCHK(hipMemcpy(b->ls_dev, ls.data(), ls.size() * sizeof(LaneStatic), hipMemcpyHostToDevice));
  b->ls_host = ls;
  for (int i = 0; i < kDetPar; ++i) {
    HIPCHK(b->own.event(&b->ev_scan[i]));
    HIPCHK(b->own.event(&b->ev_flag[i]));
  }
  for (auto& e : b->ev_ready) HIPCHK(b->own.event(&e));
  for (auto& e : b->q.slot_ev) HIPCHK(b->own.event(&e));
  if (const char* e = std::getenv("REBVIO_HIP_BATCH_LEAD")) b->lead = std::min(8, std::max(3, std::atoi(e)));
  if (const char* e = std::getenv("REBVIO_HIP_BATCH_GROUP")) b->group = std::min(4, std::max(1, std::atoi(e)));
  if (const char* e = std::getenv("REBVIO_HIP_BATCH_DM_HEAD"))
    b->dm_head_form = dm_form_by_name(e);
  HIPCHK(hipDeviceSynchronize());
  guard.b = nullptr;
  *out = b;
  return 0;
}

int rebvio_hip_batch_lanes(rebvio_hip_batch* b) { return b->B; }

// as rebvio_hip_test_forge_record_stamp, for the last lane of the next step
int rebvio_hip_batch_test_forge_record_stamp(rebvio_hip_batch* b) {
  if (!b) return -3;
  b->forge_stamp = true;
  return 0;
}
long rebvio_hip_test_live_resources(void) { return g_live_resources.load(std::memory_order_relaxed); }
rebvio_hip_ctx* rebvio_hip_batch_lane(rebvio_hip_batch* b, int lane) { return (lane >= 0 && lane < b->B) ? b->lane[lane] : nullptr; }

// masks_dev: this step's per-frame detection mask of every lane (null array, or a null entry: none); R_gyro: the gyro rotation
// of every lane's frame (null array, or a null entry: the identity)
static int batch_push(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines,
                      const uint8_t* const* masks_dev = nullptr, const float* const* R_gyro = nullptr) {
  HIPCHK(hipSetDevice(b->device));
  if (b->poisoned) return fail_msg("batch: an earlier step failed half way; the lanes are out of lock-step (destroy the batch)", -11);
  const int B = b->B;
  for (int l = 0; l < B; ++l) {
    if (out) {
      std::memset(&out[l], 0, sizeof(out[l]));
      out[l].status = -1;
    }
    if (keylines) keylines[l] = -1;
  }
  {
    std::lock_guard<std::mutex> lk(b->det_mu);
    if (!b->det_error.empty()) return fail_msg(b->det_error.c_str(), -8);
  }
  {
    // lens models (rebvio_hip_set_undistort on a lane's context, camera.hpp:39-40,54-58): all lanes or none; a change is
    // picked up here (set_undistort has synchronised the device)
    int with = 0;
    bool changed = false;
    for (int l = 0; l < B; ++l) {
      rebvio_hip_ctx* c = b->lane[l];
      with += c->undist_map ? 1 : 0;
      LaneStatic& L = b->ls_host[(size_t)l];
      if (L.undist_map != c->undist_map || std::memcmp(L.undist_img, c->undist_img, sizeof(L.undist_img)) != 0) {
        L.undist_map = c->undist_map;
        for (int i = 0; i < kDetPar; ++i) L.undist_img[i] = c->undist_img[i];
        changed = true;
      }
    }
    if (with != 0 && with != B) return fail_msg("batch: set the lens model on every lane or on none", -3);
    if (changed) {
      while (b->det_done_steps.load(std::memory_order_acquire) < b->step) std::this_thread::yield();
      HIPCHK(hipStreamSynchronize(b->st.s_det));
      HIPCHK(hipMemcpy(b->ls_dev, b->ls_host.data(), b->ls_host.size() * sizeof(LaneStatic), hipMemcpyHostToDevice));
      HIPCHK(hipStreamSynchronize(nullptr));
    }
    b->lens = with == B;
  }
  // ---- detect stage of this step (detect_launch for every lane at once) ----
  rebvio_hip_batch::Frame fr;
  fr.step = b->step;
  fr.m.resize((size_t)B);
  LaneDynB dyn{};
  const int par = (int)(b->step % kDetPar);
  rebvio_hip_map* last_reused = nullptr;
  LaneMasks masks{};
  bool masked = false;
  for (int l = 0; l < B; ++l) {
    rebvio_hip_ctx* c = b->lane[l];
    rebvio_hip_ctx::DetJob job;
    c->min_pool = std::min(kLaneMaps - 2, b->lead + 3 * b->group + 3);
    int rc = detect_prepare(c, frames_dev[l], 1, ts_us, &job, fmt, masks_dev ? masks_dev[l] : nullptr);
    if (rc == 0) {
      rebvio_hip_map* m = job.m;
      if (m->tab_idx < 0 || std::memcmp(&m->canon.pos, &m->d.pos, sizeof(void*)) != 0)  // a map the pool has just grown by
        rc = batch_upload_map_entry(b, l, m);
    }
    if (rc) {
      // lanes 0 .. l-1 have taken maps and advanced their servo rings for a step that will not run: the batch cannot
      // continue in lock-step
      if (l > 0) b->poisoned = true;
      return rc;
    }
    rebvio_hip_map* m = job.m;
    // a pooled map comes back with whatever ping-pong state its last pair left: the detector writes the canonical arrays
    m->d = m->canon;
    fr.m[l] = m;
    if (R_gyro && R_gyro[l]) {  // (checked by the entry: finite)
      m->gyro_set = true;
      std::memcpy(m->gyro_R, R_gyro[l], sizeof(m->gyro_R));
      c->gyro_stream = true;
    }
    if (l == B - 1) last_reused = m;
    LaneDyn& d = dyn.v[l];
    d.img = frames_dev[l];
    d.nm = (short)m->tab_idx;
    d.om = -1;
    d.prev = -1;
    if (job.prev_st)
      for (auto* pm : c->pool)
        if (pm->d.st == job.prev_st) d.prev = (short)pm->tab_idx;
    d.parity = (unsigned char)par;
    d.det_in = (unsigned char)(job.det_in - c->det);
    d.det_out = (unsigned char)(job.det_out - c->det);
    // detection masks: the lane's static mask as it is at this push (rebvio_hip_set_detection_mask waits for the steps queued
    // before it), and this step's per-frame mask
    masks.stat[l] = job.mask_static;
    masks.frame[l] = job.mask_frame;
    masked = masked || job.mask_static || job.mask_frame;
  }
  rebvio_hip_batch::DetStep job;
  job.dyn = dyn;
  job.par = par;
  job.step = b->step;
  // maps are released in lane order at one point of the track stream: the last lane's event covers all of them
  job.reuse_done = (last_reused && last_reused->has_done) ? (last_reused->done_ref ? last_reused->done_ref : last_reused->done) : nullptr;
  job.maps = fr.m;
  job.lens = b->lens;
  job.fmt = fmt;
  job.masked = masked;
  job.masks = masks;
  for (auto* m : fr.m) m->enqueued.store(0, std::memory_order_relaxed);
  if (!b->det_thread.joinable()) b->det_thread = std::thread(batch_det_worker, b);
  {
    std::lock_guard<std::mutex> lk(b->det_mu);
    b->det_jobs.push_back(job);
  }
  b->det_cv.notify_one();
  b->frames.push_back(fr);
  b->step++;

  // ---- track stage: the step's pairs, whole, for every lane; then whatever records have become complete ----
  const int nsteps = group_size((int)b->frames.size(), b->q.count, b->lead, b->group);
  if (nsteps >= 1) {
    const auto t0 = std::chrono::steady_clock::now();
    const double w0 = b->q.t_wait;
    const int rc = batch_enqueue_group(b, nsteps);
    b->t_trk_enq += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() - (b->q.t_wait - w0);
    if (rc) {
      b->poisoned = true;
      return rc;
    }
  }
  int rc = harvest(b->q, batch_lanes(b), 0);
  if (rc) return rc;
  (void)pop_records(b->q, b->B, out, keylines);
  return 0;
}

int rebvio_hip_batch_push_u8_device(rebvio_hip_batch* b, const uint8_t* const* frames_dev, uint64_t ts_us, rebvio_hip_pair_out* out,
                                    int* keylines) {
  return batch_push(b, reinterpret_cast<const void* const*>(frames_dev), px::GRAY8, ts_us, out, keylines);
}

int rebvio_hip_batch_push_px_device(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, uint64_t ts_us, rebvio_hip_pair_out* out,
                                    int* keylines) {
  if (!frames_dev) return fail_msg("batch_push_px_device: null frame array", -3);
  for (int l = 0; l < b->B; ++l) {
    const int rc = check_px(b->lane[l], "batch_push_px_device", frames_dev[l], fmt, false, 0);
    if (rc) return rc;
  }
  return batch_push(b, frames_dev, fmt, ts_us, out, keylines);
}

int rebvio_hip_batch_push_px_masked_device(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, const uint8_t* const* masks_dev,
                                           uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines) {
  if (!frames_dev) return fail_msg("batch_push_px_masked_device: null frame array", -3);
  if (!masks_dev) return fail_msg("batch_push_px_masked_device: null mask array", -3);
  for (int l = 0; l < b->B; ++l) {
    const int rc = check_px(b->lane[l], "batch_push_px_masked_device", frames_dev[l], fmt, false, 0);
    if (rc) return rc;
  }
  return batch_push(b, frames_dev, fmt, ts_us, out, keylines, masks_dev);
}

int rebvio_hip_batch_push_px_gyro_device(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, const uint8_t* const* masks_dev,
                                         const float* const* R_gyro, uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines) {
  if (!frames_dev) return fail_msg("batch_push_px_gyro_device: null frame array", -3);
  for (int l = 0; l < b->B; ++l) {
    int rc = check_px(b->lane[l], "batch_push_px_gyro_device", frames_dev[l], fmt, false, 0);
    if (rc == 0 && R_gyro) rc = check_gyro(b->lane[l], "batch_push_px_gyro_device", R_gyro[l]);
    if (rc) return rc;
  }
  return batch_push(b, frames_dev, fmt, ts_us, out, keylines, masks_dev, R_gyro);
}

// Static detection mask of a context (a batch lane's included). The candidate kernels of the frames queued so far read the old
// mask from the same buffer: a batch lane first waits until its batch's detect worker has launched every queued step, then the
// keyline stream (where the candidate kernels run) is drained before the buffer is rewritten. Clearing needs neither: frames
// queued from here on do not read the buffer, frames queued before it still find their mask there.
int rebvio_hip_set_detection_mask(rebvio_hip_ctx* c, const uint8_t* mask, size_t pitch_bytes) {
  const size_t rows = (size_t)c->P.rows, cols = (size_t)c->P.cols;
  if (!mask) {
    c->dmask = nullptr;
    return 0;
  }
  if (pitch_bytes != 0 && pitch_bytes < cols) {
    char buf[128];
    std::snprintf(buf, sizeof(buf), "set_detection_mask: pitch_bytes %zu below cols %zu", pitch_bytes, cols);
    return fail_msg(buf, -3);
  }
  HIPCHK(hipSetDevice(c->device));
  if (rebvio_hip_batch* b = c->batch)
    while (b->det_done_steps.load(std::memory_order_acquire) < b->step) std::this_thread::yield();
  HIPCHK(hipStreamSynchronize(c->s_key));
  if (!c->dmask_buf) HIPCHK(c->own.device(&c->dmask_buf, rows * cols));
  HIPCHK(hipMemcpy2D(c->dmask_buf, cols, mask, pitch_bytes ? pitch_bytes : cols, cols, rows, hipMemcpyHostToDevice));
  c->dmask = c->dmask_buf;
  return 0;
}

int rebvio_hip_batch_next_records(rebvio_hip_batch* b, rebvio_hip_pair_out* out, int* keylines) { return pop_records(b->q, b->B, out, keylines); }

int rebvio_hip_batch_flush(rebvio_hip_batch* b) {
  HIPCHK(hipSetDevice(b->device));
  while (b->det_done_steps.load(std::memory_order_acquire) < b->step) std::this_thread::yield();
  if (b->dbg && b->step)
    std::fprintf(stderr, "[rebvio_hip] batch of %d lanes, host time per step (us): detect worker's launches %.1f  track enqueue %.1f  waiting "
                 "for result slots %.1f\n", b->B, (double)b->t_det_ns.load() / 1e3 / (double)b->step, b->t_trk_enq / (double)b->step,
                 b->q.t_wait / (double)b->step);
  if (b->dbg)
    std::fprintf(stderr, "[rebvio_hip] batch: pool of lane 0 holds %d maps (min_pool %d), %d steps in flight, %d detected steps queued\n",
                 (int)b->lane[0]->pool.size(), b->lane[0]->min_pool, b->q.count, (int)b->frames.size());
  int rc = 0;
  while (rc == 0 && b->frames.size() >= 2)  // the steps no group was started for yet
    rc = batch_enqueue_group(b, std::min(b->group, (int)b->frames.size() - 1));
  if (rc == 0) rc = drain(b->q, batch_lanes(b));
  for (auto& f : b->frames)
    for (size_t l = 0; l < f.m.size(); ++l) release_map(f.m[l], nullptr, l + 1 == f.m.size());
  b->frames.clear();
  for (auto* c : b->lane)  // as rebvio_hip_flush: no histogram counts of a pair that will not come
    HIPCHK(hipMemsetAsync(c->hist, 0, 128 * sizeof(int), b->st.s_trk));
  HIPCHK(hipStreamSynchronize(b->st.s_det));
  HIPCHK(hipStreamSynchronize(b->st.s_key));
  HIPCHK(hipStreamSynchronize(b->st.s_trk));
  return rc;
}

}  // extern "C"
