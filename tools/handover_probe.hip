// Micro-probe (diagnostic, not product): what does a stream operation between two dependent kernels of one stream cost - on the
// device (end of a kernel -> start of the next, in-kernel clock stamps) and on the launching thread (time of the call)?
//   plain     nothing between the kernels
//   wait-done a hipStreamWaitEvent on an event of ANOTHER stream that completed long before
//   query     the same event asked with hipEventQuery, nothing queued (what a caller could do instead of such a wait)
//   record    a hipEventRecord between the kernels
//   both      record + wait-done
// Each kernel runs ~20 us so that the host stays ahead and the queue is never empty: the gaps are the command processor's.
// Build: hipcc -O2 --offload-arch=gfx950 tools/handover_probe.hip -o tools/handover_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

__global__ void k_busy(unsigned long long* stamps, int i, unsigned long long ticks) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = wall_clock64();  // 100 MHz
  while (wall_clock64() - t0 < ticks) {}
  stamps[2 * i] = t0;
  stamps[2 * i + 1] = wall_clock64();
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  constexpr int N = 200, kForms = 5;
  static const char* const name[kForms] = {"plain", "wait-done", "query", "record", "both"};
  hipStream_t s, other;
  CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&other, hipStreamNonBlocking));
  unsigned long long* stamps = nullptr;
  CK(hipHostMalloc((void**)&stamps, 2 * N * sizeof(unsigned long long), hipHostMallocDefault));
  hipEvent_t done_long_ago;
  CK(hipEventCreateWithFlags(&done_long_ago, hipEventDisableTiming));
  std::vector<hipEvent_t> ev(N);
  for (auto& e : ev) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipLaunchKernelGGL(k_busy, dim3(1), dim3(64), 0, other, stamps, 0, 100ull);
  CK(hipEventRecord(done_long_ago, other));
  CK(hipStreamSynchronize(other));
  for (int rep = 0; rep < 3; ++rep)
    for (int form = 0; form < kForms; ++form) {
      std::vector<double> host_us;
      int skipped = 0;
      for (int i = 0; i < N; ++i) {
        if (i) {
          const auto t0 = std::chrono::steady_clock::now();
          if (form == 3 || form == 4) CK(hipEventRecord(ev[i], s));
          if (form == 1 || form == 4) CK(hipStreamWaitEvent(s, done_long_ago, 0));
          if (form == 2) skipped += hipEventQuery(done_long_ago) == hipSuccess;
          if (form) host_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        hipLaunchKernelGGL(k_busy, dim3(1), dim3(64), 0, s, stamps, i, 2000ull);
      }
      CK(hipStreamSynchronize(s));
      std::vector<double> gap;
      for (int i = 20; i < N; ++i) gap.push_back((double)(stamps[2 * i] - stamps[2 * i - 1]) * 0.01);
      std::sort(gap.begin(), gap.end());
      std::sort(host_us.begin(), host_us.end());
      std::printf("run %d %-9s device gap between kernels: median %.2f us  min %.2f  p90 %.2f | host time of the call(s): median %.2f us%s\n",
                  rep, name[form], gap[gap.size() / 2], gap.front(), gap[gap.size() * 9 / 10], host_us.empty() ? 0.0 : host_us[host_us.size() / 2],
                  form == 2 ? (skipped == N - 1 ? "  (every query: complete)" : "  (SOME QUERIES NOT COMPLETE)") : "");
    }
  return 0;
}
