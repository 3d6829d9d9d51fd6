// hm::undistort_fixed_map as a stand-alone program (CPU, built under sanitizers by tests/test_lens_front_end.py): for every case
// of a file it writes the fixed-point map the device front end gathers through, so that the test can hold it word for word to
// the longdouble statement of tests/lens_cases.py. Cases whose coordinates leave int's range, and NaN / infinite coefficients,
// have to pass the float-to-int conversion without undefined behaviour.
//   lens_map_host_check cases.bin maps.bin
//   cases.bin : n x (int32 cols, int32 rows, float32 fx fy cx cy k1 k2 p1 p2 k3)
//   maps.bin  : n x (rows * cols x (int32 iu, int32 iv))
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hostmath.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int n = 0;
  for (;;) {
    int32_t size[2];
    float k[9];
    if (std::fread(size, sizeof(int32_t), 2, in) != 2) break;
    if (std::fread(k, sizeof(float), 9, in) != 9) return 3;
    const int cols = size[0], rows = size[1];
    if (cols < 1 || rows < 1 || cols > (1 << 14) || rows > (1 << 14)) return 3;
    std::vector<int> map((size_t)2 * rows * cols);
    rh::hm::undistort_fixed_map(rows, cols, k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], map.data());
    if (std::fwrite(map.data(), sizeof(int), map.size(), out) != map.size()) return 4;
    ++n;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 4;
  std::printf("%d maps\nok\n", n);
  return 0;
}
