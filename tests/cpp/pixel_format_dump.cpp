// Host form of the device's pixel-format conversion (rebvio_amd/csrc/pixel_format.hpp), for tests/test_pixel_formats.py:
//   pixel_format_dump fmt rows cols in.bin out.bin
// in.bin = rows dense rows of cols * bytes-per-pixel bytes; out.bin = the rows * cols grey bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rebvio_amd/csrc/pixel_format.hpp"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int fmt = std::atoi(argv[1]), rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  if (!rh::px::valid(fmt)) return 2;
  const size_t pitch = (size_t)cols * rh::px::bytes_per_pixel(fmt);
  std::vector<unsigned char> in(pitch * rows), out((size_t)rows * cols);
  std::FILE* f = std::fopen(argv[4], "rb");
  if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) return 3;
  std::fclose(f);
  rh::px::to_grey(fmt, in.data(), pitch, rows, cols, out.data());
  f = std::fopen(argv[5], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
  std::fclose(f);
  return 0;
}
