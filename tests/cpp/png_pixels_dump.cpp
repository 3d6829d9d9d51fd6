// rebvio::io::readPngPixels for tests/test_pixel_formats.py:  png_pixels_dump file.png out.bin [opencv]
// out.bin = int32 {format, rows, cols, cv type} followed by the rows' bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>

#include "rebvio/io/stream_io.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  try {
    const rebvio::io::PngPixels p = rebvio::io::readPngPixels(argv[1], argc > 3 && !std::strcmp(argv[3], "opencv"));
    const int t = p.data.type();
    const size_t ch = t == CV_8UC3 ? 3 : t == CV_8UC4 ? 4 : 1;
    const int32_t hdr[4] = {p.format, p.data.rows, p.data.cols, t};
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    std::fwrite(hdr, sizeof(hdr), 1, f);
    for (int r = 0; r < p.data.rows; ++r) std::fwrite(p.data.ptr<unsigned char>(r), 1, (size_t)p.data.cols * ch, f);
    std::fclose(f);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
