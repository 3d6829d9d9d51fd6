// The PLY writer of rebvio::io (no GPU): a cloud written by writePointCloudPly comes back from readPointCloudPly bit for bit,
// the file is what the header says (text header, then 16 little-endian bytes per vertex), an empty cloud is a valid file, and
// files of another shape are refused.
//   test_point_cloud_ply <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "rebvio/io/stream_io.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  using rebvio::types::CloudPoint;
  std::vector<CloudPoint> pts(1000);
  unsigned s = 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(int)(s >> 8) / 65536.0f - 128.0f;
  };
  for (size_t i = 0; i < pts.size(); ++i) {
    pts[i] = CloudPoint{{rnd(), rnd(), rnd()}, 0.5f, 0.1f, std::fabs(rnd()), (int)(3 * i), 4u};
  }
  pts[7].xyz[1] = -0.0f;
  pts[8].xyz[2] = std::numeric_limits<float>::denorm_min();
  pts[9].xyz[0] = 1.0e30f;
  const std::string path = dir + "/cloud.ply";
  rebvio::io::writePointCloudPly(path, pts.data(), pts.size(), 1403636579763555ull);
  uint64_t ts = 0;
  const std::vector<rebvio::io::PlyVertex> back = rebvio::io::readPointCloudPly(path, &ts);
  CHECK(ts == 1403636579763555ull);
  CHECK(back.size() == pts.size());
  for (size_t i = 0; i < back.size() && i < pts.size(); ++i)
    CHECK(same_bits(back[i].x, pts[i].xyz[0]) && same_bits(back[i].y, pts[i].xyz[1]) && same_bits(back[i].z, pts[i].xyz[2]) &&
          same_bits(back[i].intensity, pts[i].gradient_norm));
  // the file itself: header text, then exactly 16 bytes per vertex, little-endian
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string file = ss.str();
  const std::string header =
      "ply\nformat binary_little_endian 1.0\ncomment rebvio point cloud ts_us 1403636579763555\nelement vertex 1000\n"
      "property float x\nproperty float y\nproperty float z\nproperty float intensity\nend_header\n";
  CHECK(file.compare(0, header.size(), header) == 0);
  CHECK(file.size() == header.size() + 16 * pts.size());
  if (file.size() == header.size() + 16 * pts.size()) {
    const float one = 1.0f;  // 0x3f800000: bytes 00 00 80 3f
    pts[0].xyz[0] = one;
    rebvio::io::writePointCloudPly(path, pts.data(), 1, 5);
    std::ifstream g(path, std::ios::binary);
    std::stringstream s2;
    s2 << g.rdbuf();
    const std::string one_file = s2.str();
    const size_t at = one_file.find("end_header\n") + 11;
    CHECK(one_file.size() == at + 16);
    CHECK((unsigned char)one_file[at] == 0x00 && (unsigned char)one_file[at + 1] == 0x00 && (unsigned char)one_file[at + 2] == 0x80 &&
          (unsigned char)one_file[at + 3] == 0x3f);
  }
  // an empty cloud
  rebvio::io::writePointCloudPly(dir + "/empty.ply", nullptr, 0, 7);
  CHECK(rebvio::io::readPointCloudPly(dir + "/empty.ply", &ts).empty() && ts == 7);
  // refused: a truncated file, trailing bytes, another header
  auto refused = [&](const std::string& content) {
    const std::string p = dir + "/bad.ply";
    std::ofstream o(p, std::ios::binary);
    o << content;
    o.close();
    try {
      rebvio::io::readPointCloudPly(p);
    } catch (const std::runtime_error&) {
      return true;
    }
    return false;
  };
  CHECK(refused(file.substr(0, file.size() - 1)));
  CHECK(refused(file + "x"));
  CHECK(refused("ply\nformat ascii 1.0\nelement vertex 0\nend_header\n"));
  bool threw = false;
  try {
    rebvio::io::writePointCloudPly(dir + "/no/such/dir/cloud.ply", pts.data(), 1, 0);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  if (fails == 0) std::printf("ok\n");
  return fails ? 1 : 0;
}
