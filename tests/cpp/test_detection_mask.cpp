// rebvio::Rebvio with a detection mask, for tests/test_detection_mask_gpu.py:
//   test_detection_mask none|ones|half frames.u8 W H N fm cx cy imu.bin
// frames.u8: N MONO8 frames of W*H bytes. ones: an all-255 mask; half: only the top H/2 rows may hold keylines. The mask is set
// before the first frame. Prints the odometry records ("%.9g": every float bit for bit). Every published edge map is checked:
// with the half mask no keyline may lie below row H/2 - 1 + 0.5 (a keyline sits within half a pixel of its pixel). Exit 3 when
// one does, 1 when records or edge maps are missing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <vector>

#include "rebvio/rebvio.hpp"

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const std::string mode = argv[1];
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  const size_t fb = (size_t)W * H;
  std::vector<unsigned char> buf(fb * N);
  std::ifstream f(argv[2], std::ios::binary);
  if (!f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size())) return 2;
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(H, W, std::atof(argv[6]), std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]));
  config.edge_detector.keylines_ref = 3000;
  config.edge_detector.keylines_max = 4000;
  config.core.global_min_matches_threshold = 50;
  std::vector<std::vector<char>> imu;
  {
    std::ifstream fi(argv[9], std::ios::binary);
    std::vector<char> rec(32);
    while (fi.read(rec.data(), 32)) imu.push_back(rec);
  }
  rebvio::Rebvio rebvio(config);
  if (mode != "none") {
    cv::Mat mask(H, W, CV_8UC1);
    for (int r = 0; r < H; ++r) std::memset(mask.ptr<unsigned char>(r), (mode == "ones" || r < H / 2) ? 255 : 0, (size_t)W);
    rebvio.setDetectionMask(mask);
  }
  std::mutex mu;
  int n_odo = 0, n_edge = 0, bad = 0;
  long total = 0;
  const float y_max = (float)(H / 2 - 1) + 0.5f;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    std::printf("%llu %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", (unsigned long long)o.ts_us, o.orientation[0],
                o.orientation[1], o.orientation[2], o.position[0], o.position[1], o.position[2], o.scale, o.gyro_bias[0], o.gyro_bias[1],
                o.gyro_bias[2], o.klm_num);
    ++n_odo;
  });
  rebvio.registerEdgeImageCallback([&](cv::Mat& img, rebvio::EdgeMap::SharedPtr& map) {
    (void)img;
    const std::vector<rebvio::types::KeyLine>& kl = map->keylines();
    std::lock_guard<std::mutex> g(mu);
    for (const auto& k : kl)
      if (mode == "half" && k.pos[1] > y_max) ++bad;
    total += (long)kl.size();
    ++n_edge;
  });
  size_t k = 0;
  for (int i = 0; i < N; ++i) {
    const uint64_t ts = (uint64_t)i * 50000;
    for (; k < imu.size(); ++k) {
      long long t;
      float g[3], a[3];
      std::memcpy(&t, imu[k].data(), 8);
      if ((uint64_t)t > ts) break;
      std::memcpy(g, imu[k].data() + 8, 12);
      std::memcpy(a, imu[k].data() + 20, 12);
      rebvio.imuCallback(rebvio::types::Imu{(uint64_t)t, TooN::makeVector(g[0], g[1], g[2]), TooN::makeVector(a[0], a[1], a[2])});
    }
    cv::Mat frame(H, W, CV_8UC1, buf.data() + (size_t)i * fb);
    rebvio.imageCallback(rebvio::types::Image{ts, frame.clone()});
  }
  rebvio.waitIdle();
  std::fprintf(stderr, "frames=%d odometry=%d edge=%d keylines=%ld outside=%d running=%d\n", N, n_odo, n_edge, total, bad,
               (int)rebvio.running());
  if (bad) return 3;
  return (n_odo == N - 1 && n_edge == N && total > 0) ? 0 : 1;
}
