// rebvio::Rebvio fed one stream either as MONO8 or as BGR8 colour frames (CV_8UC3, OpenCV's channel order), for
// tests/test_pixel_formats_gpu.py:
//   test_colour_frames gray|bgr frames.bin W H N fm cx cy imu.bin edge_out.bin [k1,k2,p1,p2,k3]
// frames.bin: N frames of W*H (gray) or W*H*3 (bgr) bytes. Prints the odometry records ("%.9g": every float bit for bit);
// edge_out.bin receives every edge-image callback frame: int32 {cv type, rows, cols} + its rows' bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <vector>

#include "rebvio/rebvio.hpp"

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  const bool bgr = !std::strcmp(argv[1], "bgr");
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  const size_t fb = (size_t)W * H * (bgr ? 3 : 1);
  std::vector<unsigned char> buf(fb * N);
  std::ifstream f(argv[2], std::ios::binary);
  if (!f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size())) return 2;
  rebvio::RebvioConfig config;
  config.camera = rebvio::Camera(H, W, std::atof(argv[6]), std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]));
  if (argc > 11) {
    float k[5] = {0, 0, 0, 0, 0};
    if (std::sscanf(argv[11], "%f,%f,%f,%f,%f", &k[0], &k[1], &k[2], &k[3], &k[4]) != 5) return 2;
    config.camera.k1_ = k[0], config.camera.k2_ = k[1], config.camera.p1_ = k[2], config.camera.p2_ = k[3], config.camera.k3_ = k[4];
  }
  config.edge_detector.keylines_ref = 3000;
  config.edge_detector.keylines_max = 4000;
  config.core.global_min_matches_threshold = 50;
  std::vector<std::vector<char>> imu;
  {
    std::ifstream fi(argv[9], std::ios::binary);
    std::vector<char> rec(32);
    while (fi.read(rec.data(), 32)) imu.push_back(rec);
  }
  std::FILE* edge = std::fopen(argv[10], "wb");
  if (!edge) return 2;
  rebvio::Rebvio rebvio(config);
  std::mutex mu;
  int n_odo = 0, n_edge = 0;
  rebvio.registerOdometryCallback([&](rebvio::types::Odometry& o) {
    std::lock_guard<std::mutex> g(mu);
    std::printf("%llu %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", (unsigned long long)o.ts_us, o.orientation[0],
                o.orientation[1], o.orientation[2], o.position[0], o.position[1], o.position[2], o.scale, o.gyro_bias[0], o.gyro_bias[1],
                o.gyro_bias[2], o.klm_num);
    ++n_odo;
  });
  rebvio.registerEdgeImageCallback([&](cv::Mat& img, rebvio::EdgeMap::SharedPtr& map) {
    std::lock_guard<std::mutex> g(mu);
    const int hdr[3] = {img.type(), img.rows, img.cols};
    std::fwrite(hdr, sizeof(hdr), 1, edge);
    const size_t rowb = (size_t)img.cols * (img.type() == CV_8UC1 ? 1 : img.type() == CV_8UC3 ? 3 : 4);
    for (int r = 0; r < img.rows; ++r) std::fwrite(img.ptr<unsigned char>(r), 1, rowb, edge);
    (void)map;
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
    cv::Mat frame(H, W, bgr ? CV_8UC3 : CV_8UC1, buf.data() + (size_t)i * fb);
    rebvio.imageCallback(rebvio::types::Image{ts, frame.clone()});
  }
  rebvio.waitIdle();
  std::fclose(edge);
  std::fprintf(stderr, "frames=%d odometry=%d edge=%d running=%d\n", N, n_odo, n_edge, (int)rebvio.running());
  return (n_odo == N - 1 && n_edge == N) ? 0 : 1;
}
