// Stream sources and sinks around rebvio::Rebvio without ROS: what ros_rebvio's bag player and the
// reference's TESTING odometry logger do (ros_rebvio.cpp:89-126; log.cpp:26-41, rebvio.cpp:279-286), for data on disk.
//   EurocReader      - EuRoC / ASL dataset folder (mav0/cam0/data.csv + data/*.png, mav0/imu0/data.csv)
//   RawReader        - dense MONO8 frames (rows*cols bytes each) + optional IMU records {int64 ts_us, float gyro[3], acc[3]}
//   OdometryWriter   - "ts_us wx wy wz px py pz" lines, %.6f, the format of the reference's regression file
//                      ros_rebvio/test/data/MH_03_medium_test_15s-30s_odometry.txt
//   writePointCloudPly / readPointCloudPly - a point cloud as a binary little-endian PLY file (x, y, z, intensity)
//   replay()         - time-ordered playback into imageCallback / imuCallback
#pragma once

#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "rebvio/types/image.hpp"
#include "rebvio/types/imu.hpp"
#include "rebvio/types/odometry.hpp"
#include "rebvio/types/point_cloud.hpp"
#include "rebvio_hip.h"

namespace rebvio {
namespace io {

// 8-bit grey image from a PNG file (grey 8/16 bit, RGB/RGBA 8 bit -> luma; non-interlaced). Throws std::runtime_error.
cv::Mat readPngGray(const std::string& path);

// The stored pixels of a PNG file, not converted: 8-bit RGB -> CV_8UC3, RGBA -> CV_8UC4, grey -> CV_8UC1 (grey + alpha: the
// grey channel; 16-bit grey: the most significant byte). `format` is the REBVIO_HIP_PX_* code of the bytes. opencv_order swaps
// R and B as cv::imread does (CV_8UC3 / CV_8UC4 in OpenCV's BGR / BGRA order, what rebvio::Rebvio::imageCallback expects).
struct PngPixels {
  cv::Mat data;
  int format = REBVIO_HIP_PX_GRAY8;
};
PngPixels readPngPixels(const std::string& path, bool opencv_order = false);

struct FrameRef {
  uint64_t ts_us;
  std::string path;    // EuRoC: image file; raw: empty
  size_t raw_index;    // raw: frame number
};

class StreamSource {
 public:
  virtual ~StreamSource() {}
  virtual size_t numFrames() const = 0;
  virtual uint64_t frameTs(size_t i) const = 0;
  virtual cv::Mat frame(size_t i) = 0;  // CV_8UC1 (EurocReader with colour: CV_8UC3 / CV_8UC4 for colour PNGs)
  const std::vector<rebvio::types::Imu>& imu() const { return imu_; }

 protected:
  std::vector<rebvio::types::Imu> imu_;  // time ordered
};

class EurocReader : public StreamSource {
 public:
  // `mav0_dir` = the folder holding cam0/ and imu0/; timestamps in the csv files are nanoseconds. colour: RGB(A) PNGs are
  // delivered as they are stored (in OpenCV's BGR(A) order: readPngPixels) for the device to convert, not as luma.
  explicit EurocReader(const std::string& mav0_dir, const std::string& cam = "cam0", const std::string& imu = "imu0",
                       bool colour = false);
  size_t numFrames() const override { return frames_.size(); }
  uint64_t frameTs(size_t i) const override { return frames_[i].ts_us; }
  cv::Mat frame(size_t i) override { return colour_ ? readPngPixels(frames_[i].path, true).data : readPngGray(frames_[i].path); }

 private:
  std::vector<FrameRef> frames_;
  bool colour_;
};

class RawReader : public StreamSource {
 public:
  RawReader(const std::string& frames_file, int rows, int cols, uint64_t first_ts_us, uint64_t frame_dt_us,
            const std::string& imu_file = "");
  size_t numFrames() const override { return n_; }
  uint64_t frameTs(size_t i) const override { return t0_ + (uint64_t)i * dt_; }
  cv::Mat frame(size_t i) override;

 private:
  std::string path_;
  int rows_, cols_;
  size_t n_;
  uint64_t t0_, dt_;
};

class OdometryWriter {
 public:
  explicit OdometryWriter(const std::string& path);
  ~OdometryWriter();
  void write(const rebvio::types::Odometry& o);
  static std::string format(const rebvio::types::Odometry& o);  // one line without the newline

 private:
  std::FILE* f_;
};

// A point cloud as a PLY file, "format binary_little_endian 1.0": one vertex per point with the float properties x, y, z
// (CloudPoint::xyz) and intensity (CloudPoint::gradient_norm), in the cloud's order; ts_us goes into a comment line. What
// MeshLab, CloudCompare, Open3D and PCL read. Throws std::runtime_error when the file cannot be written.
void writePointCloudPly(const std::string& path, const rebvio::types::CloudPoint* points, size_t n, uint64_t ts_us = 0);
// Reads such a file back: x, y, z, intensity per vertex. Accepts what writePointCloudPly writes (four float properties of these
// names in this order), nothing else. Throws std::runtime_error.
struct PlyVertex {
  float x, y, z, intensity;
};
std::vector<PlyVertex> readPointCloudPly(const std::string& path, uint64_t* ts_us = nullptr);
// Polylines (EdgeMap::edgePolylines) as a PLY file of the same format: the cloud's vertex element, one vertex per point in slot
// order, then `element edge` with the int properties vertex1, vertex2 - one edge per consecutive pair of points of a line, and the
// closing edge (last point, first point) of a closed line. Lines that reach past `n` points (a capped extraction) are cut there and
// not closed. Throws std::runtime_error when the file cannot be written.
void writePolylinesPly(const std::string& path, const rebvio::types::CloudPoint* points, size_t n, const rebvio::types::Polyline* lines,
                       size_t n_lines, uint64_t ts_us = 0);
// Reads such a file back: the vertices as readPointCloudPly returns them, and the edges. Accepts what writePolylinesPly writes,
// nothing else (an edge that names a vertex outside the file is refused). Throws std::runtime_error.
struct PlyEdge {
  int vertex1, vertex2;
};
std::vector<PlyVertex> readPolylinesPly(const std::string& path, std::vector<PlyEdge>* edges, uint64_t* ts_us = nullptr);
// Straight segments (EdgeMap::edgeSegments) as a PLY file with the polyline file's elements: two vertices (xyz0, xyz1; intensity =
// the end's sigma_rho) and one edge per depth-valid segment, in order; segments without a valid depth have no 3D end points and are
// left out. The comment line says "rebvio segments". readSegmentsPly accepts what writeSegmentsPly writes, nothing else.
void writeSegmentsPly(const std::string& path, const rebvio::types::LineSegment* segments, size_t n, uint64_t ts_us = 0);
std::vector<PlyVertex> readSegmentsPly(const std::string& path, std::vector<PlyEdge>* edges, uint64_t* ts_us = nullptr);

// Plays frames [first, first+count) in time order: every IMU sample with ts <= the frame's stamp is delivered before the
// frame (a time-ordered bag delivers them that way, ros_rebvio.cpp:108-121). Returns the number of frames delivered.
size_t replay(StreamSource& src, const std::function<void(rebvio::types::Image&&)>& image_cb,
              const std::function<void(rebvio::types::Imu&&)>& imu_cb, size_t first = 0, size_t count = (size_t)-1);

}  // namespace io
}  // namespace rebvio
