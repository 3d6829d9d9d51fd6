#include "rebvio/edge_detector.hpp"

#include "session.hpp"

namespace rebvio {

EdgeDetector::EdgeDetector(rebvio::Camera::SharedPtr camera, rebvio::EdgeDetectorConfig::SharedPtr config)
    : config_(config), camera_(camera), session_(backend::Session::forCamera(*camera)) {
  session_->setDetectorConfig(*config_);
}

EdgeDetector::~EdgeDetector() {}

rebvio::EdgeMap::SharedPtr EdgeDetector::detect(rebvio::types::Image& image) {
  rebvio_hip_ctx* ctx = session_->ctx();
  if (image.data.rows != (int)camera_->rows_ || image.data.cols != (int)camera_->cols_)
    backend::fail("EdgeDetector::detect: image must have the camera's size", -1);
  rebvio_hip_map* h = nullptr;
  if (image.data.type() == CV_8UC1) {
    // raw MONO8 frame: convertTo(CV_32F, 3.0) and undistort run on the device in front of the scale space
    backend::check("rebvio_hip_detect_u8", rebvio_hip_detect_u8(ctx, image.data.ptr<unsigned char>(0), image.data.step, image.ts_us, &h));
  } else if (image.data.type() == CV_8UC3 || image.data.type() == CV_8UC4) {
    // colour frame in OpenCV's channel order: the device forms the grey byte (cv::cvtColor BGR2GRAY weights) in front of x3
    const int fmt = image.data.type() == CV_8UC3 ? REBVIO_HIP_PX_BGR8 : REBVIO_HIP_PX_BGRA8;
    backend::check("rebvio_hip_detect_px", rebvio_hip_detect_px(ctx, image.data.ptr<unsigned char>(0), image.data.step, fmt, image.ts_us, &h));
  } else if (image.data.type() == CV_32FC1) {
    // the reference's contract: an already converted and undistorted fp32 frame (rebvio.cpp:43-47)
    backend::check("rebvio_hip_detect", rebvio_hip_detect(ctx, image.data.ptr<float>(0), image.data.step, image.ts_us, &h));
  } else {
    backend::fail("EdgeDetector::detect: image must be CV_8UC1, CV_8UC3 (BGR), CV_8UC4 (BGRA) or CV_32FC1", -1);
  }
  auto map = std::make_shared<rebvio::EdgeMap>(camera_, config_->keylines_max, image.ts_us);
  map->attach(ctx, h, session_);
  return map;
}

void EdgeDetector::setDetectionMask(const cv::Mat& mask) {
  rebvio_hip_ctx* ctx = session_->ctx();
  if (mask.empty()) {
    backend::check("rebvio_hip_set_detection_mask", rebvio_hip_set_detection_mask(ctx, nullptr, 0));
    return;
  }
  if (mask.type() != CV_8UC1 || mask.rows != (int)camera_->rows_ || mask.cols != (int)camera_->cols_)
    backend::fail("EdgeDetector::setDetectionMask: the mask must be CV_8UC1 of the camera's size", -1);
  backend::check("rebvio_hip_set_detection_mask", rebvio_hip_set_detection_mask(ctx, mask.ptr<unsigned char>(0), mask.step));
}

}  // namespace rebvio
