// Stand-in for <opencv2/imgproc.hpp> (TEST INFRASTRUCTURE): rebvio/camera.hpp names cv::undistort in an inline member that
// nothing in oracle/_ref calls. It exists so that the header compiles; calling it ends the process.
#ifndef REBVIO_REF_SHIM_OPENCV_IMGPROC_HPP_
#define REBVIO_REF_SHIM_OPENCV_IMGPROC_HPP_

#include <opencv2/core.hpp>

#include <cstdio>
#include <cstdlib>

namespace cv {
inline void undistort(const Mat&, Mat&, const Mat&, const Mat&) {
  std::fputs("oracle/ref_shim: cv::undistort is not provided\n", stderr);
  std::abort();
}
}  // namespace cv
#endif
