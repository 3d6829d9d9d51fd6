// Camera pixel formats the detector takes, and the grey byte of one pixel. Shared by the device front end (detect.hip), the
// C-ABI's argument checks (api.hip) and the host library (stream_io.cpp, rebvio.cpp): one statement of the conversion.
// The codes are the REBVIO_HIP_PX_* values of include/rebvio_hip.h.
//   GRAY8          1 byte   the byte
//   RGB8 / BGR8    3 bytes  (R*4899 + G*9617 + B*1868 + 8192) >> 14, the fixed-point weights of cv::cvtColor(RGB2GRAY)
//   RGBA8 / BGRA8  4 bytes  as RGB8 / BGR8, alpha ignored
//   YUYV           2 bytes  Y (bytes Y0 U Y1 V; cv::COLOR_YUV2GRAY_YUY2)
//   UYVY           2 bytes  Y (bytes U Y0 V Y1; ROS "yuv422", cv::COLOR_YUV2GRAY_UYVY)
// The packed YUV formats carry two pixels in four bytes: frames of these formats have an even width.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RH_PX_FN __host__ __device__ __forceinline__
#else
#define RH_PX_FN inline
#endif

namespace rh {
namespace px {

enum : int { GRAY8 = 0, RGB8 = 1, BGR8 = 2, RGBA8 = 3, BGRA8 = 4, YUYV = 5, UYVY = 6, kCount = 7 };

RH_PX_FN constexpr bool valid(int fmt) { return fmt >= 0 && fmt < kCount; }
RH_PX_FN constexpr int bytes_per_pixel(int fmt) {
  return fmt == GRAY8 ? 1 : (fmt == RGB8 || fmt == BGR8) ? 3 : (fmt == RGBA8 || fmt == BGRA8) ? 4 : (fmt == YUYV || fmt == UYVY) ? 2 : 0;
}
// packed YUV: a 4-byte group holds two pixels
RH_PX_FN constexpr bool needs_even_cols(int fmt) { return fmt == YUYV || fmt == UYVY; }

RH_PX_FN constexpr uint8_t luma(uint32_t r, uint32_t g, uint32_t b) { return (uint8_t)((r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14); }

// Grey byte of pixel x of a dense row (row[] = the row's first byte). For YUYV / UYVY pixel x's Y is byte 2x (+1 for UYVY).
template <int FMT>
RH_PX_FN uint8_t grey_at(const uint8_t* row, int x) {
  if (FMT == GRAY8) return row[x];
  if (FMT == RGB8) return luma(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
  if (FMT == BGR8) return luma(row[3 * x + 2], row[3 * x + 1], row[3 * x]);
  if (FMT == RGBA8) return luma(row[4 * x], row[4 * x + 1], row[4 * x + 2]);
  if (FMT == BGRA8) return luma(row[4 * x + 2], row[4 * x + 1], row[4 * x]);
  if (FMT == YUYV) return row[2 * x];
  return row[2 * x + 1];  // UYVY
}

// host form: the grey byte of pixel x with the format as a run-time value (fmt must be valid)
inline uint8_t grey_at(int fmt, const uint8_t* row, int x) {
  switch (fmt) {
    case RGB8: return grey_at<RGB8>(row, x);
    case BGR8: return grey_at<BGR8>(row, x);
    case RGBA8: return grey_at<RGBA8>(row, x);
    case BGRA8: return grey_at<BGRA8>(row, x);
    case YUYV: return grey_at<YUYV>(row, x);
    case UYVY: return grey_at<UYVY>(row, x);
    default: return row[x];
  }
}

// host: a whole frame to GRAY8 (rows of `pitch` bytes in, dense rows of `cols` bytes out)
inline void to_grey(int fmt, const void* src, size_t pitch, int rows, int cols, uint8_t* dst) {
  for (int r = 0; r < rows; ++r) {
    const uint8_t* row = static_cast<const uint8_t*>(src) + (size_t)r * pitch;
    uint8_t* o = dst + (size_t)r * cols;
    for (int x = 0; x < cols; ++x) o[x] = grey_at(fmt, row, x);
  }
}

}  // namespace px
}  // namespace rh

#undef RH_PX_FN
