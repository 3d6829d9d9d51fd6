// Stand-in for <opencv2/core.hpp> (TEST INFRASTRUCTURE): the part of cv::Mat the reference's hot-path sources use, written
// from OpenCV's documented interface. A Mat is a reference-counted dense 2-D array: copies and assignments share the
// pixels, Mat(rows, cols, type) allocates them uninitialised and continuous, Mat(rows, cols, type, Scalar) sets every
// element to the scalar's first value, ptr<T>(row) is the row's first element, at<T>(row, col) one element and at<T>(i)
// the i-th element of a continuous matrix in row-major order. No arithmetic happens here.
#ifndef REBVIO_REF_SHIM_OPENCV_CORE_HPP_
#define REBVIO_REF_SHIM_OPENCV_CORE_HPP_

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>

#define CV_8UC1 0
#define CV_32SC1 4
#define CV_32FC1 5
#define CV_64FC1 6

namespace cv {

struct Scalar {
  double val[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) : val{a, b, c, d} {}
};

class Mat {
 public:
  int rows = 0, cols = 0;
  unsigned char* data = nullptr;
  size_t step = 0;

  Mat() = default;
  Mat(int r, int c, int type) { create(r, c, type); }
  Mat(int r, int c, int type, const Scalar& s) {
    create(r, c, type);
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < c; ++j) switch (type) {
          case CV_8UC1: at<unsigned char>(i, j) = (unsigned char)s.val[0]; break;
          case CV_32SC1: at<int>(i, j) = (int)s.val[0]; break;
          case CV_32FC1: at<float>(i, j) = (float)s.val[0]; break;
          default: at<double>(i, j) = s.val[0];
        }
  }
  void create(int r, int c, int type) {
    rows = r; cols = c; type_ = type;
    step = (size_t)c * elem_size(type);
    store_ = std::shared_ptr<unsigned char>(new unsigned char[step * (size_t)r], std::default_delete<unsigned char[]>());
    data = store_.get();
  }
  int type() const { return type_; }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data + (size_t)r * step); }
  template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data + (size_t)r * step); }
  template <class T> T& at(int r, int c) { return ptr<T>(r)[c]; }
  template <class T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }
  template <class T> T& at(int i) { return ptr<T>(0)[i]; }
  template <class T> const T& at(int i) const { return ptr<T>(0)[i]; }
  Mat clone() const {
    Mat out(rows, cols, type_);
    if (!empty()) std::memcpy(out.data, data, step * (size_t)rows);
    return out;
  }

 private:
  static size_t elem_size(int type) { return type == CV_8UC1 ? 1 : type == CV_64FC1 ? 8 : 4; }
  int type_ = CV_8UC1;
  std::shared_ptr<unsigned char> store_;
};

namespace detail {
template <class T> struct TypeOf;
template <> struct TypeOf<unsigned char> { static const int value = CV_8UC1; };
template <> struct TypeOf<int> { static const int value = CV_32SC1; };
template <> struct TypeOf<float> { static const int value = CV_32FC1; };
template <> struct TypeOf<double> { static const int value = CV_64FC1; };
}  // namespace detail

template <class T>
class Mat_ : public Mat {
 public:
  Mat_() = default;
  Mat_(int r, int c) : Mat(r, c, detail::TypeOf<T>::value) {}
};

// (Mat_<T>(r, c) << a, b, c, ...): the values in row-major order, each converted to T
template <class T>
class MatCommaInitializer_ {
 public:
  MatCommaInitializer_(const Mat_<T>& m) : m_(m), i_(0) {}
  template <class V>
  MatCommaInitializer_& operator,(V v) {
    assert(i_ < m_.rows * m_.cols);
    m_.template at<T>(i_++) = static_cast<T>(v);
    return *this;
  }
  operator Mat_<T>() const { return m_; }
  operator Mat() const { return m_; }

 private:
  Mat_<T> m_;
  int i_;
};
template <class T, class V>
MatCommaInitializer_<T> operator<<(const Mat_<T>& m, V v) {
  MatCommaInitializer_<T> init(m);
  return (init, v);
}

}  // namespace cv
#endif
