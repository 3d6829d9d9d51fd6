// Stand-in for <TooN/so3.h> (TEST INFRASTRUCTURE, see TooN/TooN.h). The reference's hot-path sources only need the type to
// exist (types/imu.hpp integrates gyro samples with it; no test reaches that code through oracle/_ref): the exponential is
// Rodrigues' formula, R = I + A K + B K^2 with A = sin(t)/t, B = (1 - cos(t))/t^2 and their Taylor series for small t.
#ifndef REBVIO_REF_SHIM_TOON_SO3_H_
#define REBVIO_REF_SHIM_TOON_SO3_H_

#include <TooN/TooN.h>

namespace TooN {

template <class P = double>
class SO3 {
 public:
  SO3() : R_(Identity) {}
  template <int N, class Q, bool B>
  SO3(const Vector<N, Q, B>& w_) {
    const Vector<3, P> w(w_);
    const P tsq = w * w;
    P A, B2;
    if (tsq < P(1e-8)) {
      A = P(1) - tsq / P(6);
      B2 = P(0.5);
    } else if (tsq < P(1e-6)) {
      B2 = P(0.5) - tsq / P(24);
      A = P(1) - tsq / P(6) * (P(1) - tsq / P(20));
    } else {
      const P t = std::sqrt(tsq);
      A = std::sin(t) / t;
      B2 = (P(1) - std::cos(t)) / tsq;
    }
    R_(0, 0) = P(1) - B2 * (w[1] * w[1] + w[2] * w[2]);
    R_(1, 1) = P(1) - B2 * (w[0] * w[0] + w[2] * w[2]);
    R_(2, 2) = P(1) - B2 * (w[0] * w[0] + w[1] * w[1]);
    R_(0, 1) = B2 * (w[0] * w[1]) - A * w[2];
    R_(1, 0) = B2 * (w[0] * w[1]) + A * w[2];
    R_(0, 2) = B2 * (w[0] * w[2]) + A * w[1];
    R_(2, 0) = B2 * (w[0] * w[2]) - A * w[1];
    R_(1, 2) = B2 * (w[1] * w[2]) - A * w[0];
    R_(2, 1) = B2 * (w[1] * w[2]) + A * w[0];
  }
  const Matrix<3, 3, P>& get_matrix() const { return R_; }
  template <int N, class Q, bool B>
  Vector<3, typename Internal::Mul<P, Q>::type> operator*(const Vector<N, Q, B>& v) const { return R_ * v; }

 private:
  Matrix<3, 3, P> R_;
};

}  // namespace TooN
#endif
