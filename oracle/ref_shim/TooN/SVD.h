// Stand-in for <TooN/SVD.h> (TEST INFRASTRUCTURE, see TooN/TooN.h) - a stand-in in the full sense: TooN's SVD calls LAPACK's
// gesvd, which is not available. The reference only decomposes symmetric positive semi-definite normal matrices (JtJ), for
// which the singular value decomposition is the eigen-decomposition: found here by cyclic Jacobi rotations in double.
// backsub(b) = sum over the kept eigen-pairs of v (v . b) / lambda; a pair is kept when lambda * condition > the largest
// lambda, with TooN's documented default condition number 1e9. A NaN anywhere in the matrix gives a NaN solution (gesvd
// propagates it). What this computes is NOT what the reference computes with LAPACK to the last bit.
#ifndef REBVIO_REF_SHIM_TOON_SVD_H_
#define REBVIO_REF_SHIM_TOON_SVD_H_

#include <TooN/TooN.h>

#include <limits>

namespace TooN {

template <int Rows = Dynamic, int Cols = Rows, class P = double>
class SVD {
  static_assert(Rows == Cols && Rows > 0, "the stand-in decomposes square, statically sized, symmetric matrices only");
  static const int N = Rows;

 public:
  template <int R, int C, class Q, bool B>
  SVD(const Matrix<R, C, Q, B>& m) : nan_(false) {
    double a[N][N];
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        if (std::isnan(m(i, j))) nan_ = true;
        a[i][j] = ((double)m(i, j) + (double)m(j, i)) / 2;
        v_[i][j] = (i == j);
      }
    for (int sweep = 0; sweep < 64; ++sweep) {
      double off = 0;
      for (int p = 0; p < N; ++p)
        for (int q = p + 1; q < N; ++q) off += a[p][q] * a[p][q];
      if (!(off > 0)) break;
      for (int p = 0; p < N; ++p)
        for (int q = p + 1; q < N; ++q) {
          if (a[p][q] == 0) continue;
          // the rotation that zeroes a[p][q]: tan of the smaller angle
          const double zeta = (a[q][q] - a[p][p]) / (2 * a[p][q]);
          const double t = (zeta < 0 ? -1.0 : 1.0) / (std::abs(zeta) + std::sqrt(1 + zeta * zeta));
          const double c = 1 / std::sqrt(1 + t * t), s = c * t;
          for (int k = 0; k < N; ++k) {  // columns p, q of a and of v
            const double x = a[k][p], y = a[k][q];
            a[k][p] = c * x - s * y;
            a[k][q] = s * x + c * y;
            const double vx = v_[k][p], vy = v_[k][q];
            v_[k][p] = c * vx - s * vy;
            v_[k][q] = s * vx + c * vy;
          }
          for (int k = 0; k < N; ++k) {  // rows p, q of a
            const double x = a[p][k], y = a[q][k];
            a[p][k] = c * x - s * y;
            a[q][k] = s * x + c * y;
          }
        }
    }
    for (int i = 0; i < N; ++i) lambda_[i] = a[i][i];
  }

  template <int M, class Q, bool B>
  Vector<N, P> backsub(const Vector<M, Q, B>& b, const P condition = P(1e9)) const {
    double top = 0;
    for (int k = 0; k < N; ++k) top = std::max(top, std::abs(lambda_[k]));
    double x[N] = {0};
    for (int k = 0; k < N; ++k) {
      if (!(std::abs(lambda_[k]) * (double)condition > top)) continue;
      double dot = 0;
      for (int i = 0; i < N; ++i) dot += v_[i][k] * (double)b[i];
      for (int i = 0; i < N; ++i) x[i] += v_[i][k] * (dot / lambda_[k]);
    }
    Vector<N, P> out;
    for (int i = 0; i < N; ++i) out[i] = nan_ ? std::numeric_limits<P>::quiet_NaN() : (P)x[i];
    return out;
  }

 private:
  double v_[N][N], lambda_[N];
  bool nan_;
};

}  // namespace TooN
#endif
