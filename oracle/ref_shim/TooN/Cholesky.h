// Stand-in for <TooN/Cholesky.h> (TEST INFRASTRUCTURE, see TooN/TooN.h). TooN documents Cholesky<N> as the square-root-free
// decomposition A = L D L^T of a symmetric matrix, computed column by column in one square array (the unit-lower L below the
// diagonal, D on it), and get_inverse() as the back-substitution of the identity, column by column: forward through L, the
// division by D, backward through L^T. Only Core's inertial glue calls it. What is computed here is compared since
// Core::gyroBiasCorrection is (tests/test_reference_pin.py, tests/test_reference_pin_gpu.py): the oracle's, the host's and the
// device's 6x6 inverse have to give the floats of get_inverse() below. That pins them to THIS reading of TooN's Cholesky, which
// the reference library shares with them - not to TooN's own file, which is not here to be compiled.
#ifndef REBVIO_REF_SHIM_TOON_CHOLESKY_H_
#define REBVIO_REF_SHIM_TOON_CHOLESKY_H_

#include <TooN/TooN.h>

namespace TooN {

template <int N, class P = double>
class Cholesky {
 public:
  template <int R, int C, class Q, bool B>
  Cholesky(const Matrix<R, C, Q, B>& m) : a_(m) {
    for (int col = 0; col < N; ++col) {
      P inv_diag = 1;
      for (int row = col; row < N; ++row) {
        P val = a_(row, col);
        for (int k = 0; k < col; ++k) val -= a_(k, col) * a_(row, k);   // a_(k, col), k < col: D[k] * L(col, k)
        if (row == col) {
          a_(row, col) = val;
          if (val == 0) break;
          inv_diag = P(1) / val;
        } else {
          a_(col, row) = val;
          a_(row, col) = val * inv_diag;
        }
      }
    }
  }
  Matrix<N, N, P> get_inverse() const {
    Matrix<N, N, P> inv;
    for (int c = 0; c < N; ++c) {
      P y[N], x[N];
      for (int i = 0; i < N; ++i) {
        P val = (i == c) ? P(1) : P(0);
        for (int j = 0; j < i; ++j) val -= a_(i, j) * y[j];
        y[i] = val;
      }
      for (int i = 0; i < N; ++i) y[i] /= a_(i, i);
      for (int i = N - 1; i >= 0; --i) {
        P val = y[i];
        for (int j = i + 1; j < N; ++j) val -= a_(j, i) * x[j];
        x[i] = val;
      }
      for (int i = 0; i < N; ++i) inv(i, c) = x[i];
    }
    return inv;
  }

 private:
  Matrix<N, N, P> a_;
};

}  // namespace TooN
#endif
