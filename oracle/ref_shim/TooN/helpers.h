// Stand-in for <TooN/helpers.h> (TEST INFRASTRUCTURE, see TooN/TooN.h): determinant, max_element, isnan, normalize.
#ifndef REBVIO_REF_SHIM_TOON_HELPERS_H_
#define REBVIO_REF_SHIM_TOON_HELPERS_H_

#include <TooN/TooN.h>

namespace TooN {

// R7: 2x2 in closed form; larger matrices by Gaussian elimination with partial pivoting: per column the row of largest
// magnitude is swapped up (one sign change), the determinant is multiplied by the pivot, and the rows below are reduced by
// (row[i] / pivot) times the pivot row, left to right.
template <int R, int C, class P, bool B>
P determinant(const Matrix<R, C, P, B>& m) {
  const int n = m.num_rows();
  assert(n == m.num_cols());
  if (n == 2) return m(0, 0) * m(1, 1) - m(1, 0) * m(0, 1);
  Matrix<Dynamic, Dynamic, P> a(m);
  P det = 1;
  for (int i = 0; i < n; ++i) {
    int best = i;
    P big = std::abs(a(i, i));
    for (int r = i + 1; r < n; ++r)
      if (std::abs(a(r, i)) > big) {
        big = std::abs(a(r, i));
        best = r;
      }
    const P pivot = a(best, i);
    if (best != i) {
      det *= -1;
      for (int c = i; c < n; ++c) std::swap(a(i, c), a(best, c));
    }
    det *= a(i, i);
    if (det == 0) return 0;
    for (int r = i + 1; r < n; ++r) {
      const P factor = a(r, i) / pivot;
      for (int c = i; c < n; ++c) a(r, c) = a(r, c) - factor * a(i, c);
    }
  }
  return det;
}

// the largest element and its (row, column), the first one found scanning row by row
template <int R, int C, class P, bool B>
std::pair<P, std::pair<int, int> > max_element(const Matrix<R, C, P, B>& m) {
  std::pair<P, std::pair<int, int> > best(m(0, 0), std::pair<int, int>(0, 0));
  for (int i = 0; i < m.num_rows(); ++i)
    for (int j = 0; j < m.num_cols(); ++j)
      if (m(i, j) > best.first) best = std::make_pair(m(i, j), std::make_pair(i, j));
  return best;
}

template <int N, class P, bool B>
bool isnan(const Vector<N, P, B>& v) {
  for (int i = 0; i < v.size(); ++i)
    if (std::isnan(v[i])) return true;
  return false;
}
template <int R, int C, class P, bool B>
bool isnan(const Matrix<R, C, P, B>& m) {
  for (int i = 0; i < m.num_rows(); ++i)
    for (int j = 0; j < m.num_cols(); ++j)
      if (std::isnan(m(i, j))) return true;
  return false;
}

// v /= sqrt(v * v)
template <int N, class P, bool B>
void normalize(Vector<N, P, B>& v) {
  v /= std::sqrt(v * v);
}

}  // namespace TooN
#endif
