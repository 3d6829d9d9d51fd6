// Stand-in for <TooN/TooN.h> (TEST INFRASTRUCTURE): just enough of TooN's interface to compile the reference's hot-path
// sources for oracle/_ref. Written from TooN's published behaviour (its manual and the documented semantics of each
// operator), not from its text. Each block names the rule it follows; DESIGN.md section 2 lists these rules as what stays
// an ASSUMPTION about TooN's arithmetic.
//
//   R1  storage: a statically sized Vector<N,P> / Matrix<R,C,P> is N (R*C, row-major) values of P and nothing else; a default
//       constructed one is uninitialised. Dynamic sizes own heap storage. slice(), T(), operator[] on a matrix, as_row() and
//       as_col() are views: they alias the object they were taken from and assigning to one writes through.
//   R2  precision: an operation on precisions P1 and P2 works in the type of (P1() * P2()) - C++'s usual promotion - and
//       yields that precision; assignment converts element by element.
//   R3  products: a dot product starts from zero and adds v1[i] * v2[i] in ascending i. Every element of Matrix*Vector and
//       Matrix*Matrix is the dot product of a row of the left with the vector / a column of the right.
//   R4  element-wise operations (+, -, unary -, *scalar, /scalar, and the compound forms) are one operation per element.
//   R5  makeVector(a, b, ...): arguments of one type give that precision, mixed arithmetic types give double.
//   R6  Zeros / Identity / Identity*s / Data(...) / as_diagonal(): fill operators. M + Identity*s adds s to the diagonal and
//       leaves the rest; Identity*s - M negates the rest.
//   R7  determinant (helpers.h): 2x2 in closed form, larger by Gaussian elimination with partial pivoting.
#ifndef REBVIO_REF_SHIM_TOON_H_
#define REBVIO_REF_SHIM_TOON_H_

#include <cassert>
#include <cmath>
#include <cstddef>
#include <iostream>
#include <type_traits>
#include <utility>
#include <vector>

namespace TooN {

static const int Dynamic = -1;

namespace Internal {
template <class P1, class P2>
struct Mul {
  typedef decltype(P1() * P2()) type;  // R2
};
template <class S>
using IfScalar = typename std::enable_if<std::is_arithmetic<S>::value, int>::type;
constexpr int pick(int a, int b) { return a != Dynamic ? a : b; }

// ---- R1: storage -----------------------------------------------------------------------------------------------------
template <int N, class P, bool Ref>
struct VStore {  // owned, static
  P d[N];
  VStore() {}
  explicit VStore(int) {}
  int size() const { return N; }
  P* ptr() const { return const_cast<P*>(d); }
  int stride() const { return 1; }
  void fit(int n) { assert(n == N); (void)n; }
};
template <class P>
struct VStore<Dynamic, P, false> {  // owned, dynamic
  std::vector<P> d;
  VStore() {}
  explicit VStore(int n) : d(n) {}
  int size() const { return (int)d.size(); }
  P* ptr() const { return const_cast<P*>(d.data()); }
  int stride() const { return 1; }
  void fit(int n) { d.resize(n); }
};
template <int N, class P>
struct VStore<N, P, true> {  // view
  P* p;
  int n, s;
  VStore(P* p_, int n_, int s_) : p(p_), n(n_), s(s_) {}
  VStore(const VStore&) = default;
  VStore& operator=(const VStore& o) {  // assigning to a view writes through it
    assert(n == o.n);
    for (int i = 0; i < n; ++i) p[i * s] = o.p[i * o.s];
    return *this;
  }
  int size() const { return n; }
  P* ptr() const { return p; }
  int stride() const { return s; }
  void fit(int n_) { assert(n == n_); (void)n_; }
};

template <int R, int C, class P, bool Ref>
struct MStore {  // owned, static, row-major
  P d[R * C];
  MStore() {}
  MStore(int, int) {}
  int num_rows() const { return R; }
  int num_cols() const { return C; }
  P* ptr() const { return const_cast<P*>(d); }
  int rs() const { return C; }
  int cs() const { return 1; }
  void fit(int r, int c) { assert(r == R && c == C); (void)r; (void)c; }
};
template <int R, int C, class P>
struct MStoreDyn {  // owned, at least one dynamic dimension
  std::vector<P> d;
  int r, c;
  MStoreDyn() : r(R == Dynamic ? 0 : R), c(C == Dynamic ? 0 : C) {}
  MStoreDyn(int r_, int c_) : d((size_t)r_ * c_), r(r_), c(c_) {}
  int num_rows() const { return r; }
  int num_cols() const { return c; }
  P* ptr() const { return const_cast<P*>(d.data()); }
  int rs() const { return c; }
  int cs() const { return 1; }
  void fit(int r_, int c_) {
    r = r_; c = c_;
    d.resize((size_t)r * c);
  }
};
template <int C, class P> struct MStore<Dynamic, C, P, false> : MStoreDyn<Dynamic, C, P> { using MStoreDyn<Dynamic, C, P>::MStoreDyn; };
template <int R, class P> struct MStore<R, Dynamic, P, false> : MStoreDyn<R, Dynamic, P> { using MStoreDyn<R, Dynamic, P>::MStoreDyn; };
template <class P> struct MStore<Dynamic, Dynamic, P, false> : MStoreDyn<Dynamic, Dynamic, P> { using MStoreDyn<Dynamic, Dynamic, P>::MStoreDyn; };
template <int R, int C, class P>
struct MStoreRef {
  P* p;
  int r, c, rs_, cs_;
  MStoreRef(P* p_, int r_, int c_, int rs__, int cs__) : p(p_), r(r_), c(c_), rs_(rs__), cs_(cs__) {}
  MStoreRef(const MStoreRef&) = default;
  MStoreRef& operator=(const MStoreRef& o) {
    assert(r == o.r && c == o.c);
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < c; ++j) p[i * rs_ + j * cs_] = o.p[i * o.rs_ + j * o.cs_];
    return *this;
  }
  int num_rows() const { return r; }
  int num_cols() const { return c; }
  P* ptr() const { return p; }
  int rs() const { return rs_; }
  int cs() const { return cs_; }
  void fit(int r_, int c_) { assert(r == r_ && c == c_); (void)r_; (void)c_; }
};
template <int R, int C, class P> struct MStore<R, C, P, true> : MStoreRef<R, C, P> { using MStoreRef<R, C, P>::MStoreRef; };
template <int C, class P> struct MStore<Dynamic, C, P, true> : MStoreRef<Dynamic, C, P> { using MStoreRef<Dynamic, C, P>::MStoreRef; };
template <int R, class P> struct MStore<R, Dynamic, P, true> : MStoreRef<R, Dynamic, P> { using MStoreRef<R, Dynamic, P>::MStoreRef; };
template <class P> struct MStore<Dynamic, Dynamic, P, true> : MStoreRef<Dynamic, Dynamic, P> { using MStoreRef<Dynamic, Dynamic, P>::MStoreRef; };
}  // namespace Internal

// ---- R6: fill operators ------------------------------------------------------------------------------------------------
struct SizedZerosV { int n; };
struct SizedZerosM { int r, c; };
struct ZerosTag {
  SizedZerosV operator()(int n) const { return SizedZerosV{n}; }
  SizedZerosM operator()(int r, int c) const { return SizedZerosM{r, c}; }
};
static const ZerosTag Zeros{};
template <class P>
struct ScaledIdentity {
  P s;
};
struct IdentityTag {};
static const IdentityTag Identity{};
template <class S, Internal::IfScalar<S> = 0>
ScaledIdentity<S> operator*(const IdentityTag&, S s) { return ScaledIdentity<S>{s}; }
template <class S, Internal::IfScalar<S> = 0>
ScaledIdentity<S> operator*(S s, const IdentityTag&) { return ScaledIdentity<S>{s}; }
template <class P, class S, Internal::IfScalar<S> = 0>
ScaledIdentity<typename Internal::Mul<P, S>::type> operator*(const ScaledIdentity<P>& i, S s) {
  return ScaledIdentity<typename Internal::Mul<P, S>::type>{i.s * s};
}
template <class P, class S, Internal::IfScalar<S> = 0>
ScaledIdentity<typename Internal::Mul<P, S>::type> operator*(S s, const ScaledIdentity<P>& i) {
  return ScaledIdentity<typename Internal::Mul<P, S>::type>{s * i.s};
}
template <class P>
struct DataFill {
  std::vector<P> d;  // row-major
};
template <class... A>
DataFill<typename std::common_type<A...>::type> Data(A... a) {
  typedef typename std::common_type<A...>::type P;
  return DataFill<P>{std::vector<P>{static_cast<P>(a)...}};
}
template <int N, class P>
struct DiagonalFill;

template <int R, int C, class P, bool Ref>
struct Matrix;

// ---- Vector ---------------------------------------------------------------------------------------------------------------
template <int N = Dynamic, class P = double, bool Ref = false>
struct Vector : Internal::VStore<N, P, Ref> {
  typedef Internal::VStore<N, P, Ref> Store;
  typedef P precision;
  static const int SizeParameter = N;
  using Store::ptr;
  using Store::size;
  using Store::stride;

  Vector() {}
  explicit Vector(int n) : Store(n) {}
  Vector(P* p, int n, int s) : Store(p, n, s) {}
  Vector(const ZerosTag&) { *this = Zeros; }
  Vector(const SizedZerosV& z) : Store(z.n) { *this = Zeros; }
  template <int N2, class P2, bool B2>
  Vector(const Vector<N2, P2, B2>& o) : Store(o.size()) { *this = o; }
  Vector(const Vector&) = default;
  Vector& operator=(const Vector&) = default;

  P& operator[](int i) { return ptr()[i * stride()]; }
  const P& operator[](int i) const { return ptr()[i * stride()]; }

  Vector& operator=(const ZerosTag&) {
    for (int i = 0; i < size(); ++i) (*this)[i] = 0;
    return *this;
  }
  template <int N2, class P2, bool B2>
  Vector& operator=(const Vector<N2, P2, B2>& o) {
    this->fit(o.size());
    for (int i = 0; i < size(); ++i) (*this)[i] = static_cast<P>(o[i]);
    return *this;
  }
  // R4
  template <int N2, class P2, bool B2>
  Vector& operator+=(const Vector<N2, P2, B2>& o) {
    assert(size() == o.size());
    for (int i = 0; i < size(); ++i) (*this)[i] += o[i];
    return *this;
  }
  template <int N2, class P2, bool B2>
  Vector& operator-=(const Vector<N2, P2, B2>& o) {
    assert(size() == o.size());
    for (int i = 0; i < size(); ++i) (*this)[i] -= o[i];
    return *this;
  }
  template <class S, Internal::IfScalar<S> = 0>
  Vector& operator/=(S s) {
    for (int i = 0; i < size(); ++i) (*this)[i] /= s;
    return *this;
  }
  template <class S, Internal::IfScalar<S> = 0>
  Vector& operator*=(S s) {
    for (int i = 0; i < size(); ++i) (*this)[i] *= s;
    return *this;
  }
  // R1: views
  template <int S, int L>
  Vector<L, P, true> slice() const {
    assert(S + L <= size());
    return Vector<L, P, true>(ptr() + S * stride(), L, stride());
  }
  Vector<Dynamic, P, true> slice(int s, int l) const {
    assert(s + l <= size());
    return Vector<Dynamic, P, true>(ptr() + s * stride(), l, stride());
  }
  Matrix<1, N, P, true> as_row() const;
  Matrix<N, 1, P, true> as_col() const;
  DiagonalFill<N, P> as_diagonal() const;
};

template <int N, class P>
struct DiagonalFill {
  Vector<N, P, false> v;
};

// R5
template <class... A>
Vector<(int)sizeof...(A), typename std::common_type<A...>::type> makeVector(A... a) {
  typedef typename std::common_type<A...>::type P;
  Vector<(int)sizeof...(A), P> r;
  const P vals[] = {static_cast<P>(a)...};
  for (int i = 0; i < (int)sizeof...(A); ++i) r[i] = vals[i];
  return r;
}

// ---- Matrix ---------------------------------------------------------------------------------------------------------------
template <int R = Dynamic, int C = R, class P = double, bool Ref = false>
struct Matrix : Internal::MStore<R, C, P, Ref> {
  typedef Internal::MStore<R, C, P, Ref> Store;
  typedef P precision;
  using Store::cs;
  using Store::num_cols;
  using Store::num_rows;
  using Store::ptr;
  using Store::rs;

  Matrix() {}
  Matrix(int r, int c) : Store(r, c) {}
  Matrix(P* p, int r, int c, int rs_, int cs_) : Store(p, r, c, rs_, cs_) {}
  Matrix(const ZerosTag&) { *this = Zeros; }
  Matrix(const SizedZerosM& z) : Store(z.r, z.c) { *this = Zeros; }
  Matrix(const IdentityTag&) { *this = ScaledIdentity<P>{P(1)}; }
  template <class Q>
  Matrix(const ScaledIdentity<Q>& i) { *this = i; }
  template <class Q>
  Matrix(const DataFill<Q>& f) { *this = f; }
  template <int N, class Q>
  Matrix(const DiagonalFill<N, Q>& f) { *this = f; }
  template <int R2, int C2, class P2, bool B2>
  Matrix(const Matrix<R2, C2, P2, B2>& o) : Store(o.num_rows(), o.num_cols()) { *this = o; }
  Matrix(const Matrix&) = default;
  Matrix& operator=(const Matrix&) = default;

  P& operator()(int i, int j) { return ptr()[i * rs() + j * cs()]; }
  const P& operator()(int i, int j) const { return ptr()[i * rs() + j * cs()]; }
  Vector<C, P, true> operator[](int i) const { return Vector<C, P, true>(ptr() + i * rs(), num_cols(), cs()); }
  Matrix<C, R, P, true> T() const { return Matrix<C, R, P, true>(ptr(), num_cols(), num_rows(), cs(), rs()); }
  template <int R0, int C0, int NR, int NC>
  Matrix<NR, NC, P, true> slice() const {
    assert(R0 + NR <= num_rows() && C0 + NC <= num_cols());
    return Matrix<NR, NC, P, true>(ptr() + R0 * rs() + C0 * cs(), NR, NC, rs(), cs());
  }
  Matrix<Dynamic, Dynamic, P, true> slice(int r0, int c0, int nr, int nc) const {
    assert(r0 + nr <= num_rows() && c0 + nc <= num_cols());
    return Matrix<Dynamic, Dynamic, P, true>(ptr() + r0 * rs() + c0 * cs(), nr, nc, rs(), cs());
  }

  Matrix& operator=(const ZerosTag&) {
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) = 0;
    return *this;
  }
  Matrix& operator=(const IdentityTag&) { return *this = ScaledIdentity<P>{P(1)}; }
  template <class Q>
  Matrix& operator=(const ScaledIdentity<Q>& id) {
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) = (i == j) ? static_cast<P>(id.s) : P(0);
    return *this;
  }
  template <class Q>
  Matrix& operator=(const DataFill<Q>& f) {
    assert((int)f.d.size() == num_rows() * num_cols());
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) = static_cast<P>(f.d[i * num_cols() + j]);
    return *this;
  }
  template <int N, class Q>
  Matrix& operator=(const DiagonalFill<N, Q>& f) {
    assert(f.v.size() == num_rows() && f.v.size() == num_cols());
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) = (i == j) ? static_cast<P>(f.v[i]) : P(0);
    return *this;
  }
  template <int R2, int C2, class P2, bool B2>
  Matrix& operator=(const Matrix<R2, C2, P2, B2>& o) {
    this->fit(o.num_rows(), o.num_cols());
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) = static_cast<P>(o(i, j));
    return *this;
  }
  // R4
  template <int R2, int C2, class P2, bool B2>
  Matrix& operator+=(const Matrix<R2, C2, P2, B2>& o) {
    assert(num_rows() == o.num_rows() && num_cols() == o.num_cols());
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) += o(i, j);
    return *this;
  }
  template <int R2, int C2, class P2, bool B2>
  Matrix& operator-=(const Matrix<R2, C2, P2, B2>& o) {
    assert(num_rows() == o.num_rows() && num_cols() == o.num_cols());
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) -= o(i, j);
    return *this;
  }
  template <class S, Internal::IfScalar<S> = 0>
  Matrix& operator/=(S s) {
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) /= s;
    return *this;
  }
  template <class S, Internal::IfScalar<S> = 0>
  Matrix& operator*=(S s) {
    for (int i = 0; i < num_rows(); ++i)
      for (int j = 0; j < num_cols(); ++j) (*this)(i, j) *= s;
    return *this;
  }
};

template <int N, class P, bool Ref>
Matrix<1, N, P, true> Vector<N, P, Ref>::as_row() const {
  return Matrix<1, N, P, true>(ptr(), 1, size(), 0, stride());
}
template <int N, class P, bool Ref>
Matrix<N, 1, P, true> Vector<N, P, Ref>::as_col() const {
  return Matrix<N, 1, P, true>(ptr(), size(), 1, stride(), 0);
}
template <int N, class P, bool Ref>
DiagonalFill<N, P> Vector<N, P, Ref>::as_diagonal() const {
  DiagonalFill<N, P> f;
  f.v = *this;
  return f;
}

// ---- R3 / R4: vector operators ----------------------------------------------------------------------------------------
#define TOON_SHIM_VV template <int N1, class P1, bool B1, int N2, class P2, bool B2>
#define TOON_SHIM_VRES Vector<Internal::pick(N1, N2), typename Internal::Mul<P1, P2>::type>

TOON_SHIM_VV typename Internal::Mul<P1, P2>::type operator*(const Vector<N1, P1, B1>& a, const Vector<N2, P2, B2>& b) {
  assert(a.size() == b.size());
  typename Internal::Mul<P1, P2>::type r = 0;
  for (int i = 0; i < a.size(); ++i) r += a[i] * b[i];
  return r;
}
TOON_SHIM_VV TOON_SHIM_VRES operator+(const Vector<N1, P1, B1>& a, const Vector<N2, P2, B2>& b) {
  assert(a.size() == b.size());
  TOON_SHIM_VRES r(a.size());
  for (int i = 0; i < a.size(); ++i) r[i] = a[i] + b[i];
  return r;
}
TOON_SHIM_VV TOON_SHIM_VRES operator-(const Vector<N1, P1, B1>& a, const Vector<N2, P2, B2>& b) {
  assert(a.size() == b.size());
  TOON_SHIM_VRES r(a.size());
  for (int i = 0; i < a.size(); ++i) r[i] = a[i] - b[i];
  return r;
}
// cross product of two 3-vectors
TOON_SHIM_VV Vector<3, typename Internal::Mul<P1, P2>::type> operator^(const Vector<N1, P1, B1>& a, const Vector<N2, P2, B2>& b) {
  assert(a.size() == 3 && b.size() == 3);
  Vector<3, typename Internal::Mul<P1, P2>::type> r;
  r[0] = a[1] * b[2] - a[2] * b[1];
  r[1] = a[2] * b[0] - a[0] * b[2];
  r[2] = a[0] * b[1] - a[1] * b[0];
  return r;
}
template <int N, class P, bool B>
Vector<N, P> operator-(const Vector<N, P, B>& a) {
  Vector<N, P> r(a.size());
  for (int i = 0; i < a.size(); ++i) r[i] = -a[i];
  return r;
}
template <int N, class P, bool B, class S, Internal::IfScalar<S> = 0>
Vector<N, typename Internal::Mul<P, S>::type> operator*(const Vector<N, P, B>& a, S s) {
  Vector<N, typename Internal::Mul<P, S>::type> r(a.size());
  for (int i = 0; i < a.size(); ++i) r[i] = a[i] * s;
  return r;
}
template <int N, class P, bool B, class S, Internal::IfScalar<S> = 0>
Vector<N, typename Internal::Mul<P, S>::type> operator*(S s, const Vector<N, P, B>& a) {
  Vector<N, typename Internal::Mul<P, S>::type> r(a.size());
  for (int i = 0; i < a.size(); ++i) r[i] = s * a[i];
  return r;
}
template <int N, class P, bool B, class S, Internal::IfScalar<S> = 0>
Vector<N, typename Internal::Mul<P, S>::type> operator/(const Vector<N, P, B>& a, S s) {
  Vector<N, typename Internal::Mul<P, S>::type> r(a.size());
  for (int i = 0; i < a.size(); ++i) r[i] = a[i] / s;
  return r;
}

// ---- R3 / R4 / R6: matrix operators ---------------------------------------------------------------------------------
#define TOON_SHIM_MM template <int R1, int C1, class P1, bool B1, int R2, int C2, class P2, bool B2>

TOON_SHIM_MM Matrix<R1, C2, typename Internal::Mul<P1, P2>::type> operator*(const Matrix<R1, C1, P1, B1>& a, const Matrix<R2, C2, P2, B2>& b) {
  assert(a.num_cols() == b.num_rows());
  typedef typename Internal::Mul<P1, P2>::type P;
  Matrix<R1, C2, P> r(a.num_rows(), b.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < b.num_cols(); ++j) {
      P s = 0;
      for (int k = 0; k < a.num_cols(); ++k) s += a(i, k) * b(k, j);
      r(i, j) = s;
    }
  return r;
}
template <int R1, int C1, class P1, bool B1, int N2, class P2, bool B2>
Vector<R1, typename Internal::Mul<P1, P2>::type> operator*(const Matrix<R1, C1, P1, B1>& a, const Vector<N2, P2, B2>& v) {
  assert(a.num_cols() == v.size());
  typedef typename Internal::Mul<P1, P2>::type P;
  Vector<R1, P> r(a.num_rows());
  for (int i = 0; i < a.num_rows(); ++i) {
    P s = 0;
    for (int k = 0; k < a.num_cols(); ++k) s += a(i, k) * v[k];
    r[i] = s;
  }
  return r;
}
TOON_SHIM_MM Matrix<Internal::pick(R1, R2), Internal::pick(C1, C2), typename Internal::Mul<P1, P2>::type> operator+(
    const Matrix<R1, C1, P1, B1>& a, const Matrix<R2, C2, P2, B2>& b) {
  assert(a.num_rows() == b.num_rows() && a.num_cols() == b.num_cols());
  Matrix<Internal::pick(R1, R2), Internal::pick(C1, C2), typename Internal::Mul<P1, P2>::type> r(a.num_rows(), a.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < a.num_cols(); ++j) r(i, j) = a(i, j) + b(i, j);
  return r;
}
TOON_SHIM_MM Matrix<Internal::pick(R1, R2), Internal::pick(C1, C2), typename Internal::Mul<P1, P2>::type> operator-(
    const Matrix<R1, C1, P1, B1>& a, const Matrix<R2, C2, P2, B2>& b) {
  assert(a.num_rows() == b.num_rows() && a.num_cols() == b.num_cols());
  Matrix<Internal::pick(R1, R2), Internal::pick(C1, C2), typename Internal::Mul<P1, P2>::type> r(a.num_rows(), a.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < a.num_cols(); ++j) r(i, j) = a(i, j) - b(i, j);
  return r;
}
template <int R, int C, class P, bool B, class S, Internal::IfScalar<S> = 0>
Matrix<R, C, typename Internal::Mul<P, S>::type> operator*(const Matrix<R, C, P, B>& a, S s) {
  Matrix<R, C, typename Internal::Mul<P, S>::type> r(a.num_rows(), a.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < a.num_cols(); ++j) r(i, j) = a(i, j) * s;
  return r;
}
template <int R, int C, class P, bool B, class S, Internal::IfScalar<S> = 0>
Matrix<R, C, typename Internal::Mul<P, S>::type> operator*(S s, const Matrix<R, C, P, B>& a) {
  Matrix<R, C, typename Internal::Mul<P, S>::type> r(a.num_rows(), a.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < a.num_cols(); ++j) r(i, j) = s * a(i, j);
  return r;
}
template <int R, int C, class P, bool B, class S, Internal::IfScalar<S> = 0>
Matrix<R, C, typename Internal::Mul<P, S>::type> operator/(const Matrix<R, C, P, B>& a, S s) {
  Matrix<R, C, typename Internal::Mul<P, S>::type> r(a.num_rows(), a.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < a.num_cols(); ++j) r(i, j) = a(i, j) / s;
  return r;
}
template <int R, int C, class P, bool B, class Q>
Matrix<R, C, typename Internal::Mul<P, Q>::type> operator+(const Matrix<R, C, P, B>& a, const ScaledIdentity<Q>& id) {
  Matrix<R, C, typename Internal::Mul<P, Q>::type> r(a);
  for (int i = 0; i < a.num_rows(); ++i) r(i, i) = a(i, i) + id.s;
  return r;
}
template <int R, int C, class P, bool B, class Q>
Matrix<R, C, typename Internal::Mul<P, Q>::type> operator+(const ScaledIdentity<Q>& id, const Matrix<R, C, P, B>& a) {
  return a + id;
}
template <int R, int C, class P, bool B>
Matrix<R, C, P> operator+(const Matrix<R, C, P, B>& a, const IdentityTag&) { return a + ScaledIdentity<P>{P(1)}; }
template <int R, int C, class P, bool B>
Matrix<R, C, P> operator+(const IdentityTag&, const Matrix<R, C, P, B>& a) { return a + ScaledIdentity<P>{P(1)}; }
template <int R, int C, class P, bool B, class Q>
Matrix<R, C, typename Internal::Mul<P, Q>::type> operator-(const Matrix<R, C, P, B>& a, const ScaledIdentity<Q>& id) {
  Matrix<R, C, typename Internal::Mul<P, Q>::type> r(a);
  for (int i = 0; i < a.num_rows(); ++i) r(i, i) = a(i, i) - id.s;
  return r;
}
template <int R, int C, class P, bool B, class Q>
Matrix<R, C, typename Internal::Mul<P, Q>::type> operator-(const ScaledIdentity<Q>& id, const Matrix<R, C, P, B>& a) {
  Matrix<R, C, typename Internal::Mul<P, Q>::type> r(a.num_rows(), a.num_cols());
  for (int i = 0; i < a.num_rows(); ++i)
    for (int j = 0; j < a.num_cols(); ++j) r(i, j) = (i == j) ? id.s - a(i, j) : -a(i, j);
  return r;
}
template <int R, int C, class P, bool B>
Matrix<R, C, P> operator-(const Matrix<R, C, P, B>& a, const IdentityTag&) { return a - ScaledIdentity<P>{P(1)}; }
template <int R, int C, class P, bool B>
Matrix<R, C, P> operator-(const IdentityTag&, const Matrix<R, C, P, B>& a) { return ScaledIdentity<P>{P(1)} - a; }

// ---- streams ---------------------------------------------------------------------------------------------------------------
template <int N, class P, bool B>
std::ostream& operator<<(std::ostream& os, const Vector<N, P, B>& v) {
  for (int i = 0; i < v.size(); ++i) os << v[i] << " ";
  return os;
}
template <int R, int C, class P, bool B>
std::ostream& operator<<(std::ostream& os, const Matrix<R, C, P, B>& m) {
  for (int i = 0; i < m.num_rows(); ++i) {
    for (int j = 0; j < m.num_cols(); ++j) os << m(i, j) << " ";
    os << "\n";
  }
  return os;
}

#undef TOON_SHIM_VV
#undef TOON_SHIM_VRES
#undef TOON_SHIM_MM

}  // namespace TooN

#include <TooN/helpers.h>

#endif
