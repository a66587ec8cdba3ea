// The per-item complex linear algebra shared by the one-lane-per-item kernels (mimo_linalg.hip, f64.hip, precoding.hip,
// post_eq_sinr.hip): a {re, im} pair with its operators, the in-place lower Cholesky factor and the two triangular
// substitutions.  mimo_linalg.hip and f64.hip call all three, post_eq_sinr.hip calls chol, precoding.hip takes the type and
// the accessors; what those two write out themselves, and why, is said at the place.  (csrc/mimo.hip keeps its own
// register-array forms.)
//
// Order of operations - the one of oracle/mimo_f32.py::cholesky and of the substitutions of tests/precoding_f32.py, which
// float32 callers compiled with -ffp-contract=off reproduce bit for bit:
//   a b = (a.re b.re - a.im b.im, a.re b.im + a.im b.re);  |z|^2 = re*re + im*im;  every sum in ascending index order;
//   Cholesky-Banachiewicz, column j:  d = a_jj.re;  d = d - |a_jq|^2 for q < j;  L_jj = sqrt(d);  inv = 1 / L_jj;
//     L_ij = (a_ij - sum_{q<j} a_iq conj(a_jq)) * inv for i > j, the sum subtracted term by term;
//   forward   x_i = (x_i - sum_{q<i} L_iq x_q) * (1 / L_ii),  i ascending;
//   backward  x_i = (x_i - sum_{q>i} conj(L_qi) x_q) * (1 / L_ii),  i descending.
// Only the lower triangle of the factor is read or written; the strict upper triangle keeps whatever the caller left there.
//
// NT > 0 is a compile-time size (loops unrolled completely, arrays in registers once inlined into a kernel); NT == 0 takes the
// size from the run-time argument and leaves the loops rolled.  The functions also compile as plain host C++
// (tests/test_cx_linalg_host.py holds them to the specification without a GPU), so this file does not include common.h.
#ifndef SAMD_CX_LINALG_H_
#define SAMD_CX_LINALG_H_
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SAMD_HD __host__ __device__ __forceinline__
#else
#define SAMD_HD inline
#endif

namespace samd {
namespace {

template <typename R> struct cx { R re, im; };
template <typename R> SAMD_HD cx<R> C(R r, R i) { return cx<R>{r, i}; }
template <typename R> SAMD_HD cx<R> operator+(cx<R> a, cx<R> b) { return C<R>(a.re + b.re, a.im + b.im); }
template <typename R> SAMD_HD cx<R> operator-(cx<R> a, cx<R> b) { return C<R>(a.re - b.re, a.im - b.im); }
template <typename R> SAMD_HD cx<R> operator*(cx<R> a, cx<R> b) {
  return C<R>(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re);
}
template <typename R> SAMD_HD cx<R> mulcj(cx<R> a, cx<R> b) {      // a conj(b)
  return C<R>(a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im);
}
template <typename R> SAMD_HD cx<R> cjm(cx<R> a, cx<R> b) {        // conj(a) b
  return C<R>(a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re);
}
template <typename R> SAMD_HD cx<R> sc(cx<R> a, R t) { return C<R>(a.re * t, a.im * t); }
template <typename R> SAMD_HD R abs2(cx<R> a) { return a.re * a.re + a.im * a.im; }

#ifdef __HIPCC__
template <typename R> struct vec2;
template <> struct vec2<float> { using type = float2; };
template <> struct vec2<double> { using type = double2; };
// element i of an interleaved complex array (one 8- / 16-byte access)
template <typename R> __device__ __forceinline__ cx<R> ld(const R* __restrict__ p, int64_t i) {
  const typename vec2<R>::type v = reinterpret_cast<const typename vec2<R>::type*>(p)[i];
  return C<R>(v.x, v.y);
}
template <typename R> __device__ __forceinline__ void st(R* __restrict__ p, int64_t i, cx<R> v) {
  typename vec2<R>::type w;
  w.x = v.re;
  w.y = v.im;
  reinterpret_cast<typename vec2<R>::type*>(p)[i] = w;
}
#endif

// in-place lower Cholesky factor of the Hermitian n x n matrix a (row stride n); a[j * n + j].re = L_jj
template <typename R, int NT> SAMD_HD void chol(cx<R>* a, int n_rt) {
  const int n = NT ? NT : n_rt;
  constexpr int U = NT ? 32 : 1;
#pragma unroll U
  for (int j = 0; j < n; ++j) {
    R d = a[j * n + j].re;
#pragma unroll U
    for (int q = 0; q < j; ++q) d = d - abs2(a[j * n + q]);
    d = sqrt(d);
    a[j * n + j] = C<R>(d, R(0));
    const R inv = R(1) / d;
#pragma unroll U
    for (int i = j + 1; i < n; ++i) {
      cx<R> v = a[i * n + j];
#pragma unroll U
      for (int q = 0; q < j; ++q) v = v - mulcj(a[i * n + q], a[j * n + q]);
      a[i * n + j] = sc(v, inv);
    }
  }
}

// x <- L^-1 x for the `cols` right-hand sides x[row * ldx + col], L the factor chol left in l
template <typename R, int NT> SAMD_HD void fwd(const cx<R>* l, int n_rt, cx<R>* x, int ldx, int cols) {
  const int n = NT ? NT : n_rt;
  constexpr int U = NT ? 32 : 1;
#pragma unroll U
  for (int c = 0; c < cols; ++c)
#pragma unroll U
    for (int i = 0; i < n; ++i) {
      cx<R> v = x[i * ldx + c];
#pragma unroll U
      for (int q = 0; q < i; ++q) v = v - l[i * n + q] * x[q * ldx + c];
      x[i * ldx + c] = sc(v, R(1) / l[i * n + i].re);
    }
}

// x <- L^-H x
template <typename R, int NT> SAMD_HD void bwd(const cx<R>* l, int n_rt, cx<R>* x, int ldx, int cols) {
  const int n = NT ? NT : n_rt;
  constexpr int U = NT ? 32 : 1;
#pragma unroll U
  for (int c = 0; c < cols; ++c)
#pragma unroll U
    for (int i = n - 1; i >= 0; --i) {
      cx<R> v = x[i * ldx + c];
#pragma unroll U
      for (int q = i + 1; q < n; ++q) v = v - cjm(l[q * n + i], x[q * ldx + c]);
      x[i * ldx + c] = sc(v, R(1) / l[i * n + i].re);
    }
}

}  // namespace
}  // namespace samd

#endif  // SAMD_CX_LINALG_H_
