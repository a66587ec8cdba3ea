// Device and host code shared by the convolutional-code kernels (conv.hip) and the turbo-code kernels (turbo.hip): the
// trellis tables, the float32 exp / log, the folds over the states of a codeword and the BCJR branch metric.
// Lane layout and order of operations: see the head of conv.hip; the specification is tests/conv_f32.py.
#ifndef SAMD_BCJR_CORE_H_
#define SAMD_BCJR_CORE_H_
#include <math.h>
#include <string.h>

#include "common.h"

namespace samd {
namespace {

constexpr int kMaxStates = 128, kCh = 32;
constexpr size_t kBcjrLdsAlphaBytes = 32768;     // alphas kept in LDS up to this size per wave

struct Trellis {
  int ns, mu, conv_n, rsc;
  uint8_t from[kMaxStates][2];     // from_nodes
  uint8_t ip_to[kMaxStates][2];    // ip_by_tonode
  uint8_t op_to[kMaxStates][2];    // op_by_tonode
  uint8_t to[kMaxStates][2];       // to_nodes
  uint8_t op_from[kMaxStates][2];  // op_by_fromnode
  uint32_t poly[8];                // generator polynomials, bit (mu - i) = character i of the string
};

// fec/conv/utils.py:146-190, state bits MSB first (int2bin), poly 0 the most significant output bit (bin2int)
int build_trellis(const uint32_t* polys, int conv_n, int constraint_length, int rsc, Trellis* t) {
  SAMD_REQUIRE(polys != nullptr, "null argument");
  SAMD_REQUIRE(constraint_length >= 3 && constraint_length <= 8, "conv: constraint length 3..8");
  SAMD_REQUIRE(conv_n >= 1 && conv_n <= 8, "conv: 1..8 generator polynomials");
  const int mu = constraint_length - 1, ns = 1 << mu;
  memset(t, 0, sizeof(*t));
  t->ns = ns;
  t->mu = mu;
  t->conv_n = conv_n;
  t->rsc = rsc ? 1 : 0;
  for (int p = 0; p < conv_n; ++p) {
    SAMD_REQUIRE(polys[p] < (1u << constraint_length), "conv: polynomial wider than the constraint length");
    t->poly[p] = polys[p];
  }
  if (rsc) SAMD_REQUIRE((polys[0] >> mu) & 1u, "conv: the feedback polynomial must start with 1");
  int ctr[kMaxStates] = {0};
  for (int i = 0; i < 2; ++i) {
    for (int j = 0; j < ns; ++j) {
      const int fb = rsc ? (__builtin_popcount((uint32_t)j & polys[0] & (uint32_t)(ns - 1)) & 1) : 0;
      const int nb = (i + fb) & 1;
      const uint32_t sbits = ((uint32_t)nb << mu) | (uint32_t)j;
      const int j_to = (int)(sbits >> 1);
      int op = 0;
      for (int p = 0; p < conv_n; ++p) op = (op << 1) | (__builtin_popcount(sbits & polys[p]) & 1);
      t->to[j][i] = (uint8_t)j_to;
      t->from[j_to][ctr[j_to]] = (uint8_t)j;
      t->op_to[j_to][ctr[j_to]] = (uint8_t)op;
      t->ip_to[j_to][ctr[j_to]] = (uint8_t)i;
      t->op_from[j][i] = (uint8_t)op;
      ++ctr[j_to];
    }
  }
  return SAMD_OK;
}

// ---------------------------------------------------------------- decoder helpers
template <typename R> __device__ __forceinline__ R dexp(R x);
template <> __device__ __forceinline__ float dexp<float>(float x) { return (float)::exp((double)x); }
template <> __device__ __forceinline__ double dexp<double>(double x) { return ::exp(x); }
template <typename R> __device__ __forceinline__ R dlog(R x);
template <> __device__ __forceinline__ float dlog<float>(float x) { return (float)::log((double)x); }
template <> __device__ __forceinline__ double dlog<double>(double x) { return ::log(x); }

template <typename R> __device__ __forceinline__ R rmax(R a, R b) { return b > a ? b : a; }

// tf.reduce_logsumexp of two values (math_ops.py): m = max, replaced by 0 when not finite
template <typename R> __device__ __forceinline__ R lse2(R a, R b) {
  R m = rmax(a, b);
  if (!isfinite(m)) m = (R)0;
  return dlog<R>(dexp<R>(a - m) + dexp<R>(b - m)) + m;
}

// value of state f (slot f / 64, lane f mod 64 of the group starting at lane g0); every lane executes it
template <typename R, int SPL>
__device__ __forceinline__ R state_val(const R (&v)[SPL], int g0, int f) {
  if (SPL == 1) return __shfl(v[0], g0 + f, 64);
  const R a = __shfl(v[0], f & 63, 64);
  const R b = __shfl(v[SPL - 1], f & 63, 64);
  return f >= 64 ? b : a;
}

// halving-fold sum over the ns states of a codeword (in-lane slots first, then lane offsets L/2 .. 1)
template <typename R, int SPL>
__device__ __forceinline__ R fold_sum(const R (&v)[SPL], int L) {
  R s = v[0];
  if (SPL == 2) s = v[0] + v[SPL - 1];
  for (int off = L >> 1; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
  return s;
}
template <typename R, int SPL>
__device__ __forceinline__ R fold_max(const R (&v)[SPL], int L) {
  R s = v[0];
  if (SPL == 2) s = rmax(v[0], v[SPL - 1]);
  for (int off = L >> 1; off >= 1; off >>= 1) s = rmax(s, __shfl_xor(s, off, 64));
  return s;
}
// tf.reduce_logsumexp over the states
template <typename R, int SPL>
__device__ __forceinline__ R fold_lse(const R (&v)[SPL], int L) {
  R m = fold_max<R, SPL>(v, L);
  if (!isfinite(m)) m = (R)0;
  R e[SPL];
#pragma unroll
  for (int q = 0; q < SPL; ++q) e[q] = dexp<R>(v[q] - m);
  return dlog<R>(fold_sum<R, SPL>(e, L)) + m;
}

// ---------------------------------------------------------------- BCJR
constexpr int kMap = 0, kLog = 1, kMaxLog = 2;

// gamma of the transition leaving a state with input bit b and output symbol o (decoding.py:760-780, 826-836):
// log domain signed_half_llr_a + bm, map exp(signed_half_llr_a) * exp(bm); bm = sum_j 0.5 * (llr_j * (1 - 2 c_j))
template <typename R, int ALG>
__device__ __forceinline__ R bcjr_gamma(const R* yt, R la, int conv_n, int b, int o) {
  R acc = (R)0;
  for (int j = 0; j < conv_n; ++j) {
    const int bit = (o >> (conv_n - 1 - j)) & 1;
    const R yn = -yt[j];                                          // log p(0)/p(1) internally (decoding.py:924-925)
    const R v = (R)0.5 * (bit ? -yn : yn);
    acc = j == 0 ? v : acc + v;
  }
  const R h = (R)0.5 * -la;
  const R sl = b ? -h : h;
  if (ALG == kMap) return dexp<R>(sl) * dexp<R>(acc);
  return sl + acc;
}

template <typename R, int ALG>
__device__ __forceinline__ R comb2(R a, R b) {
  if (ALG == kMap) return a + b;
  if (ALG == kLog) return lse2<R>(a, b);
  return rmax(a, b);
}

// codewords per wave, lanes per codeword and states per lane of a trellis with ns states
struct Shape {
  int L, G, SPL;
  int64_t waves;
};
inline Shape shape_of(int ns, int64_t batch) {
  Shape s;
  s.L = ns < 64 ? ns : 64;
  s.G = 64 / s.L;
  s.SPL = ns / s.L;
  s.waves = (batch + s.G - 1) / s.G;
  return s;
}

inline size_t bcjr_alpha_bytes(int ns, int T, int dbl) { return (size_t)T * (size_t)(ns > 64 ? 128 : 64) * (dbl ? 8 : 4); }

// bytes of the alpha workspace of a BCJR launch: 0 while the alphas of a wave fit into LDS
inline size_t bcjr_workspace_bytes(int constraint_length, int num_syms, int64_t batch, int dbl) {
  if (constraint_length < 3 || constraint_length > 8 || num_syms < 0 || batch < 0) return 0;
  const int ns = 1 << (constraint_length - 1);
  const size_t per = bcjr_alpha_bytes(ns, num_syms, dbl);
  return per <= kBcjrLdsAlphaBytes ? 0 : per * (size_t)shape_of(ns, batch).waves;
}

}  // namespace
}  // namespace samd
#endif  // SAMD_BCJR_CORE_H_
