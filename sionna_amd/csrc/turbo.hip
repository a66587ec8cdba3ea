// Turbo codes: encoder and the half-iteration of the decoder (one BCJR pass of one constituent code).
//   TurboEncoder.call       fec/turbo/encoding.py:365-421  (_conv_enc :235-289, _puncture_cw :291-341)
//   TurboDecoder.call       fec/turbo/decoding.py:357-435  (depuncture :254-269, _convenc_cws :271-312)
// The recursions, the lane layout (trellis states across the lanes of a wave, several codewords per wave), the LDS /
// workspace split of the alphas and the order of operations are those of conv_bcjr_kernel (conv.hip); the device code
// they share is bcjr_core.h.  What this kernel fuses around the recursions:
//   - the two channel values of trellis step t are loaded through an index table, llr_ch[cw * n + idx[t][j]], -1 a
//     punctured or absent position (value 0): no depunctured, re-ordered or interleaved copy of the codeword exists;
//   - for t < k the backward pass computes the extrinsic value in the reference's order (decoder 1 (L - ch) - a,
//     decoder 2 (L - a) - ch, decoding.py:407, 417), clips it to +-20 and scatters it into the other decoder's
//     a priori buffer through the (inverse) interleaver table;
//   - the last half-iteration writes out[perm[t]] = L instead, the second decoder's output de-interleaved (:428),
//     as 0 < L with hard_out.
// A decoder call is 2 num_iter launches of this kernel.  The index tables are built on the host
// (sionna_amd/phy/fec/turbo/utils.py: turbo_tables), which is also where their bounds are checked.
#include <math.h>

#include "bcjr_core.h"
#include "common.h"

namespace samd {
namespace {

constexpr int kExt1 = 0, kExt2 = 1, kFinal = 2;       // SAMD_TURBO_EXT1 / _EXT2 / _FINAL
constexpr int kConvN = 2;                             // the constituent code is rate 1/2 (decoding.py:184-187)

// ---------------------------------------------------------------- encoder
// One lane per (codeword, constituent encoder): the RSC recursion of conv_encode_rsc_kernel with the feedback
// termination (encoding.py:270-287); encoder 1 reads its input through perm.  The two output bits of step t go to
// c[opos[e][t][j]] (-1: punctured, or the systematic bit of encoder 1 which is not transmitted); the zero padding of the
// termination (utils.py:222-229) is written by the lane of encoder 0.
template <typename R>
__global__ void turbo_encode_kernel(const R* __restrict__ u, const int32_t* __restrict__ perm,
                                    const int32_t* __restrict__ opos, int64_t batch, int k, int T, int n, Trellis tr,
                                    int zpos0, int zpos1, R* __restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * batch) return;
  const int64_t b = i >> 1;
  const int e = (int)(i & 1);
  const R* ub = u + b * (int64_t)k;
  R* cb = c + b * (int64_t)n;
  const int32_t* op = opos + (int64_t)e * T * kConvN;
  const uint32_t mask = (uint32_t)tr.ns - 1u;
  uint32_t st = 0;
  for (int t = 0; t < T; ++t) {
    const uint32_t fb = __popc(st & tr.poly[0] & mask) & 1u;
    uint32_t nb = 0u;
    if (t < k) nb = ((uint32_t)(int)ub[e ? perm[t] : t] & 1u) ^ fb;
    const uint32_t sbits = (nb << tr.mu) | st;
    for (int p = 0; p < kConvN; ++p) {
      const int pos = op[t * kConvN + p];
      if (pos >= 0) cb[pos] = (R)(__popc(sbits & tr.poly[p]) & 1);
    }
    st = sbits >> 1;
  }
  if (e == 0) {
    if (zpos0 >= 0) cb[zpos0] = (R)0;
    if (zpos1 >= 0) cb[zpos1] = (R)0;
  }
}

// ---------------------------------------------------------------- half-iteration
// Stages steps [t0, t0 + kCh) of the wave's codewords: ys[tt * 2 + j] channel values through idx, as[tt] a priori.
template <typename R>
__device__ __forceinline__ void stage_idx(const R* __restrict__ y, const int32_t* __restrict__ idx, const R* __restrict__ la,
                                          int64_t cw, bool valid, int n, int T, int t0, int L, int sl, R* ys, R* as) {
  const int e0 = t0 * kConvN, E = kCh * kConvN;
  for (int e = sl; e < E; e += L) {
    R v = (R)0;
    if (valid && e0 + e < T * kConvN) {
      const int p = idx[e0 + e];
      if (p >= 0) v = y[cw * (int64_t)n + p];
    }
    ys[e] = v;
  }
  for (int j = sl; j < kCh; j += L) as[j] = (valid && t0 + j < T) ? la[cw * (int64_t)T + t0 + j] : (R)0;
}

template <typename R, int ALG, int SPL>
__global__ void __launch_bounds__(64) turbo_bcjr_kernel(const R* __restrict__ llr_ch, const int32_t* __restrict__ idx,
                                                         const R* __restrict__ la_in, const int32_t* __restrict__ scat,
                                                         int64_t batch, int n, int T, int k, Trellis tr, int terminate,
                                                         int mode, int hard_out, R beta_eq, R* __restrict__ dst,
                                                         R* __restrict__ ws_alpha) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int ns = tr.ns, conv_n = kConvN;
  const int L = ns < 64 ? ns : 64, G = 64 / L;
  const int lane = threadIdx.x, g = lane / L, sl = lane % L, g0 = g * L;
  const int64_t cw = (int64_t)blockIdx.x * G + g;
  const bool valid = cw < batch;
  R* ybuf = (R*)smem;                                          // [G][kCh * conv_n]
  R* abuf = ybuf + G * kCh * conv_n;                           // [G][kCh]
  R* alpha_st = ws_alpha ? ws_alpha + (int64_t)blockIdx.x * T * (64 * SPL) : abuf + G * kCh;   // [T][SPL][64]
  R* ys = ybuf + g * kCh * conv_n;
  R* as = abuf + g * kCh;
  const R one = ALG == kMap ? (R)1 : (R)0, zero = ALG == kMap ? (R)0 : (R)-INFINITY;
  const int dstride = mode == kFinal ? k : T;                  // out [batch, k] or the a priori buffer [batch, T]
  int f[SPL][2], ip[SPL][2], o[SPL][2], to[SPL][2], of[SPL][2];
  R alpha[SPL], beta[SPL];
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int s = sl + 64 * q;
    for (int j = 0; j < 2; ++j) {
      f[q][j] = tr.from[s][j];
      ip[q][j] = tr.ip_to[s][j];
      o[q][j] = tr.op_to[s][j];
      to[q][j] = tr.to[s][j];
      of[q][j] = tr.op_from[s][j];
    }
    alpha[q] = s == 0 ? one : zero;                            // _initialize (fec/conv/decoding.py:682-698)
    beta[q] = terminate ? alpha[q] : beta_eq;
  }
  // forward recursion (_update_fwd, fec/conv/decoding.py:700-790): alpha_t stored before step t
  for (int t0 = 0; t0 < T; t0 += kCh) {
    __syncthreads();
    stage_idx<R>(llr_ch, idx, la_in, cw, valid, n, T, t0, L, sl, ys, as);
    __syncthreads();
    const int te = T - t0 < kCh ? T - t0 : kCh;
    for (int tt = 0; tt < te; ++tt) {
      const int t = t0 + tt;
      const R* yt = ys + tt * conv_n;
      const R la = as[tt];
      R na[SPL];
#pragma unroll
      for (int q = 0; q < SPL; ++q) {
        alpha_st[(int64_t)t * (64 * SPL) + q * 64 + lane] = alpha[q];
        R term[2];
        for (int j = 0; j < 2; ++j) {
          const R p = state_val<R, SPL>(alpha, g0, f[q][j]);
          const R gm = bcjr_gamma<R, ALG>(yt, la, conv_n, ip[q][j], o[q][j]);
          term[j] = ALG == kMap ? gm * p : gm + p;
        }
        na[q] = comb2<R, ALG>(term[0], term[1]);
      }
      if (ALG == kMap) {
        const R tot = fold_sum<R, SPL>(na, L);
#pragma unroll
        for (int q = 0; q < SPL; ++q) na[q] = na[q] / tot;
      }
#pragma unroll
      for (int q = 0; q < SPL; ++q) alpha[q] = na[q];
    }
  }
  // backward recursion, output LLRs (_update_bwd, fec/conv/decoding.py:792-880) and the epilogue of the turbo loop
  const int nchunks = (T + kCh - 1) / kCh;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int t0 = c * kCh;
    __syncthreads();
    stage_idx<R>(llr_ch, idx, la_in, cw, valid, n, T, t0, L, sl, ys, as);
    __syncthreads();
    const int te = T - t0 < kCh ? T - t0 : kCh;
    for (int tt = te - 1; tt >= 0; --tt) {
      const int t = t0 + tt;
      const R* yt = ys + tt * conv_n;
      const R la = as[tt];
      R nb[SPL], l0[SPL], l1[SPL];
#pragma unroll
      for (int q = 0; q < SPL; ++q) {
        const R at = alpha_st[(int64_t)t * (64 * SPL) + q * 64 + lane];
        R gm[2], bb[2];
        for (int b = 0; b < 2; ++b) {
          gm[b] = bcjr_gamma<R, ALG>(yt, la, conv_n, b, of[q][b]);
          bb[b] = state_val<R, SPL>(beta, g0, to[q][b]);
        }
        if (ALG == kMap) {
          nb[q] = gm[0] * bb[0] + gm[1] * bb[1];
          l0[q] = (at * gm[0]) * bb[0];
          l1[q] = (at * gm[1]) * bb[1];
        } else {
          nb[q] = comb2<R, ALG>(gm[0] + bb[0], gm[1] + bb[1]);
          l0[q] = (at + gm[0]) + bb[0];
          l1[q] = (at + gm[1]) + bb[1];
        }
      }
      R llr;
      if (ALG == kMap) {
        const R tot = fold_sum<R, SPL>(nb, L);
#pragma unroll
        for (int q = 0; q < SPL; ++q) nb[q] = nb[q] / tot;
        llr = dlog<R>(fold_sum<R, SPL>(l0, L) / fold_sum<R, SPL>(l1, L));
      } else if (ALG == kLog) {
        llr = fold_lse<R, SPL>(l0, L) - fold_lse<R, SPL>(l1, L);
      } else {
        llr = fold_max<R, SPL>(l0, L) - fold_max<R, SPL>(l1, L);
      }
#pragma unroll
      for (int q = 0; q < SPL; ++q) beta[q] = nb[q];
      if (valid && sl == 0 && t < k) {
        const R m = -llr;                                         // back to log p(1)/p(0) (fec/conv/decoding.py:934)
        R v;
        if (mode == kFinal) {
          v = hard_out ? ((R)0 < m ? (R)1 : (R)0) : m;            // decoding.py:428-432
        } else {
          const R ch = yt[0];                                     // the systematic channel value of this step
          v = mode == kExt1 ? (m - ch) - la : (m - la) - ch;      // decoding.py:407, 417
          v = v < (R)-20 ? (R)-20 : (v > (R)20 ? (R)20 : v);      // clip_by_value (:411-413, 421-423); NaN passes
        }
        dst[cw * (int64_t)dstride + scat[t]] = v;
      }
    }
  }
}

// ---------------------------------------------------------------- host side
int turbo_trellis(const uint32_t* polys, int constraint_length, Trellis* tr) {
  return build_trellis(polys, kConvN, constraint_length, 1, tr);
}

template <typename R>
int encode(const R* u, const int32_t* perm, const int32_t* opos, int64_t batch, int k, int n, const uint32_t* polys,
           int constraint_length, int terminate, int zpos0, int zpos1, R* c, void* stream) {
  Trellis tr;
  int rc = turbo_trellis(polys, constraint_length, &tr);
  if (rc != SAMD_OK) return rc;
  SAMD_REQUIRE(batch >= 0 && k >= 0 && n >= 0, "TurboEncoder: invalid dimensions");
  SAMD_REQUIRE(zpos0 >= -1 && zpos0 < n && zpos1 >= -1 && zpos1 < n, "TurboEncoder: padding position outside the codeword");
  const int T = k + (terminate ? tr.mu : 0);
  if (batch == 0 || n == 0) return SAMD_OK;
  SAMD_REQUIRE(u && perm && opos && c, "null argument");
  SAMD_REQUIRE((2 * batch + 255) / 256 <= 0x7fffffff, "TurboEncoder: batch too large for one launch");
  hipLaunchKernelGGL(turbo_encode_kernel<R>, dim3((unsigned)((2 * batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u,
                     perm, opos, batch, k, T, n, tr, zpos0, zpos1, c);
  return launch_status();
}

template <typename R>
int bcjr(const R* llr_ch, const int32_t* idx, const R* la_in, const int32_t* scat, int64_t batch, int n, int k,
         const uint32_t* polys, int constraint_length, int terminate, int algorithm, int mode, int hard_out, R* dst,
         void* ws, size_t ws_bytes, void* stream) {
  Trellis tr;
  int rc = turbo_trellis(polys, constraint_length, &tr);
  if (rc != SAMD_OK) return rc;
  SAMD_REQUIRE(algorithm >= 0 && algorithm <= 2, "TurboDecoder: algorithm 0 (map), 1 (log) or 2 (maxlog)");
  SAMD_REQUIRE(mode == kExt1 || mode == kExt2 || mode == kFinal,"TurboDecoder: mode 0 (decoder 1), 1 (decoder 2) or 2 (last half-iteration)");
  SAMD_REQUIRE(batch >= 0 && n >= 0 && k >= 0, "TurboDecoder: invalid dimensions");
  const int T = k + (terminate ? tr.mu : 0);
  if (batch == 0 || k == 0) return SAMD_OK;
  SAMD_REQUIRE(llr_ch && idx && la_in && scat && dst, "null argument");
  SAMD_REQUIRE(la_in != dst, "TurboDecoder: the a priori buffer read and the buffer written must differ");
  const Shape sh = shape_of(tr.ns, batch);
  SAMD_REQUIRE(sh.waves <= 0x7fffffff, "TurboDecoder: batch too large for one launch");
  const int dbl = sizeof(R) == 8;
  const size_t need = bcjr_workspace_bytes(constraint_length, T, batch, dbl);
  if (need) {
    SAMD_REQUIRE(ws != nullptr, "TurboDecoder: workspace required (samd_turbo_workspace_bytes)");
    if (ws_bytes < need) {
      set_error("TurboDecoder: workspace too small");
      return SAMD_ERR_WORKSPACE;
    }
  }
  // eq_prob of the unterminated beta init (fec/conv/decoding.py:689-694), float64 then cast
  const double eq = 1.0 / tr.ns;
  const R beta_eq = (R)(algorithm == kMap ? eq : std::log(eq));
  const size_t lds = (size_t)sh.G * kCh * (kConvN + 1) * sizeof(R) + (need ? 0 : bcjr_alpha_bytes(tr.ns, T, dbl));
  hipStream_t s = (hipStream_t)stream;
  R* wsa = need ? (R*)ws : nullptr;
#define SAMD_TURBO(A_, S_)                                                                                    \
  if (algorithm == A_ && sh.SPL == S_) {                                                                      \
    SAMD_SET_MAX_LDS((turbo_bcjr_kernel<R, A_, S_>), (int)lds);                                               \
    hipLaunchKernelGGL((turbo_bcjr_kernel<R, A_, S_>), dim3((unsigned)sh.waves), dim3(64), lds, s, llr_ch, idx, la_in, scat, \
                       batch, n, T, k, tr, terminate, mode, hard_out, beta_eq, dst, wsa);                     \
    return launch_status();                                                                                   \
  }
  SAMD_TURBO(kMap, 1) SAMD_TURBO(kMap, 2) SAMD_TURBO(kLog, 1) SAMD_TURBO(kLog, 2) SAMD_TURBO(kMaxLog, 1) SAMD_TURBO(kMaxLog, 2)
#undef SAMD_TURBO
  set_error("TurboDecoder: no instantiation");
  return SAMD_ERR_INVALID;
}

}  // namespace
}  // namespace samd

extern "C" int samd_turbo_encode_f32(const float* u, const int32_t* perm, const int32_t* opos, int64_t batch, int k, int n,
                                     const uint32_t* polys, int constraint_length, int terminate, int zpos0, int zpos1,
                                     float* c, void* stream) {
  return samd::encode<float>(u, perm, opos, batch, k, n, polys, constraint_length, terminate, zpos0, zpos1, c, stream);
}
extern "C" int samd_turbo_encode_f64(const double* u, const int32_t* perm, const int32_t* opos, int64_t batch, int k, int n,
                                     const uint32_t* polys, int constraint_length, int terminate, int zpos0, int zpos1,
                                     double* c, void* stream) {
  return samd::encode<double>(u, perm, opos, batch, k, n, polys, constraint_length, terminate, zpos0, zpos1, c, stream);
}
extern "C" size_t samd_turbo_workspace_bytes(int constraint_length, int num_syms, int64_t batch, int dbl) {
  return samd::bcjr_workspace_bytes(constraint_length, num_syms, batch, dbl);
}
extern "C" int samd_turbo_bcjr_f32(const float* llr_ch, const int32_t* idx, const float* la_in, const int32_t* scat,
                                   int64_t batch, int n, int k, const uint32_t* polys, int constraint_length, int terminate,
                                   int algorithm, int mode, int hard_out, float* dst, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  return samd::bcjr<float>(llr_ch, idx, la_in, scat, batch, n, k, polys, constraint_length, terminate, algorithm, mode,
                           hard_out, dst, workspace, workspace_bytes, stream);
}
extern "C" int samd_turbo_bcjr_f64(const double* llr_ch, const int32_t* idx, const double* la_in, const int32_t* scat,
                                   int64_t batch, int n, int k, const uint32_t* polys, int constraint_length, int terminate,
                                   int algorithm, int mode, int hard_out, double* dst, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return samd::bcjr<double>(llr_ch, idx, la_in, scat, batch, n, k, polys, constraint_length, terminate, algorithm, mode,
                            hard_out, dst, workspace, workspace_bytes, stream);
}
