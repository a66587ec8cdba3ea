// Convolutional codes: encoder, Viterbi decoder, BCJR decoder (map / log / maxlog).
//   ConvEncoder.call        fec/conv/encoding.py:221-292
//   ViterbiDecoder.call     fec/conv/decoding.py:236-453  (_update_fwd, _optimal_path, _op_bits_path, _bmcalc)
//   BCJRDecoder.call        fec/conv/decoding.py:700-943  (_bmcalc, _initialize, _update_fwd, _update_bwd)
// The trellis tables are built here on the host exactly as Trellis._generate_transitions (fec/conv/utils.py:146-190)
// builds them, so the order of from_nodes (which decides the Viterbi tie-breaking) is the reference's.
//
// Lane layout of both decoders: trellis states across the lanes of one wave.  L = min(ns, 64) lanes per codeword,
// G = 64 / L codewords per wave, SPL = ns / L (1 or 2) states per lane; state s lives in lane (s mod 64) of its
// codeword's lane group, register slot s / 64.  One wave per workgroup.  The channel LLRs (and a priori LLRs) of the
// next kCh trellis steps of every codeword of the wave are staged in LDS by coalesced loads.
//
// The order of operations is the specification of tests/conv_f32.py:
//   branch metrics summed over conv_n in index order; Viterbi: cm[from] + bm, ties to the first predecessor of
//   from_nodes; sums over the states of a codeword (the map normalisation, the LLR sums) and the log-sum-exp sums over
//   states are the halving fold x[:h] + x[h:] (for two slots per lane the in-lane add first, then xor butterflies of
//   the lane offsets L/2 .. 1); exp / log of the float32 kernels are float64 exp / log rounded once to float32.
#include <math.h>
#include <string.h>

#include <vector>

#include "bcjr_core.h"
#include "common.h"

namespace samd {
namespace {

constexpr size_t kVitLdsDecBytes = 32768;        // decision words kept in LDS up to this size per wave
constexpr float kLargeDist = 1048576.f;          // LARGEDIST = 2^20 (decoding.py:411)

// ---------------------------------------------------------------- encoder
// Feed-forward: output symbol t is the parity of (u[t] .. u[t-mu]) & poly, u = 0 outside [0, k) (the zero tail of the
// termination, encoding.py:262-290).  One lane per (codeword, symbol).
template <typename R>
__global__ void conv_encode_ff_kernel(const R* __restrict__ u, int64_t batch, int k, int T, Trellis tr, R* __restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * (int64_t)T) return;
  const int64_t b = i / T;
  const int t = (int)(i - b * T);
  const R* ub = u + b * (int64_t)k;
  uint32_t sbits = 0;
  for (int d = 0; d <= tr.mu; ++d) {
    const int x = t - d;
    const uint32_t bit = (x >= 0 && x < k) ? ((uint32_t)(int)ub[x] & 1u) : 0u;
    sbits |= bit << (tr.mu - d);
  }
  R* cb = c + b * (int64_t)T * tr.conv_n + (int64_t)t * tr.conv_n;
  for (int p = 0; p < tr.conv_n; ++p) cb[p] = (R)(__popc(sbits & tr.poly[p]) & 1);
}

// Recursive systematic: serial per codeword, the register in a register; the termination feeds the feedback bit
// (encoding.py:270-281) so that the register input is 0.
template <typename R>
__global__ void conv_encode_rsc_kernel(const R* __restrict__ u, int64_t batch, int k, int T, Trellis tr, R* __restrict__ c) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const R* ub = u + b * (int64_t)k;
  R* cb = c + b * (int64_t)T * tr.conv_n;
  const uint32_t mask = (uint32_t)tr.ns - 1u;
  uint32_t st = 0;
  for (int t = 0; t < T; ++t) {
    const uint32_t fb = __popc(st & tr.poly[0] & mask) & 1u;
    const uint32_t nb = t < k ? (((uint32_t)(int)ub[t] & 1u) ^ fb) : 0u;
    const uint32_t sbits = (nb << tr.mu) | st;
    for (int p = 0; p < tr.conv_n; ++p) cb[(int64_t)t * tr.conv_n + p] = (R)(__popc(sbits & tr.poly[p]) & 1);
    st = sbits >> 1;
  }
}

// ---------------------------------------------------------------- decoder helpers (exp / log, folds: bcjr_core.h)
// Stages steps [t0, t0 + kCh) of the wave's codewords: y[g][e] channel values (e < kCh * conv_n), a[g][j] a priori.
// hard: int_mod_2 (fec/utils.py:1255-1262) applied on the way in.
template <typename R>
__device__ __forceinline__ void stage(const R* __restrict__ y, const R* __restrict__ la, int64_t cw, bool valid, int n,
                                      int T, int t0, int conv_n, int L, int sl, R* ys, R* as, bool hard) {
  const int e0 = t0 * conv_n, E = kCh * conv_n;
  for (int e = sl; e < E; e += L) {
    R v = (R)0;
    if (valid && e0 + e < n) {
      v = y[cw * (int64_t)n + e0 + e];
      if (hard) {
        const R r = fabs(rint(v));
        v = r - (R)2 * floor(r / (R)2);
      }
    }
    ys[e] = v;
  }
  if (as) {
    for (int j = sl; j < kCh; j += L) as[j] = (valid && la && t0 + j < T) ? la[cw * (int64_t)T + t0 + j] : (R)0;
  }
}

// Viterbi branch metric of output symbol o at one step (decoding.py:350-386; soft: inputs negated at :417)
template <typename R>
__device__ __forceinline__ R vit_bm(const R* ys, int conv_n, int o, bool hard) {
  R acc = (R)0;
  for (int j = 0; j < conv_n; ++j) {
    const int bit = (o >> (conv_n - 1 - j)) & 1;
    const R x = ys[j];
    const R v = hard ? fabs(x - (R)bit) : (bit ? -x : x);
    acc = j == 0 ? v : acc + v;
  }
  return acc;
}

// ---------------------------------------------------------------- Viterbi
template <typename R, int SPL>
__global__ void __launch_bounds__(64) conv_viterbi_kernel(const R* __restrict__ y, int64_t batch, int n, int T, int k,
                                                           Trellis tr, int hard, int terminate, int info_bits,
                                                           R* __restrict__ out, uint64_t* __restrict__ ws_dec) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int ns = tr.ns, conv_n = tr.conv_n;
  const int L = ns < 64 ? ns : 64, G = 64 / L;
  const int lane = threadIdx.x, g = lane / L, sl = lane % L, g0 = g * L;
  const int64_t cw = (int64_t)blockIdx.x * G + g;
  const bool valid = cw < batch;
  R* ybuf = (R*)smem;                                               // [G][kCh * conv_n]
  uint8_t* tb_from = (uint8_t*)(ybuf + G * kCh * conv_n);           // [ns][2]
  uint8_t* tb_to = tb_from + 2 * kMaxStates;                        // [ns][2]
  uint8_t* tb_op = tb_to + 2 * kMaxStates;                          // [ns][2] op_by_fromnode
  uint64_t* dec = ws_dec ? ws_dec + (int64_t)blockIdx.x * T * SPL
                         : (uint64_t*)(smem + ((G * kCh * conv_n * sizeof(R) + 6 * kMaxStates + 7) & ~(size_t)7));
  for (int i = lane; i < 2 * ns; i += 64) {
    tb_from[i] = (&tr.from[0][0])[i];
    tb_to[i] = (&tr.to[0][0])[i];
    tb_op[i] = (&tr.op_from[0][0])[i];
  }
  int f[SPL][2], o[SPL][2];
  R cm[SPL];
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int s = sl + 64 * q;
    f[q][0] = tr.from[s][0];
    f[q][1] = tr.from[s][1];
    o[q][0] = tr.op_to[s][0];
    o[q][1] = tr.op_to[s][1];
    cm[q] = s == 0 ? (R)0 : (R)kLargeDist;
  }
  R* ys = ybuf + g * kCh * conv_n;
  for (int t0 = 0; t0 < T; t0 += kCh) {
    __syncthreads();
    stage<R>(y, nullptr, cw, valid, n, T, t0, conv_n, L, sl, ys, nullptr, hard != 0);
    __syncthreads();
    const int te = T - t0 < kCh ? T - t0 : kCh;
    for (int tt = 0; tt < te; ++tt) {
      const R* yt = ys + tt * conv_n;
      R nc[SPL];
      uint64_t bal[SPL];
#pragma unroll
      for (int q = 0; q < SPL; ++q) {
        const R p0 = state_val<R, SPL>(cm, g0, f[q][0]);
        const R p1 = state_val<R, SPL>(cm, g0, f[q][1]);
        const R m0 = p0 + vit_bm<R>(yt, conv_n, o[q][0], hard != 0);
        const R m1 = p1 + vit_bm<R>(yt, conv_n, o[q][1], hard != 0);
        const bool d = m1 < m0;                                     // argmin: first minimum
        nc[q] = d ? m1 : m0;
        bal[q] = __ballot(d);
      }
#pragma unroll
      for (int q = 0; q < SPL; ++q) {
        cm[q] = nc[q];
        if (lane == 0) dec[(int64_t)(t0 + tt) * SPL + q] = bal[q];
      }
    }
  }
  // start of the traceback: state 0 when terminated, else the first minimum of the last metrics (decoding.py:334-337)
  R bv = cm[0];
  int bi = sl;
  if (SPL == 2 && cm[SPL - 1] < bv) { bv = cm[SPL - 1]; bi = sl + 64; }
  for (int off = L >> 1; off >= 1; off >>= 1) {
    const R ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  __syncthreads();
  if (!valid || sl != 0) return;
  int cur = terminate ? 0 : bi;
  R* ob = out + cw * (int64_t)(info_bits ? k : n);
  for (int t = T - 1; t >= 0; --t) {
    int prev = 0;
    if (t > 0) {
      const uint64_t w = dec[(int64_t)t * SPL + (cur >> 6)];
      const int d = (int)((w >> (g0 + (cur & 63))) & 1ull);
      prev = tb_from[2 * cur + d];
    }
    // _op_bits_path (decoding.py:275-320): input bit and output symbol of the transition prev -> cur
    const bool m0 = tb_to[2 * prev] == cur, m1 = tb_to[2 * prev + 1] == cur;
    if (info_bits) {
      if (t < k) ob[t] = m1 ? (R)1 : (R)0;
    } else {
      const int sym = m0 ? tb_op[2 * prev] : (m1 ? tb_op[2 * prev + 1] : 0);
      for (int j = 0; j < conv_n; ++j) ob[(int64_t)t * conv_n + j] = (R)((sym >> (conv_n - 1 - j)) & 1);
    }
    cur = prev;
  }
}

// ---------------------------------------------------------------- BCJR (bcjr_gamma, comb2: bcjr_core.h)
template <typename R, int ALG, int SPL>
__global__ void __launch_bounds__(64) conv_bcjr_kernel(const R* __restrict__ llr_ch, const R* __restrict__ llr_a,
                                                        int64_t batch, int n, int T, int k, Trellis tr, int terminate,
                                                        int hard_out, R beta_eq, R* __restrict__ out, R* __restrict__ ws_alpha) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int ns = tr.ns, conv_n = tr.conv_n;
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
    alpha[q] = s == 0 ? one : zero;                            // _initialize (decoding.py:682-698)
    beta[q] = terminate ? alpha[q] : beta_eq;
  }
  // forward recursion (_update_fwd, decoding.py:700-790): alpha_t stored before step t
  for (int t0 = 0; t0 < T; t0 += kCh) {
    __syncthreads();
    stage<R>(llr_ch, llr_a, cw, valid, n, T, t0, conv_n, L, sl, ys, as, false);
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
  // backward recursion and output LLRs (_update_bwd, decoding.py:792-880)
  const int nchunks = (T + kCh - 1) / kCh;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int t0 = c * kCh;
    __syncthreads();
    stage<R>(llr_ch, llr_a, cw, valid, n, T, t0, conv_n, L, sl, ys, as, false);
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
        const R m = -llr;                                         // back to log p(1)/p(0) (decoding.py:934)
        out[cw * (int64_t)k + t] = hard_out ? ((R)0 < m ? (R)1 : (R)0) : m;
      }
    }
  }
}

// ---------------------------------------------------------------- host side
size_t vit_dec_bytes(int ns, int T) { return (size_t)T * (size_t)(ns > 64 ? 2 : 1) * 8; }

size_t workspace_bytes(int decoder, int constraint_length, int num_syms, int64_t batch, int dbl) {
  if (constraint_length < 3 || constraint_length > 8 || num_syms < 0 || batch < 0) return 0;
  const int ns = 1 << (constraint_length - 1);
  const Shape sh = shape_of(ns, batch);
  const size_t per = decoder == 0 ? vit_dec_bytes(ns, num_syms) : bcjr_alpha_bytes(ns, num_syms, dbl);
  const size_t cap = decoder == 0 ? kVitLdsDecBytes : kBcjrLdsAlphaBytes;
  return per <= cap ? 0 : per * (size_t)sh.waves;
}

int check_common(int64_t batch, int n, int conv_n, int T, int terminate, int mu) {
  SAMD_REQUIRE(batch >= 0 && n >= 0, "conv: invalid dimensions");
  SAMD_REQUIRE(n % conv_n == 0, "conv: n must be divisible by the number of generator polynomials");
  SAMD_REQUIRE(!terminate || T >= mu, "conv: terminated codeword shorter than its tail");
  return SAMD_OK;
}

template <typename R>
int encode(const R* u, int64_t batch, int k, const uint32_t* polys, int conv_n, int constraint_length, int rsc,
           int terminate, R* c, void* stream) {
  Trellis tr;
  int rc = build_trellis(polys, conv_n, constraint_length, rsc, &tr);
  if (rc != SAMD_OK) return rc;
  SAMD_REQUIRE(batch >= 0 && k >= 0, "ConvEncoder: invalid dimensions");
  const int T = k + (terminate ? tr.mu : 0);               // k = 0 terminated: the mu tail symbols are still written
  if (batch == 0 || T == 0) return SAMD_OK;
  SAMD_REQUIRE(u && c, "null argument");
  hipStream_t s = (hipStream_t)stream;
  if (!rsc) {
    const int64_t total = batch * (int64_t)T;
    SAMD_REQUIRE((total + 255) / 256 <= 0x7fffffff, "ConvEncoder: too many symbols for one launch");
    hipLaunchKernelGGL(conv_encode_ff_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, u, batch, k, T, tr, c);
  } else {
    SAMD_REQUIRE((batch + 255) / 256 <= 0x7fffffff, "ConvEncoder: batch too large for one launch");
    hipLaunchKernelGGL(conv_encode_rsc_kernel<R>, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, u, batch, k, T, tr, c);
  }
  return launch_status();
}

template <typename R>
int viterbi(const R* y, int64_t batch, int n, const uint32_t* polys, int conv_n, int constraint_length, int rsc,
            int terminate, int method, int info_bits, R* out, void* ws, size_t ws_bytes, void* stream) {
  Trellis tr;
  int rc = build_trellis(polys, conv_n, constraint_length, rsc, &tr);
  if (rc != SAMD_OK) return rc;
  SAMD_REQUIRE(method == 0 || method == 1, "ViterbiDecoder: method 0 (soft_llr) or 1 (hard)");
  const int T = n / conv_n, k = T - (terminate ? tr.mu : 0);
  rc = check_common(batch, n, conv_n, T, terminate, tr.mu);
  if (rc != SAMD_OK) return rc;
  if (batch == 0 || T == 0) return SAMD_OK;
  SAMD_REQUIRE(y && out, "null argument");
  const Shape sh = shape_of(tr.ns, batch);
  SAMD_REQUIRE(sh.waves <= 0x7fffffff, "ViterbiDecoder: batch too large for one launch");
  const size_t need = workspace_bytes(0, constraint_length, T, batch, 0);
  if (need) {
    SAMD_REQUIRE(ws != nullptr, "ViterbiDecoder: workspace required (samd_conv_workspace_bytes)");
    if (ws_bytes < need) {
      set_error("ViterbiDecoder: workspace too small");
      return SAMD_ERR_WORKSPACE;
    }
  }
  const size_t head = align_up((size_t)sh.G * kCh * conv_n * sizeof(R) + 6 * kMaxStates, 8);
  const size_t lds = head + (need ? 0 : vit_dec_bytes(tr.ns, T));
  hipStream_t s = (hipStream_t)stream;
  uint64_t* wsd = need ? (uint64_t*)ws : nullptr;
#define SAMD_VIT(SPL)                                                                                         \
  {                                                                                                           \
    SAMD_SET_MAX_LDS((conv_viterbi_kernel<R, SPL>), (int)lds);                                                \
    hipLaunchKernelGGL((conv_viterbi_kernel<R, SPL>), dim3((unsigned)sh.waves), dim3(64), lds, s, y, batch, n, T, k, tr, \
                       method, terminate, info_bits, out, wsd);                                               \
  }
  if (sh.SPL == 1) SAMD_VIT(1) else SAMD_VIT(2)
#undef SAMD_VIT
  return launch_status();
}

template <typename R>
int bcjr(const R* llr_ch, const R* llr_a, int64_t batch, int n, const uint32_t* polys, int conv_n, int constraint_length,
         int rsc, int terminate, int algorithm, int hard_out, R* out, void* ws, size_t ws_bytes, void* stream) {
  Trellis tr;
  int rc = build_trellis(polys, conv_n, constraint_length, rsc, &tr);
  if (rc != SAMD_OK) return rc;
  SAMD_REQUIRE(algorithm >= 0 && algorithm <= 2, "BCJRDecoder: algorithm 0 (map), 1 (log) or 2 (maxlog)");
  const int T = n / conv_n, k = T - (terminate ? tr.mu : 0);
  rc = check_common(batch, n, conv_n, T, terminate, tr.mu);
  if (rc != SAMD_OK) return rc;
  if (batch == 0 || T == 0) return SAMD_OK;
  SAMD_REQUIRE(llr_ch && out, "null argument");
  const Shape sh = shape_of(tr.ns, batch);
  SAMD_REQUIRE(sh.waves <= 0x7fffffff, "BCJRDecoder: batch too large for one launch");
  const int dbl = sizeof(R) == 8;
  const size_t need = workspace_bytes(1, constraint_length, T, batch, dbl);
  if (need) {
    SAMD_REQUIRE(ws != nullptr, "BCJRDecoder: workspace required (samd_conv_workspace_bytes)");
    if (ws_bytes < need) {
      set_error("BCJRDecoder: workspace too small");
      return SAMD_ERR_WORKSPACE;
    }
  }
  // eq_prob of the unterminated beta init (decoding.py:689-694), float64 then cast
  const double eq = 1.0 / tr.ns;
  const R beta_eq = (R)(algorithm == kMap ? eq : std::log(eq));
  const size_t lds = (size_t)sh.G * kCh * (conv_n + 1) * sizeof(R) + (need ? 0 : bcjr_alpha_bytes(tr.ns, T, dbl));
  hipStream_t s = (hipStream_t)stream;
  R* wsa = need ? (R*)ws : nullptr;
#define SAMD_BCJR(A_, S_)                                                                                   \
  if (algorithm == A_ && sh.SPL == S_) {                                                                    \
    SAMD_SET_MAX_LDS((conv_bcjr_kernel<R, A_, S_>), (int)lds);                                              \
    hipLaunchKernelGGL((conv_bcjr_kernel<R, A_, S_>), dim3((unsigned)sh.waves), dim3(64), lds, s, llr_ch, llr_a, batch, \
                       n, T, k, tr, terminate, hard_out, beta_eq, out, wsa);                                  \
    return launch_status();                                                                                   \
  }
  SAMD_BCJR(kMap, 1) SAMD_BCJR(kMap, 2) SAMD_BCJR(kLog, 1) SAMD_BCJR(kLog, 2) SAMD_BCJR(kMaxLog, 1) SAMD_BCJR(kMaxLog, 2)
#undef SAMD_BCJR
  set_error("BCJRDecoder: no instantiation");
  return SAMD_ERR_INVALID;
}

}  // namespace
}  // namespace samd

extern "C" int samd_conv_encode_f32(const float* u, int64_t batch, int k, const uint32_t* polys, int conv_n,
                                    int constraint_length, int rsc, int terminate, float* c, void* stream) {
  return samd::encode<float>(u, batch, k, polys, conv_n, constraint_length, rsc, terminate, c, stream);
}
extern "C" int samd_conv_encode_f64(const double* u, int64_t batch, int k, const uint32_t* polys, int conv_n,
                                    int constraint_length, int rsc, int terminate, double* c, void* stream) {
  return samd::encode<double>(u, batch, k, polys, conv_n, constraint_length, rsc, terminate, c, stream);
}
extern "C" size_t samd_conv_workspace_bytes(int decoder, int constraint_length, int num_syms, int64_t batch, int dbl) {
  return samd::workspace_bytes(decoder, constraint_length, num_syms, batch, dbl);
}
extern "C" int samd_conv_viterbi_f32(const float* y, int64_t batch, int n, const uint32_t* polys, int conv_n,
                                     int constraint_length, int rsc, int terminate, int method, int return_info_bits,
                                     float* out, void* workspace, size_t workspace_bytes, void* stream) {
  return samd::viterbi<float>(y, batch, n, polys, conv_n, constraint_length, rsc, terminate, method, return_info_bits, out,
                              workspace, workspace_bytes, stream);
}
extern "C" int samd_conv_viterbi_f64(const double* y, int64_t batch, int n, const uint32_t* polys, int conv_n,
                                     int constraint_length, int rsc, int terminate, int method, int return_info_bits,
                                     double* out, void* workspace, size_t workspace_bytes, void* stream) {
  return samd::viterbi<double>(y, batch, n, polys, conv_n, constraint_length, rsc, terminate, method, return_info_bits, out,
                               workspace, workspace_bytes, stream);
}
extern "C" int samd_conv_bcjr_f32(const float* llr_ch, const float* llr_a, int64_t batch, int n, const uint32_t* polys,
                                  int conv_n, int constraint_length, int rsc, int terminate, int algorithm, int hard_out,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
  return samd::bcjr<float>(llr_ch, llr_a, batch, n, polys, conv_n, constraint_length, rsc, terminate, algorithm, hard_out,
                           out, workspace, workspace_bytes, stream);
}
extern "C" int samd_conv_bcjr_f64(const double* llr_ch, const double* llr_a, int64_t batch, int n, const uint32_t* polys,
                                  int conv_n, int constraint_length, int rsc, int terminate, int algorithm, int hard_out,
                                  double* out, void* workspace, size_t workspace_bytes, void* stream) {
  return samd::bcjr<double>(llr_ch, llr_a, batch, n, polys, conv_n, constraint_length, rsc, terminate, algorithm, hard_out,
                            out, workspace, workspace_bytes, stream);
}
