// Post-equalisation SINR of every stream after LMMSE combining - LMMSEPostEqualizationSINR.call
// (ofdm/equalization.py:800-839) with the helpers of PostEqualizationSINR (:571-752), inv_cholesky
// (utils/linalg.py:8-32) and the s=None branch of lmmse_matrix (mimo/equalization.py:91-97) fused into one launch.
//
// One lane per item (b, rx, t, fe), fe fastest, so that every load of a wave is contiguous.  The order of operations
// is the specification of tests/precoded_channel_f32.py, every sum in ascending index order starting from zero, no
// contraction (-ffp-contract=off), |z|^2 = re*re + im*im:
//   Hd [RXA, S]  the receiver's desired columns, gathered through detection_desired_ind (flat over [rx, tx, stream]);
//   V_ij = sum_u Hu_iu conj(Hu_ju) (j <= i) streamed over the U undesired columns (with interference whitening, else
//          0), then V_ii.re += no_i;  V = L L^H (chol of csrc/cx_linalg.h, in the order stated there);
//   Li = L^-1 by forward substitution of the identity: Li_ic = ((i == c) - sum_{c <= q < i} L_iq Li_qc) * (1 / L_ii);
//   Hw = Li Hd:  Hw_is = sum_{q <= i} Li_iq Hd_qs;
//   A_ab = (a == b) + sum_i conj(Hw_ia) Hw_ib (b <= a);  A = C C^H;  F = C^-H C^-1 Hw^H (forward, then backward
//          substitution in the order of cx_linalg.h, each row times the reciprocal of C_ii);
//   signal_s = |sum_a F_sa Hw_as|^2;
//   total_s  = sum_c |sum_a F_sa w_ac|^2 over the S desired and then the U undesired columns, each undesired column
//          whitened on the fly (w = Li hu) whether or not it entered V, as the reference does;
//   interference_s = max(total_s - signal_s, 0);  noise_s = sum_a |F_sa|^2;
//   sinr_s = signal_s / (interference_s + noise_s), 0 where the denominator is 0 (divide_no_nan).
// (RXA, S) in (1,1) (2,1) (2,2) (4,2) (4,4) are compiled with constant sizes (arrays in registers, loops unrolled);
// the rest of RXA <= 16, S <= 16 runs one run-time-size instantiation with its arrays in scratch.  U has no cap.
#include "common.h"
#include "cx_linalg.h"

namespace samd {
namespace {

constexpr int kD = 16, kBlock = 128;

template <typename R> struct SinrArgs {
  const R* heff;       // [B, RX, RXA, TX, K, T, Fe] complex (the estimate when one is given)
  const R* no;         // [B, RX, RXA, T, Fe] or nullptr (no0 everywhere)
  R no0;
  const int* desired;  // [RX, S] flat indices over [rx, tx, stream] (StreamManagement.detection_desired_ind)
  const int* undesired;  // [RX, U] (detection_undesired_ind); unused when U == 0
  R* sinr;             // [B, T, Fe, RX, S]
  int64_t n;           // B * RX * T * Fe
  int RX, RXA, TXK, T, Fe, S, U, whiten;
};

template <typename R, int AT, int ST> __global__ __launch_bounds__(kBlock) void lmmse_sinr_kernel(SinrArgs<R> p) {
  const int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= p.n) return;
  constexpr int AA = AT ? AT : kD, SA = ST ? ST : kD;
  const int RA = AT ? AT : p.RXA, S = ST ? ST : p.S;
  constexpr int UR = AT && ST ? 32 : 1;
  const int64_t TFe = (int64_t)p.T * p.Fe;
  const int64_t tfe = it % TFe;
  const int64_t brx = it / TFe;                         // b * RX + rx
  const int rx = (int)(brx % p.RX);
  const int64_t b = brx / p.RX;
  // column q (flat over [rx, tx, stream]) of the effective channel, antenna a: h_eff[b, q / TXK, a, q % TXK, t, fe]
  auto hidx = [&](int q, int a) -> int64_t {
    return (((b * p.RX + q / p.TXK) * RA + a) * p.TXK + q % p.TXK) * TFe + tfe;
  };

  cx<R> Hd[AA * SA], V[AA * AA], Li[AA * AA], A[SA * SA], G[SA * AA], hu[AA];
  R total[SA], signal[SA];
#pragma unroll UR
  for (int s = 0; s < S; ++s) {
    const int q = p.desired[rx * S + s];
#pragma unroll UR
    for (int a = 0; a < RA; ++a) Hd[a * S + s] = ld(p.heff, hidx(q, a));
  }
  // interference-plus-noise covariance (lower triangle)
#pragma unroll UR
  for (int i = 0; i < RA; ++i)
#pragma unroll UR
    for (int j = 0; j <= i; ++j) V[i * RA + j] = C<R>(R(0), R(0));
  if (p.whiten)
    for (int u = 0; u < p.U; ++u) {
      const int q = p.undesired[rx * p.U + u];
#pragma unroll UR
      for (int a = 0; a < RA; ++a) hu[a] = ld(p.heff, hidx(q, a));
#pragma unroll UR
      for (int i = 0; i < RA; ++i)
#pragma unroll UR
        for (int j = 0; j <= i; ++j) V[i * RA + j] = V[i * RA + j] + mulcj(hu[i], hu[j]);
    }
#pragma unroll UR
  for (int i = 0; i < RA; ++i)
    V[i * RA + i].re = V[i * RA + i].re + (p.no ? p.no[(brx * RA + i) * TFe + tfe] : p.no0);
  chol<R, AT>(V, RA);
  // Li = L^-1 (lower triangle)
#pragma unroll UR
  for (int c = 0; c < RA; ++c)
#pragma unroll UR
    for (int i = c; i < RA; ++i) {
      cx<R> v = C<R>(i == c ? R(1) : R(0), R(0));
#pragma unroll UR
      for (int q = c; q < i; ++q) v = v - V[i * RA + q] * Li[q * RA + c];
      Li[i * RA + c] = sc(v, R(1) / V[i * RA + i].re);
    }
  // Hd <- Li Hd, rows from the last to the first (row i needs rows q <= i of the unwhitened matrix)
#pragma unroll UR
  for (int s = 0; s < S; ++s)
#pragma unroll UR
    for (int i = RA - 1; i >= 0; --i) {
      cx<R> v = C<R>(R(0), R(0));
#pragma unroll UR
      for (int q = 0; q <= i; ++q) v = v + Li[i * RA + q] * Hd[q * S + s];
      Hd[i * S + s] = v;
    }
  // F = (Hw^H Hw + I)^-1 Hw^H through a Cholesky solve; G[a * RA + i] = F_ai
#pragma unroll UR
  for (int a = 0; a < S; ++a)
#pragma unroll UR
    for (int c = 0; c <= a; ++c) {
      cx<R> v = C<R>(a == c ? R(1) : R(0), R(0));
#pragma unroll UR
      for (int i = 0; i < RA; ++i) v = v + cjm(Hd[i * S + a], Hd[i * S + c]);
      A[a * S + c] = v;
    }
  chol<R, ST>(A, S);
  // column i of Hw^H: the substitutions of cx_linalg.h written out, the forward one reading conj(Hd) in place of a
  // copy (through fwd / bwd the run-time-size kernel stores and reloads every column first and runs 1.6 % longer)
#pragma unroll UR
  for (int i = 0; i < RA; ++i) {
#pragma unroll UR
    for (int a = 0; a < S; ++a) {
      cx<R> v = C<R>(Hd[i * S + a].re, -Hd[i * S + a].im);
#pragma unroll UR
      for (int q = 0; q < a; ++q) v = v - A[a * S + q] * G[q * RA + i];
      G[a * RA + i] = sc(v, R(1) / A[a * S + a].re);
    }
#pragma unroll UR
    for (int a = S - 1; a >= 0; --a) {
      cx<R> v = G[a * RA + i];
#pragma unroll UR
      for (int q = a + 1; q < S; ++q) v = v - cjm(A[q * S + a], G[q * RA + i]);
      G[a * RA + i] = sc(v, R(1) / A[a * S + a].re);
    }
  }
  // signal, then the total over the desired and the (whitened on the fly) undesired columns
#pragma unroll UR
  for (int s = 0; s < S; ++s) {
    cx<R> v = C<R>(R(0), R(0));
#pragma unroll UR
    for (int a = 0; a < RA; ++a) v = v + G[s * RA + a] * Hd[a * S + s];
    signal[s] = abs2(v);
    total[s] = R(0);
  }
#pragma unroll UR
  for (int c = 0; c < S; ++c)
#pragma unroll UR
    for (int s = 0; s < S; ++s) {
      cx<R> v = C<R>(R(0), R(0));
#pragma unroll UR
      for (int a = 0; a < RA; ++a) v = v + G[s * RA + a] * Hd[a * S + c];
      total[s] = total[s] + abs2(v);
    }
  for (int u = 0; u < p.U; ++u) {
    const int q = p.undesired[rx * p.U + u];
#pragma unroll UR
    for (int a = 0; a < RA; ++a) hu[a] = ld(p.heff, hidx(q, a));
#pragma unroll UR
    for (int i = RA - 1; i >= 0; --i) {
      cx<R> v = C<R>(R(0), R(0));
#pragma unroll UR
      for (int k = 0; k <= i; ++k) v = v + Li[i * RA + k] * hu[k];
      hu[i] = v;
    }
#pragma unroll UR
    for (int s = 0; s < S; ++s) {
      cx<R> v = C<R>(R(0), R(0));
#pragma unroll UR
      for (int a = 0; a < RA; ++a) v = v + G[s * RA + a] * hu[a];
      total[s] = total[s] + abs2(v);
    }
  }
  const int64_t t_fe = tfe;                              // t * Fe + fe
  const int64_t obase = ((b * TFe + t_fe) * p.RX + rx) * S;
#pragma unroll UR
  for (int s = 0; s < S; ++s) {
    R interference = total[s] - signal[s];
    interference = interference > R(0) ? interference : R(0);
    R noise = R(0);
#pragma unroll UR
    for (int a = 0; a < RA; ++a) noise = noise + abs2(G[s * RA + a]);
    const R den = interference + noise;
    p.sinr[obase + s] = den == R(0) ? R(0) : signal[s] / den;
  }
}

// the compile-time (RXA, S) instantiations; every other RXA <= 16, S <= 16 takes the run-time-size path
#define SAMD_SINR_SHAPES(X) X(1, 1) X(2, 1) X(2, 2) X(4, 2) X(4, 4)

inline unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

template <typename R>
int lmmse_sinr(const R* h_eff, const R* no, R no0, const int32_t* desired_ind, const int32_t* undesired_ind, int whiten,
               int batch, int num_rx, int num_rx_ant, int num_tx, int num_streams_per_tx, int num_ofdm_symbols, int num_eff_sc,
               int num_streams_per_rx, int num_interfering, R* sinr, void* stream) {
  SAMD_REQUIRE(h_eff && desired_ind && sinr, "null argument");
  SAMD_REQUIRE(batch >= 0 && num_rx >= 1 && num_rx_ant >= 1 && num_tx >= 1 && num_streams_per_tx >= 1 && num_ofdm_symbols >= 1 &&
               num_eff_sc >= 0 && num_streams_per_rx >= 1 && num_interfering >= 0, "LMMSEPostEqualizationSINR: invalid dimensions");
  SAMD_REQUIRE(num_rx_ant <= kD && num_streams_per_rx <= kD,
               "LMMSEPostEqualizationSINR: supported up to 16 receive antennas and 16 streams per receiver");
  SAMD_REQUIRE((int64_t)num_tx * num_streams_per_tx == (int64_t)num_streams_per_rx + num_interfering,
               "LMMSEPostEqualizationSINR: desired plus interfering streams must be all num_tx x num_streams_per_tx streams");
  SAMD_REQUIRE(num_interfering == 0 || undesired_ind, "null argument");
  SinrArgs<R> p;
  p.heff = h_eff; p.no = no; p.no0 = no0; p.desired = desired_ind; p.undesired = undesired_ind; p.sinr = sinr;
  p.n = (int64_t)batch * num_rx * num_ofdm_symbols * num_eff_sc;
  p.RX = num_rx; p.RXA = num_rx_ant; p.TXK = num_tx * num_streams_per_tx; p.T = num_ofdm_symbols; p.Fe = num_eff_sc;
  p.S = num_streams_per_rx; p.U = num_interfering; p.whiten = whiten ? 1 : 0;
  SAMD_REQUIRE((p.n + kBlock - 1) / kBlock <= 0x7fffffff, "LMMSEPostEqualizationSINR: too many items for one launch");
  if (p.n == 0) return SAMD_OK;
  hipStream_t s = (hipStream_t)stream;
#define SAMD_SINR_CASE(AA, SS)                                                                               \
  if (p.RXA == AA && p.S == SS) {                                                                            \
    hipLaunchKernelGGL((lmmse_sinr_kernel<R, AA, SS>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);            \
    return launch_status();                                                                                  \
  }
  SAMD_SINR_SHAPES(SAMD_SINR_CASE)
#undef SAMD_SINR_CASE
  hipLaunchKernelGGL((lmmse_sinr_kernel<R, 0, 0>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);
  return launch_status();
}

}  // namespace
}  // namespace samd

using namespace samd;

extern "C" int samd_lmmse_post_eq_sinr_c64(const float* h_eff, const float* no, float no0, const int32_t* desired_ind,
                                           const int32_t* undesired_ind, int interference_whitening, int batch, int num_rx,
                                           int num_rx_ant, int num_tx, int num_streams_per_tx, int num_ofdm_symbols,
                                           int num_eff_sc, int num_streams_per_rx, int num_interfering_streams_per_rx,
                                           float* sinr, void* stream) {
  return lmmse_sinr<float>(h_eff, no, no0, desired_ind, undesired_ind, interference_whitening, batch, num_rx, num_rx_ant, num_tx,
                           num_streams_per_tx, num_ofdm_symbols, num_eff_sc, num_streams_per_rx, num_interfering_streams_per_rx,
                           sinr, stream);
}
extern "C" int samd_lmmse_post_eq_sinr_c128(const double* h_eff, const double* no, double no0, const int32_t* desired_ind,
                                            const int32_t* undesired_ind, int interference_whitening, int batch, int num_rx,
                                            int num_rx_ant, int num_tx, int num_streams_per_tx, int num_ofdm_symbols,
                                            int num_eff_sc, int num_streams_per_rx, int num_interfering_streams_per_rx,
                                            double* sinr, void* stream) {
  return lmmse_sinr<double>(h_eff, no, no0, desired_ind, undesired_ind, interference_whitening, batch, num_rx, num_rx_ant, num_tx,
                            num_streams_per_tx, num_ofdm_symbols, num_eff_sc, num_streams_per_rx, num_interfering_streams_per_rx,
                            sinr, stream);
}
