// Linear precoding at the transmitter: regularised zero forcing and conjugate beamforming.
//   rzf_precoding_matrix / rzf_precoder   mimo/precoding.py:12-88, 157-244   G = V D, V = H^H (H H^H + alpha I)^-1
//   cbf_precoding_matrix                  mimo/precoding.py:91-155           G = H^H D
//   RZFPrecoder.call                      ofdm/precoding.py:118-177          gather of the intended receivers' channels,
//                                         precoding, and the effective channel H_r G at the effective subcarriers
//                                         (_compute_effective_channel :81-116 + RemoveNulledSubcarriers)
//   RZF/CBF/EyePrecodedChannel.call       ofdm/precoding.py:417-446, 486-510, 547-566 (helpers :246-369): G from the
//                                         channel knowledge h_hat (or the identity), column k times sqrt(tx_power_k), and
//                                         the effective channel H_r G from the true h at the effective subcarriers
// D = diag(1 / ||v_k||) normalises every column of G to unit norm; a zero column stays zero (divide_no_nan).
//
// One lane per item (an OFDM resource element (b, tx, t, f), f fastest, so that every load and store of a wave is
// contiguous; or one matrix of the contiguous entry).  The order of operations is the float32 specification of
// tests/precoding_f32.py, with every sum in ascending index order and no contraction (-ffp-contract=off):
//   A_ij = sum_m H_im conj(H_jm) (j <= i), then A_ii.re += alpha;
//   A = L L^H and X = L^-H L^-1 H in the order stated in csrc/cx_linalg.h, column by column (both substitutions of a
//   column before the next).  The complex type is that header's; the factor and the substitutions are written out here:
//   called as chol / fwd / bwd, the same operations compile to other schedules that cost several constant-size kernels
//   registers, scratch or occupancy.
//   n_k = sqrt(sum_m (re^2 + im^2) of X_km);  G_mk = conj(X_km) / n_k as two divisions (0 where n_k == 0);
//   x_precoded_m = sum_k G_mk x_k;  h_eff[r, a, k] = sum_m H_r[a, m] G_mk.
// (K, M) pairs that occur in practice are compiled with constant sizes (arrays in registers, loops unrolled); the rest of
// K <= 16, M <= 32 runs one run-time-size instantiation with its arrays in scratch and its loops rolled.
#include "common.h"
#include "cx_linalg.h"

namespace samd {
namespace {

constexpr int kKMax = 16, kMMax = 32, kBlock = 128;
constexpr int kModeRzf = 0, kModeCbf = 1;
constexpr int kModeEye = 2;                              // precoded channels only: G = I (K == M)

// X [K, M] (row stride M) holds the channel H on entry.  On exit X[k * M + m] = G[m][k], the normalised precoding
// matrix stored transposed.  A: K x K workspace.  KT / MT > 0: compile-time sizes.
template <typename R, int KT, int MT>
__device__ __forceinline__ void precoding_matrix(cx<R>* X, cx<R>* A, int k_rt, int m_rt, R alpha, int mode) {
  const int K = KT ? KT : k_rt, M = MT ? MT : m_rt;
  constexpr int U = KT && MT ? 32 : 1;                   // unroll the constant-size loops completely
  if (mode == kModeRzf) {
#pragma unroll U
    for (int i = 0; i < K; ++i)
#pragma unroll U
      for (int j = 0; j <= i; ++j) {
        cx<R> v = C<R>(R(0), R(0));
#pragma unroll U
        for (int m = 0; m < M; ++m) v = v + mulcj(X[i * M + m], X[j * M + m]);
        if (i == j) v.re = v.re + alpha;
        A[i * K + j] = v;
      }
    // lower Cholesky factor in place (the lower triangle of A only); A[j][j].re = L_jj
#pragma unroll U
    for (int j = 0; j < K; ++j) {
      R d = A[j * K + j].re;
#pragma unroll U
      for (int q = 0; q < j; ++q) d = d - (A[j * K + q].re * A[j * K + q].re + A[j * K + q].im * A[j * K + q].im);
      d = sqrt(d);
      A[j * K + j] = C<R>(d, R(0));
      const R inv = R(1) / d;
#pragma unroll U
      for (int i = j + 1; i < K; ++i) {
        cx<R> v = A[i * K + j];
#pragma unroll U
        for (int q = 0; q < j; ++q) v = v - mulcj(A[i * K + q], A[j * K + q]);
        A[i * K + j] = sc(v, inv);
      }
    }
    // X <- L^-1 X, then X <- L^-H X: the solution of A X = H, column by column
#pragma unroll U
    for (int m = 0; m < M; ++m) {
#pragma unroll U
      for (int i = 0; i < K; ++i) {
        cx<R> v = X[i * M + m];
#pragma unroll U
        for (int q = 0; q < i; ++q) v = v - A[i * K + q] * X[q * M + m];
        X[i * M + m] = sc(v, R(1) / A[i * K + i].re);
      }
#pragma unroll U
      for (int i = K - 1; i >= 0; --i) {
        cx<R> v = X[i * M + m];
#pragma unroll U
        for (int q = i + 1; q < K; ++q) v = v - cjm(A[q * K + i], X[q * M + m]);
        X[i * M + m] = sc(v, R(1) / A[i * K + i].re);
      }
    }
  }
  // G = X^H with unit-norm columns
#pragma unroll U
  for (int k = 0; k < K; ++k) {
    R n2 = R(0);
#pragma unroll U
    for (int m = 0; m < M; ++m) n2 = n2 + (X[k * M + m].re * X[k * M + m].re + X[k * M + m].im * X[k * M + m].im);
    const R nrm = sqrt(n2);
#pragma unroll U
    for (int m = 0; m < M; ++m)
      X[k * M + m] = nrm == R(0) ? C<R>(R(0), R(0)) : C<R>(X[k * M + m].re / nrm, -X[k * M + m].im / nrm);
  }
}

// out[m] = sum_k G[m][k] x[k] for the transposed G of precoding_matrix
template <typename R, int KT, int MT>
__device__ __forceinline__ cx<R> precode_row(const cx<R>* Gt, const cx<R>* xv, int K, int M, int m) {
  constexpr int U = KT && MT ? 32 : 1;
  cx<R> v = C<R>(R(0), R(0));
#pragma unroll U
  for (int k = 0; k < (KT ? KT : K); ++k) v = v + Gt[k * (MT ? MT : M) + m] * xv[k];
  return v;
}

// ------------------------------------------------------------------------------------------------------------------
// RZFPrecoder: one lane per resource element (b, tx, t, f)
// ------------------------------------------------------------------------------------------------------------------
template <typename R> struct OfdmPrecodeArgs {
  const R* x;          // [B, TX, K, T, F] complex
  const R* h;          // [B, RX, RXA, TX, M, T, F] complex
  const R* alpha;      // [B, TX, T, F] or nullptr (alpha0 everywhere)
  R alpha0;
  const int* pind;     // [TX, NRXT] receivers served by each transmitter (StreamManagement.precoding_ind)
  const int* fe_of_f;  // [F] index among the effective subcarriers, -1 for a nulled one
  R* xp;               // [B, TX, M, T, F] complex
  R* heff;             // [B, RX, RXA, TX, K, T, Fe] complex, or nullptr
  int64_t n;           // B * TX * T * F
  int RX, RXA, TX, M, K, NRXT, T, F, Fe;
};

template <typename R, int KT, int MT> __global__ __launch_bounds__(kBlock) void rzf_ofdm_kernel(OfdmPrecodeArgs<R> p) {
  const int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= p.n) return;
  constexpr int KA = KT ? KT : kKMax, MA = MT ? MT : kMMax;
  const int K = KT ? KT : p.K, M = MT ? MT : p.M;
  constexpr int U = KT && MT ? 32 : 1;
  const int64_t TF = (int64_t)p.T * p.F;
  const int64_t tf = it % TF;
  const int64_t btx = it / TF;                          // b * TX + tx
  const int tx = (int)(btx % p.TX);
  const int64_t b = btx / p.TX;
  // channel element h[b, r, a, tx, m, t, f]
  auto hidx = [&](int r, int a, int m) -> int64_t { return ((((b * p.RX + r) * p.RXA + a) * p.TX + tx) * M + m) * TF + tf; };

  cx<R> X[KA * MA], A[KA * KA], xv[KA];
#pragma unroll U
  for (int k = 0; k < K; ++k) {
    const int r = p.pind[tx * p.NRXT + k / p.RXA], a = k % p.RXA;
#pragma unroll U
    for (int m = 0; m < M; ++m) X[k * M + m] = ld(p.h, hidx(r, a, m));
  }
#pragma unroll U
  for (int k = 0; k < K; ++k) xv[k] = ld(p.x, (btx * K + k) * TF + tf);
  const R alpha = p.alpha ? p.alpha[it] : p.alpha0;
  precoding_matrix<R, KT, MT>(X, A, K, M, alpha, kModeRzf);
#pragma unroll U
  for (int m = 0; m < M; ++m) st(p.xp, (btx * M + m) * TF + tf, precode_row<R, KT, MT>(X, xv, K, M, m));
  if (p.heff == nullptr) return;
  const int f = (int)(tf % p.F), t = (int)(tf / p.F);
  const int fe = p.fe_of_f[f];
  if (fe < 0) return;
  const int64_t TFe = (int64_t)p.T * p.Fe, tfe = (int64_t)t * p.Fe + fe;
  for (int r = 0; r < p.RX; ++r)
    for (int a = 0; a < p.RXA; ++a) {
      cx<R> row[MA];
#pragma unroll U
      for (int m = 0; m < M; ++m) row[m] = ld(p.h, hidx(r, a, m));
      const int64_t base = (((b * p.RX + r) * p.RXA + a) * p.TX + tx) * K;
#pragma unroll U
      for (int k = 0; k < K; ++k) {
        cx<R> v = C<R>(R(0), R(0));
#pragma unroll U
        for (int m = 0; m < M; ++m) v = v + row[m] * X[k * M + m];
        st(p.heff, (base + k) * TFe + tfe, v);
      }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// PrecodedChannel (RZF / CBF / identity): one lane per resource element (b, tx, t, f); only h_eff is written
// ------------------------------------------------------------------------------------------------------------------
template <typename R> struct PrecodedChannelArgs {
  const R* h;          // [B, RX, RXA, TX, M, T, F] complex: the true channel, h_eff is formed from it
  const R* h_hat;      // same shape: the channel knowledge G is computed from (may be h; unused in the identity mode)
  const R* alpha;      // [B, TX, T, F] or nullptr (alpha0 everywhere); RZF only
  R alpha0;
  const R* tx_power;   // [B, TX, K, T, F] or nullptr (tx_power0 everywhere)
  R tx_power0;
  const int* pind;     // [TX, NRXT] (StreamManagement.precoding_ind; unused in the identity mode)
  const int* fe_of_f;  // [F] index among the effective subcarriers, -1 for a nulled one
  R* heff;             // [B, RX, RXA, TX, K, T, Fe] complex
  int64_t n;           // B * TX * T * F
  int RX, RXA, TX, M, K, NRXT, T, F, Fe, mode;
};

template <typename R, int KT, int MT>
__global__ __launch_bounds__(kBlock) void precoded_channel_kernel(PrecodedChannelArgs<R> p) {
  const int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= p.n) return;
  constexpr int KA = KT ? KT : kKMax, MA = MT ? MT : kMMax;
  const int K = KT ? KT : p.K, M = MT ? MT : p.M;
  constexpr int U = KT && MT ? 32 : 1;
  const int64_t TF = (int64_t)p.T * p.F;
  const int64_t tf = it % TF;
  const int f = (int)(tf % p.F), t = (int)(tf / p.F);
  const int fe = p.fe_of_f[f];
  if (fe < 0) return;                                   // a nulled subcarrier has no entry in h_eff
  const int64_t btx = it / TF;                          // b * TX + tx
  const int tx = (int)(btx % p.TX);
  const int64_t b = btx / p.TX;
  auto hidx = [&](int r, int a, int m) -> int64_t { return ((((b * p.RX + r) * p.RXA + a) * p.TX + tx) * M + m) * TF + tf; };

  cx<R> X[KA * MA], A[KA * KA];
  if (p.mode == kModeEye) {
#pragma unroll U
    for (int k = 0; k < K; ++k)
#pragma unroll U
      for (int m = 0; m < M; ++m) X[k * M + m] = C<R>(k == m ? R(1) : R(0), R(0));
  } else {
#pragma unroll U
    for (int k = 0; k < K; ++k) {
      const int r = p.pind[tx * p.NRXT + k / p.RXA], a = k % p.RXA;
#pragma unroll U
      for (int m = 0; m < M; ++m) X[k * M + m] = ld(p.h_hat, hidx(r, a, m));
    }
    const R alpha = p.alpha ? p.alpha[it] : p.alpha0;
    precoding_matrix<R, KT, MT>(X, A, K, M, alpha, p.mode);
  }
  // column k of G times sqrt(tx_power[b, tx, k, t, f]): a real square root, then real times complex
#pragma unroll U
  for (int k = 0; k < K; ++k) {
    const R s = sqrt(p.tx_power ? p.tx_power[(btx * K + k) * TF + tf] : p.tx_power0);
#pragma unroll U
    for (int m = 0; m < M; ++m) X[k * M + m] = sc(X[k * M + m], s);
  }
  const int64_t TFe = (int64_t)p.T * p.Fe, tfe = (int64_t)t * p.Fe + fe;
  for (int r = 0; r < p.RX; ++r)
    for (int a = 0; a < p.RXA; ++a) {
      cx<R> row[MA];
#pragma unroll U
      for (int m = 0; m < M; ++m) row[m] = ld(p.h, hidx(r, a, m));
      const int64_t base = (((b * p.RX + r) * p.RXA + a) * p.TX + tx) * K;
#pragma unroll U
      for (int k = 0; k < K; ++k) {
        cx<R> v = C<R>(R(0), R(0));
#pragma unroll U
        for (int m = 0; m < M; ++m) v = v + row[m] * X[k * M + m];
        st(p.heff, (base + k) * TFe + tfe, v);
      }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// mimo functions: n independent problems, h [n, K, M] -> g [n, M, K], x [n, K] -> x_precoded [n, M]
// ------------------------------------------------------------------------------------------------------------------
template <typename R> struct MatPrecodeArgs {
  const R* h;
  const R* x;          // or nullptr
  const R* alpha;      // [n] or nullptr
  R alpha0;
  R* g;                // or nullptr
  R* xp;               // or nullptr
  int64_t n;
  int K, M, mode;
};

template <typename R, int KT, int MT> __global__ __launch_bounds__(kBlock) void precoding_matrix_kernel(MatPrecodeArgs<R> p) {
  const int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= p.n) return;
  constexpr int KA = KT ? KT : kKMax, MA = MT ? MT : kMMax;
  const int K = KT ? KT : p.K, M = MT ? MT : p.M;
  constexpr int U = KT && MT ? 32 : 1;
  cx<R> X[KA * MA], A[KA * KA];
#pragma unroll U
  for (int i = 0; i < K * M; ++i) X[i] = ld(p.h, it * K * M + i);
  const R alpha = p.alpha ? p.alpha[it] : p.alpha0;
  precoding_matrix<R, KT, MT>(X, A, K, M, alpha, p.mode);
  if (p.g)
#pragma unroll U
    for (int m = 0; m < M; ++m)
#pragma unroll U
      for (int k = 0; k < K; ++k) st(p.g, (it * M + m) * K + k, X[k * M + m]);
  if (p.xp) {
    cx<R> xv[KA];
#pragma unroll U
    for (int k = 0; k < K; ++k) xv[k] = ld(p.x, it * K + k);
#pragma unroll U
    for (int m = 0; m < M; ++m) st(p.xp, it * M + m, precode_row<R, KT, MT>(X, xv, K, M, m));
  }
}

// the compile-time (K, M) instantiations; every other K <= 16, M <= 32 with K <= M takes the run-time-size path
#define SAMD_PRECODING_SHAPES(X) \
  X(1, 2) X(1, 4) X(1, 8) X(1, 16) X(2, 2) X(2, 4) X(2, 8) X(2, 16) X(4, 4) X(4, 8) X(4, 16) X(8, 8) X(8, 16)

inline unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int check_sizes(int k, int m, int64_t n) {
  SAMD_REQUIRE(k >= 1 && m >= 1, "precoding: K, M >= 1");
  SAMD_REQUIRE(k <= m, "precoding: more streams than transmit antennas (K <= M required)");
  SAMD_REQUIRE(k <= kKMax && m <= kMMax, "precoding: supported up to K = 16 streams and M = 32 transmit antennas");
  SAMD_REQUIRE((n + kBlock - 1) / kBlock <= 0x7fffffff, "precoding: too many items for one launch");
  return SAMD_OK;
}

template <typename R> int rzf_ofdm(const OfdmPrecodeArgs<R>& p, void* stream) {
  SAMD_REQUIRE(p.x && p.h && p.pind && p.fe_of_f && p.xp, "null argument");
  SAMD_REQUIRE(p.n >= 0 && p.RX >= 1 && p.RXA >= 1 && p.TX >= 1 && p.NRXT >= 1 && p.T >= 1 && p.F >= 1 && p.Fe >= 0 &&
               p.Fe <= p.F, "RZFPrecoder: invalid dimensions");
  SAMD_REQUIRE(p.NRXT <= p.RX, "RZFPrecoder: more receivers per transmitter than receivers");
  SAMD_REQUIRE(p.K == p.NRXT * p.RXA, "RZFPrecoder: num_streams_per_tx must equal (receivers per transmitter) x num_rx_ant");
  const int rc = check_sizes(p.K, p.M, p.n);
  if (rc != SAMD_OK) return rc;
  if (p.n == 0) return SAMD_OK;
  hipStream_t s = (hipStream_t)stream;
#define SAMD_PC_CASE(KK, MM)                                                                                 \
  if (p.K == KK && p.M == MM) {                                                                              \
    hipLaunchKernelGGL((rzf_ofdm_kernel<R, KK, MM>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);              \
    return launch_status();                                                                                  \
  }
  SAMD_PRECODING_SHAPES(SAMD_PC_CASE)
#undef SAMD_PC_CASE
  hipLaunchKernelGGL((rzf_ofdm_kernel<R, 0, 0>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);
  return launch_status();
}

template <typename R> int precoding_matrix_launch(const MatPrecodeArgs<R>& p, void* stream) {
  SAMD_REQUIRE(p.h && p.n >= 0, "null argument");
  SAMD_REQUIRE(p.mode == kModeRzf || p.mode == kModeCbf, "precoding: unknown mode");
  SAMD_REQUIRE(p.g || p.xp, "precoding: no output requested");
  SAMD_REQUIRE(!p.xp || p.x, "precoding: x_precoded needs x");
  const int rc = check_sizes(p.K, p.M, p.n);
  if (rc != SAMD_OK) return rc;
  if (p.n == 0) return SAMD_OK;
  hipStream_t s = (hipStream_t)stream;
#define SAMD_PC_CASE(KK, MM)                                                                                 \
  if (p.K == KK && p.M == MM) {                                                                              \
    hipLaunchKernelGGL((precoding_matrix_kernel<R, KK, MM>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);      \
    return launch_status();                                                                                  \
  }
  SAMD_PRECODING_SHAPES(SAMD_PC_CASE)
#undef SAMD_PC_CASE
  hipLaunchKernelGGL((precoding_matrix_kernel<R, 0, 0>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);
  return launch_status();
}

template <typename R> int precoded_channel(const PrecodedChannelArgs<R>& p, void* stream) {
  SAMD_REQUIRE(p.h && p.fe_of_f && p.heff, "null argument");
  SAMD_REQUIRE(p.mode == kModeRzf || p.mode == kModeCbf || p.mode == kModeEye, "PrecodedChannel: unknown mode");
  SAMD_REQUIRE(p.n >= 0 && p.RX >= 1 && p.RXA >= 1 && p.TX >= 1 && p.T >= 1 && p.F >= 1 && p.Fe >= 0 && p.Fe <= p.F,
               "PrecodedChannel: invalid dimensions");
  if (p.mode == kModeEye) {
    SAMD_REQUIRE(p.K == p.M, "EyePrecodedChannel: num_streams_per_tx must equal num_tx_ant");
  } else {
    SAMD_REQUIRE(p.h_hat && p.pind, "null argument");
    SAMD_REQUIRE(p.NRXT >= 1 && p.NRXT <= p.RX, "PrecodedChannel: more receivers per transmitter than receivers");
    SAMD_REQUIRE(p.K == p.NRXT * p.RXA,
                 "PrecodedChannel: num_streams_per_tx must equal (receivers per transmitter) x num_rx_ant");
  }
  const int rc = check_sizes(p.K, p.M, p.n);
  if (rc != SAMD_OK) return rc;
  if (p.n == 0 || p.Fe == 0) return SAMD_OK;
  hipStream_t s = (hipStream_t)stream;
#define SAMD_PC_CASE(KK, MM)                                                                                 \
  if (p.K == KK && p.M == MM) {                                                                              \
    hipLaunchKernelGGL((precoded_channel_kernel<R, KK, MM>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);      \
    return launch_status();                                                                                  \
  }
  SAMD_PRECODING_SHAPES(SAMD_PC_CASE)
#undef SAMD_PC_CASE
  hipLaunchKernelGGL((precoded_channel_kernel<R, 0, 0>), dim3(blocks(p.n)), dim3(kBlock), 0, s, p);
  return launch_status();
}

template <typename R>
int precoded_channel_entry(const R* h, const R* h_hat, const R* alpha, R alpha0, const R* tx_power, R tx_power0,
                           const int32_t* precoding_ind, const int32_t* eff_pos, int mode, int batch, int num_tx,
                           int num_streams, int num_rx, int num_rx_ant, int num_tx_ant, int num_rx_per_tx,
                           int num_ofdm_symbols, int fft_size, int num_eff_sc, R* h_eff, void* stream) {
  SAMD_REQUIRE(batch >= 0, "PrecodedChannel: batch >= 0");
  PrecodedChannelArgs<R> p;
  p.h = h; p.h_hat = h_hat; p.alpha = alpha; p.alpha0 = alpha0; p.tx_power = tx_power; p.tx_power0 = tx_power0;
  p.pind = precoding_ind; p.fe_of_f = eff_pos; p.heff = h_eff; p.mode = mode;
  p.n = (int64_t)batch * num_tx * num_ofdm_symbols * fft_size;
  p.RX = num_rx; p.RXA = num_rx_ant; p.TX = num_tx; p.M = num_tx_ant; p.K = num_streams; p.NRXT = num_rx_per_tx;
  p.T = num_ofdm_symbols; p.F = fft_size; p.Fe = num_eff_sc;
  return precoded_channel<R>(p, stream);
}

template <typename R>
int rzf_ofdm_entry(const R* x, const R* h, const R* alpha, R alpha0, const int32_t* precoding_ind, const int32_t* eff_pos,
                   int batch, int num_tx, int num_streams, int num_rx, int num_rx_ant, int num_tx_ant, int num_rx_per_tx,
                   int num_ofdm_symbols, int fft_size, int num_eff_sc, R* x_precoded, R* h_eff, void* stream) {
  SAMD_REQUIRE(batch >= 0, "RZFPrecoder: batch >= 0");
  OfdmPrecodeArgs<R> p;
  p.x = x; p.h = h; p.alpha = alpha; p.alpha0 = alpha0; p.pind = precoding_ind; p.fe_of_f = eff_pos;
  p.xp = x_precoded; p.heff = h_eff;
  p.n = (int64_t)batch * num_tx * num_ofdm_symbols * fft_size;
  p.RX = num_rx; p.RXA = num_rx_ant; p.TX = num_tx; p.M = num_tx_ant; p.K = num_streams; p.NRXT = num_rx_per_tx;
  p.T = num_ofdm_symbols; p.F = fft_size; p.Fe = num_eff_sc;
  return rzf_ofdm<R>(p, stream);
}

template <typename R>
int matrix_entry(const R* h, const R* x, const R* alpha, R alpha0, int64_t n, int k, int m, int mode, R* g, R* x_precoded,
                 void* stream) {
  MatPrecodeArgs<R> p;
  p.h = h; p.x = x; p.alpha = alpha; p.alpha0 = alpha0; p.g = g; p.xp = x_precoded; p.n = n; p.K = k; p.M = m; p.mode = mode;
  return precoding_matrix_launch<R>(p, stream);
}

}  // namespace
}  // namespace samd

using namespace samd;

extern "C" int samd_rzf_precode_ofdm_c64(const float* x, const float* h, const float* alpha, float alpha0,
                                         const int32_t* precoding_ind, const int32_t* eff_pos, int batch, int num_tx,
                                         int num_streams, int num_rx, int num_rx_ant, int num_tx_ant, int num_rx_per_tx,
                                         int num_ofdm_symbols, int fft_size, int num_eff_sc, float* x_precoded, float* h_eff,
                                         void* stream) {
  return rzf_ofdm_entry<float>(x, h, alpha, alpha0, precoding_ind, eff_pos, batch, num_tx, num_streams, num_rx, num_rx_ant,
                               num_tx_ant, num_rx_per_tx, num_ofdm_symbols, fft_size, num_eff_sc, x_precoded, h_eff, stream);
}
extern "C" int samd_rzf_precode_ofdm_c128(const double* x, const double* h, const double* alpha, double alpha0,
                                          const int32_t* precoding_ind, const int32_t* eff_pos, int batch, int num_tx,
                                          int num_streams, int num_rx, int num_rx_ant, int num_tx_ant, int num_rx_per_tx,
                                          int num_ofdm_symbols, int fft_size, int num_eff_sc, double* x_precoded,
                                          double* h_eff, void* stream) {
  return rzf_ofdm_entry<double>(x, h, alpha, alpha0, precoding_ind, eff_pos, batch, num_tx, num_streams, num_rx, num_rx_ant,
                                num_tx_ant, num_rx_per_tx, num_ofdm_symbols, fft_size, num_eff_sc, x_precoded, h_eff, stream);
}

extern "C" int samd_precoding_matrix_c64(const float* h, const float* x, const float* alpha, float alpha0, int64_t n, int k,
                                         int m, int mode, float* g, float* x_precoded, void* stream) {
  return matrix_entry<float>(h, x, alpha, alpha0, n, k, m, mode, g, x_precoded, stream);
}
extern "C" int samd_precoding_matrix_c128(const double* h, const double* x, const double* alpha, double alpha0, int64_t n,
                                          int k, int m, int mode, double* g, double* x_precoded, void* stream) {
  return matrix_entry<double>(h, x, alpha, alpha0, n, k, m, mode, g, x_precoded, stream);
}

extern "C" int samd_precoded_channel_c64(const float* h, const float* h_hat, const float* alpha, float alpha0,
                                         const float* tx_power, float tx_power0, const int32_t* precoding_ind,
                                         const int32_t* eff_pos, int mode, int batch, int num_tx, int num_streams,
                                         int num_rx, int num_rx_ant, int num_tx_ant, int num_rx_per_tx, int num_ofdm_symbols,
                                         int fft_size, int num_eff_sc, float* h_eff, void* stream) {
  return precoded_channel_entry<float>(h, h_hat, alpha, alpha0, tx_power, tx_power0, precoding_ind, eff_pos, mode, batch,
                                       num_tx, num_streams, num_rx, num_rx_ant, num_tx_ant, num_rx_per_tx, num_ofdm_symbols,
                                       fft_size, num_eff_sc, h_eff, stream);
}
extern "C" int samd_precoded_channel_c128(const double* h, const double* h_hat, const double* alpha, double alpha0,
                                          const double* tx_power, double tx_power0, const int32_t* precoding_ind,
                                          const int32_t* eff_pos, int mode, int batch, int num_tx, int num_streams,
                                          int num_rx, int num_rx_ant, int num_tx_ant, int num_rx_per_tx,
                                          int num_ofdm_symbols, int fft_size, int num_eff_sc, double* h_eff, void* stream) {
  return precoded_channel_entry<double>(h, h_hat, alpha, alpha0, tx_power, tx_power0, precoding_ind, eff_pos, mode, batch,
                                        num_tx, num_streams, num_rx, num_rx_ant, num_tx_ant, num_rx_per_tx, num_ofdm_symbols,
                                        fft_size, num_eff_sc, h_eff, stream);
}
