// PUSCH DMRS least-squares estimates, de-spread, in one launch: what PUSCHLSChannelEstimator does between the received grid
// and the interpolator (nr/pusch_channel_estimation.py:103-169, behind the pilot gather of BaseChannelEstimator.call,
// ofdm/channel_estimation.py:138-173) as a gather, a divide, two splits, two sums, two repeats, a where and three reshapes -
// and, with a nearest-neighbour table, the gather of NearestNeighborInterpolator (ofdm/channel_estimation.py:364-435) on top.
//
//   ls(p)  = y[r, src[s, p]] * coef[s, p]                   coef = 1 / pilot, 0 for a zero pilot: then ls(p) = +0, y is not read
//   t(p)   = (ls(p) + ls(p')) / 2                           dmrs_length 2: p' is the same position in the adjacent DMRS symbol
//          = ls(p)                                          dmrs_length 1
//   h(p)   = (t(g) + t(g + 1) + ... + t(g + n - 1)) / 2     g the first pilot of p's run of n = 2 * num_cdm_groups_without_data
//          = 0                                              where t(p) = 0 (re and im), which depends on the data
//   out[r, s, j] = h(j)              (gather NULL, n_out = num_pilots)
//                = h(gather[s, j])   (gather [S, n_out]: pilot number of the nearest pilot with energy)
//
// Pilots of a stream are numbered row-major: DMRS symbol d = p / pilots_per_symbol, position q = p % pilots_per_symbol.
// Memory-bound.  A lane owns one (stream, output position) for all rows: consecutive lanes are consecutive output positions,
// so stores run along subcarriers, and the sources of neighbouring lanes are the same or neighbouring pilot resource elements
// of one DMRS symbol.  Indices and coefficients of the lane's at most 2 n = 12 sources are read once and stay in registers
// across the grid-stride loop over the rows (blockIdx.z); half of them are zero pilots of the other CDM ports and cost no load.
// Arithmetic (tests/pusch_rx_f32.py, bit-identical): ls re = yr cr - yi ci, im = yr ci + yi cr; the run's sum starts at +0 and
// adds in ascending p; every product, sum and halving is rounded once (-ffp-contract=off).
#include "common.h"

namespace samd {
namespace {

constexpr int kPuschRxThreads = 256;
constexpr int kPuschRxRowCap = 1024;                    // blockIdx.z of one launch; more rows take further trips
constexpr int kPuschRxMaxRun = 6;                       // 2 * num_cdm_groups_without_data, at most 3 CDM groups

template <typename R>
struct alignas(2 * sizeof(R)) CplxRx {                  // one vector load or store per complex value
  R re, im;
};

template <typename R, int N, bool TWO>
__global__ __launch_bounds__(kPuschRxThreads) void pusch_ls_kernel(
    const CplxRx<R>* __restrict__ y, const int32_t* __restrict__ src, const CplxRx<R>* __restrict__ coef,
    const int32_t* __restrict__ gather, int64_t rows, int NP, int PPS, int n_out, int64_t n_in, CplxRx<R>* __restrict__ out) {
  constexpr int M = TWO ? 2 : 1;
  const int j = blockIdx.x * kPuschRxThreads + threadIdx.x, s = blockIdx.y, S = gridDim.y;
  if (j >= n_out) return;
  int p = gather ? gather[(int64_t)s * n_out + j] : j;
  const bool known = p >= 0 && p < NP;                  // a table entry that names no pilot gives zero
  if (!known) p = 0;
  const int d = p / PPS, q = p - d * PPS;
  const int first = (q / N) * N, self = q - first;
  int at[M][N];
  R cr[M][N], ci[M][N];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int64_t base = (int64_t)s * NP + (int64_t)(m == 0 ? d : (d ^ 1)) * PPS + first;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const CplxRx<R> c = coef[base + k];
      const int a = src[base + k];
      cr[m][k] = c.re;
      ci[m][k] = c.im;
      at[m][k] = (known && a >= 0 && a < n_in && (c.re != (R)0 || c.im != (R)0)) ? a : -1;
    }
  }
  for (int64_t r = blockIdx.z; r < rows; r += gridDim.z) {
    const CplxRx<R>* row = y + r * n_in;
    R tr[N], ti[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      R lr[M], li[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        lr[m] = li[m] = (R)0;
        if (at[m][k] >= 0) {
          const CplxRx<R> v = row[at[m][k]];
          lr[m] = v.re * cr[m][k] - v.im * ci[m][k];
          li[m] = v.re * ci[m][k] + v.im * cr[m][k];
        }
      }
      if (TWO) {
        tr[k] = (lr[0] + lr[M - 1]) / (R)2;
        ti[k] = (li[0] + li[M - 1]) / (R)2;
      } else {
        tr[k] = lr[0];
        ti[k] = li[0];
      }
    }
    R sr = (R)0, si = (R)0, mr = (R)0, mi = (R)0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      sr += tr[k];
      si += ti[k];
      if (k == self) {
        mr = tr[k];
        mi = ti[k];
      }
    }
    const bool live = mr != (R)0 || mi != (R)0;
    out[(r * S + s) * (int64_t)n_out + j] = live ? CplxRx<R>{sr / (R)2, si / (R)2} : CplxRx<R>{(R)0, (R)0};
  }
}

template <typename R, int N, bool TWO>
int launch_run(const R* y, const int32_t* src, const R* coef, const int32_t* gather, int64_t rows, int S, int NP, int PPS,
               int n_out, int64_t n_in, R* out, hipStream_t stream) {
  const dim3 grid((unsigned)((n_out + kPuschRxThreads - 1) / kPuschRxThreads), (unsigned)S,
                  (unsigned)(rows < kPuschRxRowCap ? rows : kPuschRxRowCap));
  pusch_ls_kernel<R, N, TWO><<<grid, kPuschRxThreads, 0, stream>>>(
      reinterpret_cast<const CplxRx<R>*>(y), src, reinterpret_cast<const CplxRx<R>*>(coef), gather, rows, NP, PPS, n_out, n_in,
      reinterpret_cast<CplxRx<R>*>(out));
  return launch_status();
}

template <typename R, bool TWO>
int launch_length(const R* y, const int32_t* src, const R* coef, const int32_t* gather, int64_t rows, int S, int NP, int PPS,
                  int N, int n_out, int64_t n_in, R* out, hipStream_t stream) {
  switch (N) {
    case 2: return launch_run<R, 2, TWO>(y, src, coef, gather, rows, S, NP, PPS, n_out, n_in, out, stream);
    case 4: return launch_run<R, 4, TWO>(y, src, coef, gather, rows, S, NP, PPS, n_out, n_in, out, stream);
    default: return launch_run<R, kPuschRxMaxRun, TWO>(y, src, coef, gather, rows, S, NP, PPS, n_out, n_in, out, stream);
  }
}

template <typename R>
int pusch_ls(const R* y, const int32_t* src, const R* coef, const int32_t* gather, int64_t rows, int S, int NP, int PPS, int N,
             int dmrs_length, int n_out, int64_t n_in, R* out, void* stream) {
  SAMD_REQUIRE(rows >= 0 && S >= 1 && S <= 65535 && NP >= 1 && PPS >= 1 && n_out >= 1 && n_in >= 1, "sizes out of range");
  SAMD_REQUIRE(N == 2 || N == 4 || N == kPuschRxMaxRun, "runs of 2, 4 or 6 pilots (1 to 3 CDM groups without data)");
  SAMD_REQUIRE(dmrs_length == 1 || dmrs_length == 2, "dmrs_length must be 1 or 2");
  SAMD_REQUIRE(NP % PPS == 0 && PPS % N == 0, "num_pilots must be whole DMRS symbols of whole runs");
  SAMD_REQUIRE(dmrs_length == 1 || (NP / PPS) % 2 == 0, "dmrs_length 2 needs pairs of DMRS symbols");
  SAMD_REQUIRE(gather || n_out == NP, "without a gather table there is one output per pilot");
  SAMD_REQUIRE((int64_t)S * NP < (1ll << 31) && (int64_t)S * n_out < (1ll << 31) && n_in < (1ll << 31), "slot too large");
  if (rows == 0) return SAMD_OK;
  SAMD_REQUIRE(y && src && coef && out, "null argument");
  constexpr uintptr_t kAlign = 2 * sizeof(R) - 1;
  SAMD_REQUIRE((reinterpret_cast<uintptr_t>(y) & kAlign) == 0 && (reinterpret_cast<uintptr_t>(coef) & kAlign) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & kAlign) == 0,
               "y, coef and out must be aligned to one complex value");
  hipStream_t st = (hipStream_t)stream;
  if (dmrs_length == 2) return launch_length<R, true>(y, src, coef, gather, rows, S, NP, PPS, N, n_out, n_in, out, st);
  return launch_length<R, false>(y, src, coef, gather, rows, S, NP, PPS, N, n_out, n_in, out, st);
}

}  // namespace
}  // namespace samd

using namespace samd;

extern "C" int samd_pusch_ls_c64(const float* y, const int32_t* src, const float* coef, const int32_t* gather, int64_t rows,
                                 int num_streams, int num_pilots, int pilots_per_symbol, int run, int dmrs_length, int n_out,
                                 int64_t n_in, float* out, void* stream) {
  return pusch_ls<float>(y, src, coef, gather, rows, num_streams, num_pilots, pilots_per_symbol, run, dmrs_length, n_out, n_in,
                         out, stream);
}

extern "C" int samd_pusch_ls_c128(const double* y, const int32_t* src, const double* coef, const int32_t* gather, int64_t rows,
                                  int num_streams, int num_pilots, int pilots_per_symbol, int run, int dmrs_length, int n_out,
                                  int64_t n_in, double* out, void* stream) {
  return pusch_ls<double>(y, src, coef, gather, rows, num_streams, num_pilots, pilots_per_symbol, run, dmrs_length, n_out, n_in,
                          out, stream);
}
