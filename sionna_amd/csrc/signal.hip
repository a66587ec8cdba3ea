// Batched FIR filtering: convolve / Filter.call with Upsampling and Downsampling folded into the indexing.
//   convolve            /root/reference/src/sionna/phy/signal/utils.py:13-159 (the four real sums: :122-151)
//   Filter.call         /root/reference/src/sionna/phy/signal/filter.py:268-285
//   Upsampling.call     /root/reference/src/sionna/phy/signal/upsampling.py:57-65
//   Downsampling.call   /root/reference/src/sionna/phy/signal/downsampling.py:59-72
//
//   y[b, m] = sum_{k = 0..K-1} h[k] * xu[b, start + m * down - k],   xu[b, j] = x[b, j / up] if up | j, else 0
//
// With p = start + m * down the taps that meet a sample are k = p % up, p % up + up, ... and the sample of the i-th of them
// is x[b, p / up - i]: the inserted zeros are never formed and a decimated output is never computed.
//
// A workgroup of 256 lanes handles one (row, tile) work item per trip of a grid-stride loop.  The taps (planar, the
// conjugation applied) stay in LDS for the whole launch; per trip the input samples the tile needs, with the halo of
// (K - 1) / up samples to its left, are staged planar in LDS, zeros where the row has no sample: a product with such a zero
// is +-0 and leaves a sum that started at +0 unchanged (finite inputs), so staging zeros equals skipping the tap.
//   up = down = 1 (convolve): tile of 1024 outputs, a lane owns 4 CONSECUTIVE outputs and slides a window of 4 input samples
//     through registers: per tap one broadcast read of the tap and one read of one new sample for 4 multiply-adds.
//   otherwise: tile of 256 * opl outputs (opl = 4, 2 or 1, the largest whose tile fits 64 KB of LDS), a lane owns the
//     outputs tid, tid + 256, ...: consecutive lanes read consecutive LDS words when down = 1.
// Arithmetic (tests/signal_f32.py, bit-identical): every real sum starts at +0 and adds h[k] * x in ascending k with one
// multiplication and one addition (the library is built with -ffp-contract=off); complex output (rr - ii) + j (ri + ir).
#include "common.h"

namespace samd {
namespace {

constexpr int kSigThreads = 256;
constexpr int kSigOpl = 4;                              // outputs per lane of the up = down = 1 path
constexpr int kSigTile = kSigThreads * kSigOpl;         // its tile: 1024 outputs
constexpr int kSigGridCap = 256 * 32;                   // workgroups of one launch; more work items take further trips
constexpr size_t kSigLdsBytes = 64 * 1024;

template <typename R, bool XC, bool HC, bool UNIT>
__global__ __launch_bounds__(kSigThreads) void upfirdn_kernel(const R* __restrict__ x, const R* __restrict__ h_re,
                                                              const R* __restrict__ h_im, int64_t rows, int64_t n, int K,
                                                              int up, int64_t start, int down, int64_t m_out, int conjugate,
                                                              int tile, int span, int64_t tiles, R* __restrict__ out) {
  constexpr bool OC = XC || HC;
  extern __shared__ __align__(16) unsigned char sig_lds[];
  R* hr = reinterpret_cast<R*>(sig_lds);
  R* hi = hr + K;                                       // [K] only if HC
  R* xr = hi + (HC ? K : 0);
  R* xi = xr + span;                                    // [span] only if XC
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += kSigThreads) {
    hr[k] = h_re[k];
    if (HC) hi[k] = conjugate ? -h_im[k] : h_im[k];
  }
  const int halo = (K - 1) / up + 1;
  for (int64_t w = blockIdx.x; w < rows * tiles; w += gridDim.x) {
    const int64_t b = w / tiles, m0 = (w - b * tiles) * tile;
    const int64_t p0 = start + m0 * down;               // >= 0
    const int64_t jlo = p0 / up - halo;                 // input index of LDS slot 0; every slot read lies in [0, span)
    __syncthreads();                                    // the taps are in place / the previous tile has been read
    const R* xrow = x + b * n * (XC ? 2 : 1);
    for (int s = tid; s < span; s += kSigThreads) {
      const int64_t j = jlo + s;
      const bool in = j >= 0 && j < n;
      xr[s] = in ? xrow[XC ? 2 * j : j] : (R)0;
      if (XC) xi[s] = in ? xrow[2 * j + 1] : (R)0;
    }
    __syncthreads();
    R* orow = out + b * m_out * (OC ? 2 : 1);
    if (UNIT) {
      // outputs m0 + 4 tid + j, j = 0..3; win[j] = sample of output j at the current tap
      const int64_t m = m0 + (int64_t)tid * kSigOpl;
      if (m < m_out) {
        int s = tid * kSigOpl + halo;                   // slot of x[p0 + 4 tid]
        R wr[kSigOpl], wi[kSigOpl], rr[kSigOpl], ii[kSigOpl], ri[kSigOpl], ir[kSigOpl];
#pragma unroll
        for (int j = 0; j < kSigOpl; ++j) {
          wr[j] = xr[s + j];
          wi[j] = XC ? xi[s + j] : (R)0;
          rr[j] = ii[j] = ri[j] = ir[j] = (R)0;
        }
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
          const R a = hr[k], c = HC ? hi[k] : (R)0;
#pragma unroll
          for (int j = 0; j < kSigOpl; ++j) {
            rr[j] += a * wr[j];
            if (XC) ir[j] += a * wi[j];
            if (HC) ri[j] += c * wr[j];
            if (XC && HC) ii[j] += c * wi[j];
          }
#pragma unroll
          for (int j = kSigOpl - 1; j > 0; --j) {
            wr[j] = wr[j - 1];
            wi[j] = wi[j - 1];
          }
          --s;                                          // s = 4 tid >= 0 after the last tap: halo = K
          wr[0] = xr[s];
          wi[0] = XC ? xi[s] : (R)0;
        }
#pragma unroll
        for (int j = 0; j < kSigOpl; ++j) {
          if (m + j < m_out) {
            if (OC) {
              orow[2 * (m + j)] = rr[j] - ii[j];
              orow[2 * (m + j) + 1] = ri[j] + ir[j];
            } else {
              orow[m + j] = rr[j];
            }
          }
        }
      }
    } else {
      for (int j = tid; j < tile; j += kSigThreads) {
        const int64_t m = m0 + j;
        if (m >= m_out) break;
        const int64_t p = start + m * down;
        int s = (int)(p / up - jlo);
        R rr = (R)0, ii = (R)0, ri = (R)0, ir = (R)0;
        for (int k = (int)(p % up); k < K; k += up, --s) {
          const R a = hr[k], vr = xr[s];
          rr += a * vr;
          if (XC) ir += a * xi[s];
          if (HC) ri += hi[k] * vr;
          if (XC && HC) ii += hi[k] * xi[s];
        }
        if (OC) {
          orow[2 * m] = rr - ii;
          orow[2 * m + 1] = ri + ir;
        } else {
          orow[m] = rr;
        }
      }
    }
  }
}

template <typename R, bool XC, bool HC, bool UNIT>
int launch_variant(const R* x, const R* h_re, const R* h_im, int64_t B, int64_t N, int K, int up, int64_t start, int down,
                   int64_t M, int conjugate, int tile, int span, size_t lds, R* out, hipStream_t stream) {
  const int64_t tiles = (M + tile - 1) / tile, items = B * tiles;
  const unsigned grid = (unsigned)(items < kSigGridCap ? items : kSigGridCap);
  upfirdn_kernel<R, XC, HC, UNIT><<<grid, kSigThreads, lds, stream>>>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate,
                                                                     tile, span, tiles, out);
  return launch_status();
}

template <typename R, bool XC>
int upfirdn(const R* x, const R* h_re, const R* h_im, int64_t B, int64_t N, int K, int up, int64_t start, int down, int64_t M,
            int conjugate, R* out, void* stream) {
  SAMD_REQUIRE(B >= 0 && N >= 0 && M >= 0, "negative size");
  SAMD_REQUIRE(K >= 1 && K <= SAMD_UPFIRDN_MAX_TAPS, "the kernel takes 1 to SAMD_UPFIRDN_MAX_TAPS (1025) taps");
  SAMD_REQUIRE(up >= 1 && down >= 1 && start >= 0, "up, down >= 1 and start >= 0");
  SAMD_REQUIRE(N * (int64_t)up + K < (1ll << 31) && M < (1ll << 31) && start < (1ll << 31), "row too long");
  SAMD_REQUIRE(up < (1 << 20) && down < (1 << 20), "factor too large");
  if (B == 0 || M == 0) return SAMD_OK;
  SAMD_REQUIRE(x && h_re && out, "null argument");
  SAMD_REQUIRE(B * ((M + kSigThreads - 1) / kSigThreads) < (1ll << 62), "too many work items");
  const bool unit = up == 1 && down == 1, hc = h_im != nullptr;
  int tile = kSigTile, span = 0;
  size_t lds = 0;
  for (;; tile /= 2) {
    // slots of one tile: the samples of its outputs, ((tile - 1) * down) / up + 2 at most, and the halo to their left
    span = (int)(((int64_t)(tile - 1) * down) / up + (K - 1) / up + 3);
    lds = sizeof(R) * ((size_t)(hc ? 2 : 1) * K + (size_t)(XC ? 2 : 1) * span);
    if (lds <= kSigLdsBytes || unit || tile == kSigThreads) break;
  }
  SAMD_REQUIRE(lds <= kSigLdsBytes, "down / up too large: the input samples of 256 outputs exceed 64 KB of LDS");
  hipStream_t st = (hipStream_t)stream;
  if (unit)
    return hc ? launch_variant<R, XC, true, true>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, tile, span, lds, out, st)
              : launch_variant<R, XC, false, true>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, tile, span, lds, out, st);
  return hc ? launch_variant<R, XC, true, false>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, tile, span, lds, out, st)
            : launch_variant<R, XC, false, false>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, tile, span, lds, out, st);
}

}  // namespace
}  // namespace samd

using namespace samd;

extern "C" int samd_upfirdn_f32(const float* x, const float* h_re, const float* h_im, int64_t B, int64_t N, int K, int up,
                                int64_t start, int down, int64_t M, int conjugate, float* out, void* stream) {
  return upfirdn<float, false>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, out, stream);
}

extern "C" int samd_upfirdn_f64(const double* x, const double* h_re, const double* h_im, int64_t B, int64_t N, int K, int up,
                                int64_t start, int down, int64_t M, int conjugate, double* out, void* stream) {
  return upfirdn<double, false>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, out, stream);
}

extern "C" int samd_upfirdn_c64(const float* x, const float* h_re, const float* h_im, int64_t B, int64_t N, int K, int up,
                                int64_t start, int down, int64_t M, int conjugate, float* out, void* stream) {
  return upfirdn<float, true>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, out, stream);
}

extern "C" int samd_upfirdn_c128(const double* x, const double* h_re, const double* h_im, int64_t B, int64_t N, int K, int up,
                                 int64_t start, int down, int64_t M, int conjugate, double* out, void* stream) {
  return upfirdn<double, true>(x, h_re, h_im, B, N, K, up, start, down, M, conjugate, out, stream);
}
