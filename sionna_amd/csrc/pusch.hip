// PUSCH slot grids from the scrambled coded bits in one launch: what PUSCHTransmitter.call does after the transport-block
// encoder (/root/reference/src/sionna/phy/nr/pusch_transmitter.py:217-230) as four passes with three intermediate tensors -
//   Mapper.call               /root/reference/src/sionna/phy/mapping.py:497-519
//   LayerMapper.call          /root/reference/src/sionna/phy/nr/layer_mapping.py:165-189
//   ResourceGridMapper.call   /root/reference/src/sionna/phy/ofdm/resource_grid.py:394-412
//   PUSCHPrecoder.call        /root/reference/src/sionna/phy/nr/pusch_precoder.py:71-95
//
//   grid[b, tx, l, re] = points[label of bits (d * L + l) * m ... + m - 1]   d = data_pos[tx * L + l, re] >= 0
//                      = pilots[tx * L + l, p]                               p = pilot_pos[tx * L + l, re] >= 0
//                      = 0                                                   otherwise
//   out[b, tx, q, re]  = sum_l W[tx, q, l] * grid[b, tx, l, re]              (W = NULL: out = grid)
//
// The layer mapper is the factor L in the bit index.  Memory-bound: 4 m L bytes of bits in, 8 P (16 P) bytes out per
// resource element.  A lane owns one resource element of one transmitter for the whole batch: consecutive lanes are
// consecutive subcarriers, so every store of a wave is one contiguous run per port and the bits a wave reads for its L
// layers are one contiguous run (two bits per load).  The index tables and the pilot values of the lane's element are
// read once and stay in registers across the grid-stride loop over the batch (blockIdx.z); the constellation and the
// transmitter's W sit in LDS.
// Arithmetic (tests/pusch_f32.py, bit-identical): per port re and im start at +0 and add (wr xr - wi xi), (wr xi + wi xr)
// in ascending layer order; the library is built with -ffp-contract=off, so every product and sum is rounded once.
#include "common.h"

namespace samd {
namespace {

constexpr int kPuschThreads = 256;
constexpr int kPuschBatchCap = 1024;                    // blockIdx.z of one launch; a larger batch takes further trips
constexpr int kPuschMaxLayers = 4;                      // 38.211 Sec. 6.3.1.3: a PUSCH has up to four layers and ports
constexpr int kPuschMaxBits = 10;

template <typename R>
struct alignas(2 * sizeof(R)) Cplx {                    // one vector store per complex value
  R re, im;
};

template <typename R, int L>
__global__ __launch_bounds__(kPuschThreads) void pusch_grid_kernel(
    const float* __restrict__ bits, const R* __restrict__ points, const R* __restrict__ pilots,
    const int32_t* __restrict__ data_pos, const int32_t* __restrict__ pilot_pos, const R* __restrict__ w, int64_t B,
    int num_tx, int P, int TF, int ND, int NP, int m, R* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char pusch_lds[];
  R* lut = reinterpret_cast<R*>(pusch_lds);             // [2^m] interleaved re, im
  R* wm = lut + (2 << m);                               // [P, L] interleaved, only with w
  const int tid = threadIdx.x, tx = blockIdx.y;
  for (int i = tid; i < (2 << m); i += kPuschThreads) lut[i] = points[i];
  if (w)
    for (int i = tid; i < 2 * P * L; i += kPuschThreads) wm[i] = w[(int64_t)tx * 2 * P * L + i];
  __syncthreads();
  const int re = blockIdx.x * kPuschThreads + tid;
  if (re >= TF) return;                                 // no barrier follows
  int d[L];
  R fr[L], fi[L];                                       // what the layer carries where it has no data symbol
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int64_t at = (int64_t)(tx * L + l) * TF + re;
    d[l] = data_pos[at];
    fr[l] = fi[l] = (R)0;
    if (d[l] >= ND) d[l] = -1;                          // a table entry the bits do not cover reads nothing
    if (d[l] < 0 && NP > 0) {
      const int p = pilot_pos[at];
      if (p >= 0 && p < NP) {
        fr[l] = pilots[2 * ((int64_t)(tx * L + l) * NP + p)];
        fi[l] = pilots[2 * ((int64_t)(tx * L + l) * NP + p) + 1];
      }
    }
  }
  const int64_t row = (int64_t)ND * L * m;              // bits of one (batch, transmitter)
  for (int64_t b = blockIdx.z; b < B; b += gridDim.z) {
    const float* cw = bits + (b * num_tx + tx) * row;
    R xr[L], xi[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      xr[l] = fr[l];
      xi[l] = fi[l];
      if (d[l] >= 0) {
        const float2* p2 = reinterpret_cast<const float2*>(cw + ((int64_t)d[l] * L + l) * m);   // m even: 8-byte aligned
        int label = 0;
        for (int i = 0; i < m / 2; ++i) {
          const float2 v = p2[i];
          label = (label << 2) | (((int)v.x & 1) << 1) | ((int)v.y & 1);                         // mapping.py:507-511
        }
        xr[l] = lut[2 * label];
        xi[l] = lut[2 * label + 1];
      }
    }
    Cplx<R>* o = reinterpret_cast<Cplx<R>*>(out) + ((b * num_tx + tx) * P) * (int64_t)TF + re;
    if (!w) {
#pragma unroll
      for (int l = 0; l < L; ++l) o[(int64_t)l * TF] = Cplx<R>{xr[l], xi[l]};
    } else {
      for (int q = 0; q < P; ++q) {
        R ar = (R)0, ai = (R)0;
#pragma unroll
        for (int l = 0; l < L; ++l) {
          const R wr = wm[2 * (q * L + l)], wi = wm[2 * (q * L + l) + 1];
          ar += wr * xr[l] - wi * xi[l];
          ai += wr * xi[l] + wi * xr[l];
        }
        o[(int64_t)q * TF] = Cplx<R>{ar, ai};
      }
    }
  }
}

template <typename R, int L>
int launch_layers(const float* bits, const R* points, const R* pilots, const int32_t* data_pos, const int32_t* pilot_pos,
                  const R* w, int64_t B, int num_tx, int P, int TF, int ND, int NP, int m, R* out, hipStream_t stream) {
  const dim3 grid((unsigned)((TF + kPuschThreads - 1) / kPuschThreads), (unsigned)num_tx,
                  (unsigned)(B < kPuschBatchCap ? B : kPuschBatchCap));
  const size_t lds = sizeof(R) * ((size_t)(2 << m) + 2 * (size_t)P * L);
  pusch_grid_kernel<R, L><<<grid, kPuschThreads, lds, stream>>>(bits, points, pilots, data_pos, pilot_pos, w, B, num_tx, P, TF,
                                                               ND, NP, m, out);
  return launch_status();
}

template <typename R>
int pusch_grid(const float* bits, const R* points, const R* pilots, const int32_t* data_pos, const int32_t* pilot_pos,
               const R* w, int64_t B, int num_tx, int L, int P, int TF, int ND, int NP, int m, R* out, void* stream) {
  SAMD_REQUIRE(B >= 0 && num_tx >= 1 && num_tx <= 65535 && TF >= 1 && ND >= 0 && NP >= 0, "sizes out of range");
  SAMD_REQUIRE(L >= 1 && L <= kPuschMaxLayers && P >= 1 && P <= kPuschMaxLayers, "1 to 4 layers and antenna ports");
  SAMD_REQUIRE(m >= 2 && m <= kPuschMaxBits && m % 2 == 0, "num_bits_per_symbol must be even, 2 to 10");
  SAMD_REQUIRE(w || P == L, "without precoding matrices num_ports must equal num_layers");
  SAMD_REQUIRE((int64_t)ND * L * m < (1ll << 31) && (int64_t)num_tx * L * TF < (1ll << 31), "slot too large");
  if (B == 0) return SAMD_OK;
  SAMD_REQUIRE(bits && points && data_pos && pilot_pos && out, "null argument");
  SAMD_REQUIRE(pilots || NP == 0, "null pilots");
  SAMD_REQUIRE((reinterpret_cast<uintptr_t>(bits) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & (2 * sizeof(R) - 1)) == 0,
               "bits must be 8-byte aligned and out aligned to one complex value");
  hipStream_t st = (hipStream_t)stream;
  switch (L) {
    case 1: return launch_layers<R, 1>(bits, points, pilots, data_pos, pilot_pos, w, B, num_tx, P, TF, ND, NP, m, out, st);
    case 2: return launch_layers<R, 2>(bits, points, pilots, data_pos, pilot_pos, w, B, num_tx, P, TF, ND, NP, m, out, st);
    case 3: return launch_layers<R, 3>(bits, points, pilots, data_pos, pilot_pos, w, B, num_tx, P, TF, ND, NP, m, out, st);
    default: return launch_layers<R, 4>(bits, points, pilots, data_pos, pilot_pos, w, B, num_tx, P, TF, ND, NP, m, out, st);
  }
}

}  // namespace
}  // namespace samd

using namespace samd;

extern "C" int samd_pusch_grid_c64(const float* bits, const float* points, const float* pilots, const int32_t* data_pos,
                                   const int32_t* pilot_pos, const float* w, int64_t batch, int num_tx, int num_layers,
                                   int num_ports, int num_re, int num_data, int num_pilots, int num_bits_per_symbol, float* out,
                                   void* stream) {
  return pusch_grid<float>(bits, points, pilots, data_pos, pilot_pos, w, batch, num_tx, num_layers, num_ports, num_re, num_data,
                           num_pilots, num_bits_per_symbol, out, stream);
}

extern "C" int samd_pusch_grid_c128(const float* bits, const double* points, const double* pilots, const int32_t* data_pos,
                                    const int32_t* pilot_pos, const double* w, int64_t batch, int num_tx, int num_layers,
                                    int num_ports, int num_re, int num_data, int num_pilots, int num_bits_per_symbol,
                                    double* out, void* stream) {
  return pusch_grid<double>(bits, points, pilots, data_pos, pilot_pos, w, batch, num_tx, num_layers, num_ports, num_re,
                            num_data, num_pilots, num_bits_per_symbol, out, stream);
}
