// Discrete channels (binary memoryless / symmetric / Z / erasure) on the counter-based Philox4x32-10 stream.
//
// Replaces (reference src/sionna/phy/channel/discrete_channel.py):
//   BinaryMemorylessChannel.call   :238-296   (BinarySymmetricChannel :376-385 and BinaryZChannel :470-478 call it)
//   BinaryErasureChannel.call      :564-596
//   _sample_errors                 :191-222   Gumbel-softmax + straight-through binariser -> ONE threshold comparison
//   _custom_xor                    :168-179
//
// The reference's sampler exists to keep pb trainable; without an autograd path the law is drawn directly (DESIGN.md,
// "Discrete channels"): element i of the flattened input uses word i % 4 of philox_block(seed, call, i / 4) - the layout
// of binary_source_kernel (channel.hip) - and the error event is  (uint64)word < (uint64)ceil(p * 2^32)  with
// p = pb > 0 ? (pb < 1 ? pb : 1) : 0  (NaN -> 0).  p * 2^32 is exact in float32 and float64, so P(e) = ceil(p 2^32) / 2^32
// lies in [p, p + 2^-32); p = 0 never fires, p = 1 always does.  One word per element: the memoryless channel compares
// against pb0 where x is the neutral element (0, or -1 for bipolar input) and against pb1 elsewhere.
// Specification: tests/discrete_f32.py (bit for bit; float64 LLRs within two ulp of each device log).
#include "common.h"
#include "accurate_math.h"

namespace samd {

// four consecutive elements, moved with one instruction up to 16 bytes (two for the 8-byte types)
template <typename T>
struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) Quad {
  T v[4];
};

template <typename P>
__device__ __forceinline__ P unit_clip(P pb) {                 // tf.clip_by_value(pb, 0, 1) of :255-256, NaN -> 0
  return pb > (P)0 ? (pb < (P)1 ? pb : (P)1) : (P)0;
}

template <typename P>
__device__ __forceinline__ uint64_t threshold(P p) {            // ceil(p 2^32): exact product, 0 .. 2^32
  return (uint64_t)ceil(p * (P)4294967296.0);
}

__device__ __forceinline__ float log_def(float a) {             // the defined float32 log; a <= 0 only as 1 - 1 - eps < 0
  return a > 0.0f ? log_rn_f32(a) : __builtin_nanf("");
}
__device__ __forceinline__ double log_def(double a) { return log(a); }

template <typename P>
__device__ __forceinline__ P sym_clip(P v, P m) {               // tf.clip_by_value(v, -m, m) of :293-294; NaN stays NaN
  return v < -m ? -m : (v > m ? m : v);
}

template <typename T>
struct is_float_t { static constexpr bool value = false; };
template <>
struct is_float_t<float> { static constexpr bool value = true; };
template <>
struct is_float_t<double> { static constexpr bool value = true; };

// One element.  KIND 0: memoryless family, 1: erasure.  LLR only for the float types (T == P).
template <typename T, typename P, int KIND, bool LLR>
__device__ __forceinline__ T channel_element(T x, uint32_t word, P pb0, P pb1, bool bipolar, P llr_max) {
  if constexpr (KIND == 1) {
    const bool e = (uint64_t)word < threshold<float>(unit_clip<float>((float)pb1));      // :570: pb as float32
    if constexpr (LLR) {
      const T xb = bipolar ? x : (T)((T)2 * x - (T)1);                                     // :582-584
      return e ? (T)0 : (T)(xb * (T)llr_max);
    } else {
      return e ? (bipolar ? (T)0 : (T)-1) : x;                                             // :589-595
    }
  } else {
    const P p0 = unit_clip<P>(pb0), p1 = unit_clip<P>(pb1);
    const bool one = x != (bipolar ? (T)-1 : (T)0);                                        // :264-270
    const bool e = (uint64_t)word < threshold<P>(one ? p1 : p0);
    T y;
    if (bipolar) {
      y = (T)(x * (T)(1 - 2 * (int)e));                                                    // :275
    } else if constexpr (is_float_t<T>::value) {
      y = x - (T)e;                                                                        // :177 |x - e|
      y = y < (T)0 ? -y : y;
    } else {
      y = (T)((x + (T)e) & (T)1);                                                          // :175 (a + b) mod 2, sum in {0,1,2}
    }
    if constexpr (LLR) {
      const P eps = (P)1e-9;
      const bool r1 = bipolar ? (y == (T)1) : ((T)2 * y - (T)1 == (T)1);                   // :282-283, 291
      P v;
      if (r1) {
        v = log_def(((P)1 - p1) - eps) - log_def(p0 + eps);                                // :288-289
      } else {
        v = log_def(p1 + eps) - log_def(((P)1 - p0) - eps);                                // :286-287 times y = -1
      }
      return (T)sym_clip<P>(v, llr_max);
    } else {
      return y;
    }
  }
}

template <typename T, typename P, int KIND, bool LLR>
__global__ __launch_bounds__(256) void discrete_channel_kernel(const T* x, const P* __restrict__ pb0,
                                                               const P* __restrict__ pb1, int64_t pb_stride,
                                                               int64_t pb_len, int bipolar, P llr_max, uint64_t seed,
                                                               uint64_t call, int64_t n, T* y) {
  const int64_t nblk = (n + 3) / 4;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= nblk) return;
  // position of element blk * 4 in the period of pb: one division per lane, then additions modulo pb_len
  const uint64_t len = (uint64_t)pb_len;
  uint64_t r = len == 1 ? 0 : ((uint64_t)blk * 4) % len;
  const uint64_t dr = len == 1 ? 0 : ((uint64_t)step * 4) % len;
  const bool vec = ((((uintptr_t)x) | ((uintptr_t)y)) & (alignof(Quad<T>) - 1)) == 0;
  for (; blk < nblk; blk += step) {
    const uint4 w4 = philox_block(seed, call, (uint64_t)blk);
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    const int64_t i = blk * 4;
    const int cnt = n - i >= 4 ? 4 : (int)(n - i);
    Quad<T> q;
    if (cnt == 4 && vec) {
      q = *reinterpret_cast<const Quad<T>*>(x + i);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) q.v[j] = j < cnt ? x[i + j] : (T)0;
    }
    uint64_t rj = r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // (a lane of the tail block still reads pb at a valid index: rj < pb_len always)
      const P b1 = pb1[rj * (uint64_t)pb_stride];
      const P b0 = pb0 ? pb0[rj * (uint64_t)pb_stride] : (P)0;
      q.v[j] = channel_element<T, P, KIND, LLR>(q.v[j], w[j], b0, b1, bipolar != 0, llr_max);
      if (++rj == len) rj = 0;
    }
    if (cnt == 4 && vec) {
      *reinterpret_cast<Quad<T>*>(y + i) = q;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) y[i + j] = q.v[j];
    }
    r += dr;
    if (r >= len) r -= len;
  }
}

}  // namespace samd

using namespace samd;

// grid-stride over a capped grid, the cap of channel.hip: 8192 blocks of 256 lanes, 4 elements each = 2^23 elements a trip
static constexpr int kMaxGrid = 256 * 32;

template <typename T, typename P, bool FLOAT>
static int discrete_channel(const T* x, const P* pb0, const P* pb1, int64_t pb_stride, int64_t pb_len, int kind, int bipolar,
                            int return_llrs, double llr_max, uint64_t seed, uint64_t call, int64_t n, T* y, void* stream) {
  SAMD_REQUIRE(x && y && pb1 && n >= 0, "bad argument");
  SAMD_REQUIRE(pb_len >= 1 && pb_stride >= 1, "pb needs a period and an element stride of at least 1");
  SAMD_REQUIRE(kind == 0 || kind == 1, "kind: 0 memoryless family, 1 erasure");
  SAMD_REQUIRE(llr_max >= 0.0, "llr_max must not be negative");
  SAMD_REQUIRE(FLOAT || !return_llrs, "LLR outputs require a float entry");
  SAMD_REQUIRE((T)-1 < (T)0 || (!bipolar && kind == 0), "bipolar input and the erasure channel need a signed type");
  if (n == 0) return SAMD_OK;
  const int64_t nblk = (n + 3) / 4;
  const dim3 grid((unsigned)std::min<int64_t>((nblk + 255) / 256, kMaxGrid)), block(256);
  hipStream_t s = (hipStream_t)stream;
  const P lm = (P)llr_max;
#define SAMD_DISCRETE_LAUNCH(KIND, LLR)                                                                          \
  hipLaunchKernelGGL((discrete_channel_kernel<T, P, KIND, LLR>), grid, block, 0, s, x, pb0, pb1, pb_stride, pb_len, \
                     bipolar, lm, seed, call, n, y)
  if (FLOAT && return_llrs) {
    if (kind == 0) SAMD_DISCRETE_LAUNCH(0, FLOAT); else SAMD_DISCRETE_LAUNCH(1, FLOAT);
  } else {
    if (kind == 0) SAMD_DISCRETE_LAUNCH(0, false); else SAMD_DISCRETE_LAUNCH(1, false);
  }
#undef SAMD_DISCRETE_LAUNCH
  return launch_status();
}

#define SAMD_DISCRETE_ENTRY(SUFFIX, T, P, FLOAT)                                                                       \
  extern "C" int samd_discrete_channel_##SUFFIX(const T* x, const P* pb0, const P* pb1, int64_t pb_stride,             \
                                                int64_t pb_len, int kind, int bipolar, int return_llrs, double llr_max, \
                                                uint64_t seed, uint64_t call, int64_t n, T* y, void* stream) {         \
    return discrete_channel<T, P, FLOAT>(x, pb0, pb1, pb_stride, pb_len, kind, bipolar, return_llrs, llr_max, seed,    \
                                         call, n, y, stream);                                                          \
  }
SAMD_DISCRETE_ENTRY(f32, float, float, true)
SAMD_DISCRETE_ENTRY(f64, double, double, true)
SAMD_DISCRETE_ENTRY(i8, int8_t, float, false)
SAMD_DISCRETE_ENTRY(u8, uint8_t, float, false)
SAMD_DISCRETE_ENTRY(i16, int16_t, float, false)
SAMD_DISCRETE_ENTRY(i32, int32_t, float, false)
SAMD_DISCRETE_ENTRY(i64, int64_t, float, false)
