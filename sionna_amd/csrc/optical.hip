// Optical channels: split-step Fourier method (SSFM) fibre and lumped EDFA.
//
// Replaces (reference src/sionna/phy/channel/optical/):
//   SSFM.call                    fiber.py:377-449    fixed step count :425-447, adaptive step width :329-354, :414-422
//   SSFM._apply_linear_operator  fiber.py:257-282    dispersion in fft-shifted order (:271), attenuation, Raman gain
//   SSFM._apply_nonlinear_operator / _apply_noise / _apply_window   fiber.py:284-358
//   EDFA.call                    edfa.py:145-170
//
// The transforms are rocFFT's (rocfft_plan.h, batched over rows, in place); the HIP here is the pointwise work between
// them, fused into one time-domain kernel (window, Kerr rotation, Raman ASE noise, constant factors) and one
// frequency-domain kernel (one complex factor per bin: dispersion, exp(-+alpha dz / 2) and rocFFT's 1/n).  A step is at
// most four launches; without dispersion no transform runs and the constant factor rides in the time kernel.  The noise
// is the element-indexed Philox stream of channel.hip (element i takes half i & 1 of block i / 2) with a fresh call
// counter per step.  Specification: tests/optical_f32.py.
#include "common.h"
#include "rocfft_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace samd {
namespace {

template <typename R> struct Cx;
template <> struct Cx<float> { using type = float2; };
template <> struct Cx<double> { using type = double2; };

__device__ __forceinline__ float2 mk(float a, float b) { return make_float2(a, b); }
__device__ __forceinline__ double2 mk(double a, double b) { return make_double2(a, b); }
__device__ __forceinline__ void sincos_o(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ void sincos_o(double x, double* s, double* c) { sincos(x, s, c); }

__device__ __forceinline__ double u01_d(uint32_t x) {
  return (double)(x >> 8) * 5.9604644775390625e-08 + 2.98023223876953125e-08;      // the float32 stream's uniforms, exact in double
}

// Box-Muller of channel.hip (float) and of f64_ofdm.hip (double, on the same 24-bit uniforms)
__device__ __forceinline__ float2 box_muller_o(uint32_t a, uint32_t b, float) {
  const float r = sqrtf(-2.0f * logf(u01(a)));
  float s, c;
  sincosf(6.283185307179586f * u01(b), &s, &c);
  return make_float2(r * c, r * s);
}
__device__ __forceinline__ double2 box_muller_o(uint32_t a, uint32_t b, double) {
  const double r = sqrt(-2.0 * log(u01_d(a)));
  double s, c;
  sincos(6.283185307179586 * u01_d(b), &s, &c);
  return make_double2(r * c, r * s);
}

// unit normal pair of the flat element index i on the stream (seed, call)
template <typename R>
__device__ __forceinline__ typename Cx<R>::type normal_of(uint64_t seed, uint64_t call, int64_t i) {
  const uint4 r = philox_block(seed, call, (uint64_t)i >> 1);
  return (i & 1) ? box_muller_o(r.z, r.w, R(0)) : box_muller_o(r.x, r.y, R(0));
}

// State of the adaptive step width on the device (fiber.py:329-354), in the block's real type like the reference's loop
// variables; max_bits: the bit pattern of max |q|^2 (non-negative floats order like unsigned integers).
template <typename R>
struct State {
  R remaining, dz, scale;
  unsigned long long max_bits;
};

__device__ __forceinline__ float from_bits(unsigned long long b, float) { return __uint_as_float((unsigned)b); }
__device__ __forceinline__ double from_bits(unsigned long long b, double) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ unsigned long long to_bits(float v) { return (unsigned long long)__float_as_uint(v); }
__device__ __forceinline__ unsigned long long to_bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// Hamming taper in the first and last h samples, 1 elsewhere (fiber.py:391-407); win [2h]
template <typename R>
__device__ __forceinline__ R window_at(const R* __restrict__ win, int h, int n, int t) {
  if (t < h) return win[t];
  if (t >= n - h) return win[t - (n - 2 * h)];
  return R(1);
}

template <typename R>
struct TimeArgs {
  const R* win;              // [2h] or null: no window
  int h;
  R pre, post;               // constant factors before the window and after the noise (1: none)
  R kerr;                    // -gamma dz (8/9 with Manakov); adaptive: per unit length
  R sigma;                   // noise standard deviation per real dimension; adaptive: per sqrt(unit length)
  int nonlin, noise;
  uint64_t seed, call;
  const State<R>* st;        // adaptive: dz (and, with st_scale, the factor `pre`) from the device
  int st_scale;
};

// One lane per sample (both polarisations with P = 2): q = post * (noise + exp(j kerr sum_p |q_p|^2) * w[t] * pre * q)
template <typename R, int P>
__global__ __launch_bounds__(256) void time_kernel(const typename Cx<R>::type* in, int64_t samples, int n, TimeArgs<R> a,
                                                   typename Cx<R>::type* out) {                 // out may be in
  using R2 = typename Cx<R>::type;
  R pre = a.pre, kerr = a.kerr, sigma = a.sigma;
  if (a.st) {
    const R dz = a.st->dz;
    kerr = a.kerr * dz;
    sigma = a.sigma * (R)sqrt(dz);
    if (a.st_scale) pre = a.st->scale;
  }
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < samples; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = s / n;
    const int t = (int)(s - row * n);
    const int64_t i0 = row * P * n + t;
    R f = pre;
    if (a.win) f = f * window_at(a.win, a.h, n, t);
    R2 q[P];
    R power = R(0);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const R2 v = in[i0 + (int64_t)p * n];
      q[p] = mk(v.x * f, v.y * f);
      power += q[p].x * q[p].x + q[p].y * q[p].y;
    }
    R sn = R(0), cs = R(1);
    if (a.nonlin) sincos_o(power * kerr, &sn, &cs);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      R2 v = q[p];
      if (a.nonlin) v = mk(v.x * cs - v.y * sn, v.x * sn + v.y * cs);
      if (a.noise) {
        const R2 w = normal_of<R>(a.seed, a.call, i0 + (int64_t)p * n);
        v = mk(v.x + w.x * sigma, v.y + w.y * sigma);
      }
      out[i0 + (int64_t)p * n] = mk(v.x * a.post, v.y * a.post);
    }
  }
}

// bin of the flat element index: a 32-bit remainder wherever the tensor allows it
__device__ __forceinline__ int bin_of(int64_t i, int n, bool small) {
  return small ? (int)((uint32_t)i % (uint32_t)n) : (int)(i % n);
}

// q[r, k] *= tf[k]: the step's whole linear operator in the frequency domain.  Fixed scheme: tf is the host table and
// carries every factor (st null).  Adaptive scheme: tf is the step's (cos, sin) of adaptive_factor_kernel, and the
// product is scaled by the step's exp(-+alpha dz / 2) / n from the device state.
template <typename R>
__global__ __launch_bounds__(256) void freq_kernel(typename Cx<R>::type* __restrict__ q, int64_t total, int n,
                                                   const typename Cx<R>::type* __restrict__ tf,
                                                   const State<R>* __restrict__ st, R inv_n) {
  const bool small = total <= 0x7fffffffll;
  const R scale = st ? st->scale * inv_n : R(1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto v = q[i];
    const auto h = tf[bin_of(i, n, small)];
    auto o = mk(v.x * h.x - v.y * h.y, v.x * h.y + v.y * h.x);
    if (st) o = mk(o.x * scale, o.y * scale);
    q[i] = o;
  }
}

// Adaptive step: the n factors exp(j c2[k] dz) of the step, once per bin.  The phase (it can be thousands of radians),
// its sine and its cosine are formed in double and rounded once to the block's type, like the entries of the fixed
// scheme's host tables: the adaptive scheme answers errors of the step's operator through max |q|^2 and the next step
// width, so the factor is held to the table's accuracy.
template <typename R>
__global__ __launch_bounds__(256) void adaptive_factor_kernel(const double* __restrict__ c2, const State<R>* __restrict__ st, int n,
                                                              typename Cx<R>::type* __restrict__ tf) {
  const double dz = (double)st->dz;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    double sn, cs;
    sincos(c2[k] * dz, &sn, &cs);
    tf[k] = mk((R)cs, (R)sn);
  }
}

// max |q|^2 over the whole tensor into st->max_bits (fiber.py:330), and the step's window on the way through
template <typename R>
__global__ __launch_bounds__(256) void max_window_kernel(const typename Cx<R>::type* in, int64_t total, int n,
                                                         const R* __restrict__ win, int h, State<R>* __restrict__ st,
                                                         typename Cx<R>::type* out) {           // out may be in
  __shared__ R red[256];
  R m = R(0);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto v = in[i];
    const R p = v.x * v.x + v.y * v.y;
    m = p > m ? p : m;
    if (win) {
      const R w = window_at(win, h, n, bin_of(i, n, total <= 0x7fffffffll));
      out[i] = mk(v.x * w, v.y * w);
    } else if (out != in) {
      out[i] = v;
    }
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(&st->max_bits, to_bits(red[0]));
}

template <typename R>
__global__ void state_init_kernel(State<R>* st, R length) {
  st->remaining = length;
  st->dz = R(0);
  st->scale = R(1);
  st->max_bits = 0ull;
}

// dz = min(phase_inc / gamma / max |q|^2, remaining) (fiber.py:332; an all-zero signal or gamma = 0 divides to +inf and
// takes the remaining length), remaining -= dz (:346), the step's constant factor, and the maximum cleared for the next step
template <typename R>
__global__ void step_width_kernel(State<R>* st, R phase_inc, R gamma, double half_alpha) {
  const R maxp = from_bits(st->max_bits, R(0));
  const R want = phase_inc / gamma / maxp;
  const R rem = st->remaining;
  const R dz = want < rem ? want : rem;        // a NaN (0 / 0) takes the remaining length
  st->dz = dz;
  st->remaining = rem - dz;
  st->scale = (R)exp(half_alpha * (double)dz);
  st->max_bits = 0ull;
}

// y = sqrt(g) x + n (edfa.py:149-168)
template <typename R>
__global__ __launch_bounds__(256) void edfa_kernel(const typename Cx<R>::type* __restrict__ x, int64_t total, R sqrt_g, R sigma,
                                                   uint64_t seed, uint64_t call, typename Cx<R>::type* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto v = x[i];
    auto o = mk(v.x * sqrt_g, v.y * sqrt_g);
    if (sigma != R(0)) {
      const auto w = normal_of<R>(seed, call, i);
      o = mk(o.x + w.x * sigma, o.y + w.y * sigma);
    }
    y[i] = o;
  }
}

inline int grid_for(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), 256 * 32);
}

// workspace: [3n complex: the transfer vectors over dz, dz / 2 and 3 dz / 2 - the adaptive scheme keeps its n doubles of
// phase per unit length in the first vector's place and the step's n factors in the third's][n real: window][state]
template <typename R>
struct Layout {
  size_t tf_off, win_off, st_off, bytes;
  explicit Layout(int n) {
    tf_off = 0;
    win_off = align_up((size_t)3 * n * 2 * sizeof(R), 16);
    st_off = align_up(win_off + (size_t)n * sizeof(R), 16);
    bytes = st_off + align_up(sizeof(State<R>), 16);
  }
};

struct SsfmConfig {
  int64_t rows;
  int n, manakov;
  double alpha, beta_2, gamma, length, sample_duration;
  int n_ssfm;
  double phase_inc;
  int h;
  double p_n_ase;
  int amp, att, disp, nonlin;
  uint64_t seed, call;
};

// The reference's frequency of bin k in fft-shifted order (utils.py:104-118, fiber.py:271): np.fft.fftshift moves entry
// (k - n // 2) mod n of the ascending vector f = (-(n // 2) + j) df to bin k - for odd n that is one bin off the
// transform's own order, and it is what the reference computes.
inline double bin_frequency(int k, int n, double sample_duration) {
  const int j = ((k - n / 2) % n + n) % n;
  return (double)(j - n / 2) * (1.0 / sample_duration / (double)n);
}

template <typename R>
int launch_time(const typename Cx<R>::type* in, typename Cx<R>::type* out, const SsfmConfig& c, const TimeArgs<R>& a, hipStream_t st) {
  const int64_t samples = c.rows * c.n;
  if (c.manakov)
    time_kernel<R, 2><<<grid_for(samples), 256, 0, st>>>(in, samples, c.n, a, out);
  else
    time_kernel<R, 1><<<grid_for(samples), 256, 0, st>>>(in, samples, c.n, a, out);
  return launch_status();
}

// host table -> workspace: the copy, then the wait that lets the pageable source leave scope
inline int upload(void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return SAMD_OK;
  SAMD_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
  SAMD_HIP_CHECK(hipStreamSynchronize(st));
  return SAMD_OK;
}

template <typename R>
int ssfm(const R* x_, R* y_, const SsfmConfig& c, int64_t* steps_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  using R2 = typename Cx<R>::type;
  constexpr bool dbl = sizeof(R) == 8;
  const R2* x = (const R2*)x_;
  R2* y = (R2*)y_;
  const int P = c.manakov ? 2 : 1;
  const int n = c.n;
  const int64_t total = c.rows * P * n;
  const int batch = (int)(c.rows * P);
  const Layout<R> lay(n);
  char* ws = (char*)workspace;
  R2* tf_full = (R2*)(ws + lay.tf_off);
  R2* tf_half = tf_full + n;
  R2* tf_join = tf_half + n;
  double* c2_dev = (double*)(ws + lay.tf_off);
  R* win = c.h > 0 ? (R*)(ws + lay.win_off) : nullptr;
  State<R>* state = (State<R>*)(ws + lay.st_off);

  const bool adaptive = c.n_ssfm < 0;
  const bool noise = c.amp && c.p_n_ase > 0.0;
  // exp(-alpha dz / 2) of the attenuation and exp(+alpha dz / 2) of the Raman gain as one factor (fiber.py:274-280)
  const double half_alpha = ((c.amp ? 1.0 : 0.0) - (c.att ? 1.0 : 0.0)) * c.alpha / 2.0;
  const double kerr_unit = -c.gamma * (c.manakov ? 8.0 / 9.0 : 1.0);
  const double sigma_unit = noise ? std::sqrt(c.p_n_ase / c.length / 2.0) : 0.0;      // per sqrt(dz)

  // host tables, float64, rounded once: phase per unit length c2[k] = -beta_2 / 2 (2 pi f_k)^2, the window
  std::vector<double> c2(c.disp ? n : 0);
  for (int k = 0; k < (int)c2.size(); ++k) {
    const double w = 2.0 * M_PI * bin_frequency(k, n, c.sample_duration);
    c2[k] = -c.beta_2 / 2.0 * w * w;
  }
  auto transfer = [&](double dz, R2* dst) {        // dispersion, constant factor and rocFFT's 1 / n over dz
    const double sc = std::exp(half_alpha * dz) / (double)n;
    for (int k = 0; k < n; ++k) dst[k] = R2{(R)(std::cos(c2[k] * dz) * sc), (R)(std::sin(c2[k] * dz) * sc)};
  };
  std::vector<R> win_host(2 * (size_t)c.h);
  for (int k = 0; k < 2 * c.h; ++k) win_host[k] = (R)(0.54 - 0.46 * std::cos(2.0 * M_PI * (double)k / (double)(2 * c.h)));
  if (int rc = upload(win, win_host.data(), win_host.size() * sizeof(R), st)) return rc;

  TimeArgs<R> ta;
  std::memset(&ta, 0, sizeof(ta));
  ta.pre = ta.post = R(1);
  ta.h = c.h;
  ta.nonlin = c.nonlin;
  ta.noise = noise;
  ta.seed = c.seed;

  if (!adaptive) {
    const double dz = c.length / (double)c.n_ssfm;
    // Where linear operators meet with no work between them they are applied in one pass: without nonlinearity and
    // noise the last step's N is empty, so the last full step and the closing half step join (3 dz / 2); the window is
    // never applied in the last step, so with one step, or no window, the whole fibre is one operator over its length.
    const bool last_empty = !c.nonlin && !noise;
    const bool identity_time = last_empty && (c.h == 0 || c.n_ssfm == 1);
    ta.kerr = (R)(kerr_unit * dz);
    ta.sigma = (R)(sigma_unit * std::sqrt(dz));
    *steps_out = c.n_ssfm;
    const int windowed = c.n_ssfm - 1;                                 // steps of window, N, noise, D (fiber.py:435-441)
    if (c.disp) {
      std::vector<R2> tfs(3 * (size_t)n);
      transfer(identity_time ? c.length : dz, tfs.data());
      transfer(dz / 2.0, tfs.data() + n);
      transfer(1.5 * dz, tfs.data() + 2 * (size_t)n);
      if (int rc = upload(tf_full, tfs.data(), tfs.size() * sizeof(R2), st)) return rc;
      if (y != x) SAMD_HIP_CHECK(hipMemcpyAsync(y, x, (size_t)total * sizeof(R2), hipMemcpyDeviceToDevice, st));
      auto linear = [&](const R2* tf) -> int {
        if (int rc = fft_inplace(y, n, batch, false, st, dbl)) return rc;
        freq_kernel<R><<<grid_for(total), 256, 0, st>>>(y, total, n, tf, nullptr, R(1));
        if (int rc = launch_status()) return rc;
        return fft_inplace(y, n, batch, true, st, dbl);
      };
      if (identity_time) return linear(tf_full);
      if (int rc = linear(tf_half)) return rc;                         // fiber.py:433
      for (int s = 0; s < windowed; ++s) {
        ta.win = win;
        ta.call = c.call + (uint64_t)s;
        if (ta.win || ta.nonlin || ta.noise)
          if (int rc = launch_time<R>(y, y, c, ta, st)) return rc;
        if (int rc = linear(last_empty && s == windowed - 1 ? tf_join : tf_full)) return rc;
      }
      if (last_empty) return SAMD_OK;
      ta.win = nullptr;                                                // :443-447: N, noise, half D
      ta.call = c.call + (uint64_t)windowed;
      if (int rc = launch_time<R>(y, y, c, ta, st)) return rc;
      return linear(tf_half);
    }
    // no dispersion: no transform at all, the constant factors ride in the time kernel
    if (identity_time) {
      ta.pre = (R)std::exp(half_alpha * c.length);
      return launch_time<R>(x, y, c, ta, st);
    }
    const R a_half = (R)std::exp(half_alpha * dz / 2.0), a_full = (R)std::exp(half_alpha * dz);
    const R a_join = (R)std::exp(half_alpha * 1.5 * dz);
    const R2* src = x;
    for (int s = 0; s < c.n_ssfm; ++s) {
      const bool last = s == windowed;
      if (last && last_empty) break;                                   // joined into the step before
      ta.win = last ? nullptr : win;
      ta.call = c.call + (uint64_t)s;
      ta.pre = s == 0 ? a_half : R(1);
      ta.post = last ? a_half : (last_empty && s == windowed - 1) ? a_join : a_full;
      if (int rc = launch_time<R>(src, y, c, ta, st)) return rc;
      src = y;
    }
    return SAMD_OK;
  }

  // adaptive step width (fiber.py:335-354, 414-422): window, D, N, noise
  if (int rc = upload(c2_dev, c2.data(), c2.size() * sizeof(double), st)) return rc;
  state_init_kernel<R><<<1, 1, 0, st>>>(state, (R)c.length);
  if (int rc = launch_status()) return rc;
  ta.kerr = (R)kerr_unit;
  ta.sigma = (R)sigma_unit;
  ta.st = state;
  ta.st_scale = c.disp ? 0 : 1;
  R remaining = (R)c.length;
  int64_t steps = 0;
  const R2* src = x;
  while (remaining >= (R)1e-3) {                                       // :352-354
    max_window_kernel<R><<<grid_for(total), 256, 0, st>>>(src, total, n, (const R*)win, c.h, state, y);
    if (int rc = launch_status()) return rc;
    src = y;
    step_width_kernel<R><<<1, 1, 0, st>>>(state, (R)c.phase_inc, (R)c.gamma, half_alpha);
    if (int rc = launch_status()) return rc;
    if (c.disp) {
      if (int rc = fft_inplace(y, n, batch, false, st, dbl)) return rc;
      adaptive_factor_kernel<R><<<grid_for(n), 256, 0, st>>>(c2_dev, state, n, tf_join);
      if (int rc = launch_status()) return rc;
      freq_kernel<R><<<grid_for(total), 256, 0, st>>>(y, total, n, tf_join, state, (R)(1.0 / (double)n));
      if (int rc = launch_status()) return rc;
      if (int rc = fft_inplace(y, n, batch, true, st, dbl)) return rc;
    }
    ta.call = c.call + (uint64_t)steps;
    if (ta.nonlin || ta.noise || ta.st_scale)
      if (int rc = launch_time<R>(y, y, c, ta, st)) return rc;
    ++steps;
    R next = R(0);
    SAMD_HIP_CHECK(hipMemcpyAsync(&next, &state->remaining, sizeof(R), hipMemcpyDeviceToHost, st));
    SAMD_HIP_CHECK(hipStreamSynchronize(st));
    if (!(next < remaining)) {
      set_error("SSFM: the adaptive step width does not advance (phase_inc / gamma / max|q|^2 is zero or not a number)");
      return SAMD_ERR_INVALID;
    }
    remaining = next;
  }
  if (steps == 0 && y != x) SAMD_HIP_CHECK(hipMemcpyAsync(y, x, (size_t)total * sizeof(R2), hipMemcpyDeviceToDevice, st));
  *steps_out = steps;
  return SAMD_OK;
}

int check_ssfm(const void* x, const void* y, const SsfmConfig& c, const int64_t* steps, const void* workspace, size_t workspace_bytes,
               size_t need) {
  SAMD_REQUIRE(x && y && steps, "null argument");
  SAMD_REQUIRE(c.rows >= 0 && c.n > 0, "bad shape");
  SAMD_REQUIRE(c.rows * (c.manakov ? 2 : 1) < (1ll << 31), "too many rows for one batched transform");
  SAMD_REQUIRE(c.n_ssfm > 0 || c.n_ssfm == -1, "n_ssfm must be positive, or -1 for the adaptive step width");
  SAMD_REQUIRE(c.h >= 0 && 2 * (int64_t)c.h <= c.n, "half_window_length must lie in [0, n / 2]");
  SAMD_REQUIRE(c.length >= 0.0 && c.sample_duration > 0.0 && c.p_n_ase >= 0.0, "bad parameter");
  if (c.rows > 0) {
    SAMD_REQUIRE(workspace, "null workspace");
    if (workspace_bytes < need) {
      set_error("SSFM: workspace too small (samd_ssfm_workspace_bytes)");
      return SAMD_ERR_WORKSPACE;
    }
  }
  return SAMD_OK;
}

}  // namespace
}  // namespace samd

using namespace samd;

extern "C" size_t samd_ssfm_workspace_bytes(int n, int double_precision) {
  if (n <= 0) return 0;
  return double_precision ? Layout<double>(n).bytes : Layout<float>(n).bytes;
}

#define SAMD_SSFM_CONFIG                                                                                                  \
  SsfmConfig c{rows, n, with_manakov, alpha, beta_2, gamma, length, sample_duration, n_ssfm, phase_inc, half_window_length, \
               p_n_ase, with_amplification, with_attenuation, with_dispersion, with_nonlinearity, seed, call}

extern "C" int samd_ssfm_c64(const float* x, int64_t rows, int n, int with_manakov, double alpha, double beta_2, double gamma,
                             double length, double sample_duration, int n_ssfm, double phase_inc, int half_window_length,
                             double p_n_ase, int with_amplification, int with_attenuation, int with_dispersion,
                             int with_nonlinearity, uint64_t seed, uint64_t call, int64_t* steps, void* workspace,
                             size_t workspace_bytes, float* y, void* stream) {
  SAMD_SSFM_CONFIG;
  if (int rc = check_ssfm(x, y, c, steps, workspace, workspace_bytes, samd_ssfm_workspace_bytes(n, 0))) return rc;
  *steps = 0;
  if (rows == 0) return SAMD_OK;
  return ssfm<float>(x, y, c, steps, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int samd_ssfm_c128(const double* x, int64_t rows, int n, int with_manakov, double alpha, double beta_2, double gamma,
                              double length, double sample_duration, int n_ssfm, double phase_inc, int half_window_length,
                              double p_n_ase, int with_amplification, int with_attenuation, int with_dispersion,
                              int with_nonlinearity, uint64_t seed, uint64_t call, int64_t* steps, void* workspace,
                              size_t workspace_bytes, double* y, void* stream) {
  SAMD_SSFM_CONFIG;
  if (int rc = check_ssfm(x, y, c, steps, workspace, workspace_bytes, samd_ssfm_workspace_bytes(n, 1))) return rc;
  *steps = 0;
  if (rows == 0) return SAMD_OK;
  return ssfm<double>(x, y, c, steps, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int samd_edfa_c64(const float* x, int64_t n, double sqrt_g, double sigma, uint64_t seed, uint64_t call, float* y,
                             void* stream) {
  SAMD_REQUIRE(x && y && n >= 0 && sigma >= 0.0, "bad argument");
  if (n == 0) return SAMD_OK;
  edfa_kernel<float><<<grid_for(n), 256, 0, (hipStream_t)stream>>>((const float2*)x, n, (float)sqrt_g, (float)sigma, seed, call, (float2*)y);
  return launch_status();
}

extern "C" int samd_edfa_c128(const double* x, int64_t n, double sqrt_g, double sigma, uint64_t seed, uint64_t call, double* y,
                              void* stream) {
  SAMD_REQUIRE(x && y && n >= 0 && sigma >= 0.0, "bad argument");
  if (n == 0) return SAMD_OK;
  edfa_kernel<double><<<grid_for(n), 256, 0, (hipStream_t)stream>>>((const double2*)x, n, sqrt_g, sigma, seed, call, (double2*)y);
  return launch_status();
}
