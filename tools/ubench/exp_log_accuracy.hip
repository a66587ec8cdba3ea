// Accuracy of the device functions the LLR demapper kernels are built on, against float64, over the argument ranges the kernels
// use - the constants c_exp, c_log (and those of the prior path) of tests/demap_f32.py are twice what this prints (DESIGN.md
// "Demapper bound").  EVERY float of each range is evaluated.  Errors in units of u = 2^-24.
//   exp2  __builtin_amdgcn_exp2f(t),  t in [-126, 0]:        |f - 2^t| / 2^t
//   log2  __builtin_amdgcn_logf(x),   x in [2^-116, 2^10]:   |f - log2 x| / max(|log2 x|, 1)
//   expf  (device libm),              x in [-87, 0]:         |f - e^x| / e^x         (log_sigmoid of the prior path)
//   log1pf (device libm),             x in [2^-126, 1]:      |f - log1p x| / log1p x
//   logf  (device libm),              x in [1, 2^10]:        |f - ln x| / ln x       (the sum of SymbolDemapper's log-softmax,
//                                                                                     tests/symbol_f32.py; ln 1 = 0 must be exact)
//   demap_exp / exp_core_f32,         x in [-87, 0]:         |f - e^x| / e^x         (cross-checks of the derivation, not inputs)
//   log_core_f32,                     x in [2^-116, 2^10]:   |f - ln x| / max(|ln x|, 1)
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off exp_log_accuracy.hip -o exp_log_accuracy
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "../../sionna_amd/csrc/bp_math.h"
#include "../../sionna_amd/csrc/demap_core.h"
using namespace samd;

enum { F_EXP2, F_LOG2, F_EXPF, F_LOG1PF, F_LOGF, F_DEMAP_EXP, F_EXP_CORE, F_LOG_CORE, F_COUNT };

template <int F>
__global__ void sweep(unsigned lo, unsigned hi, unsigned sign, unsigned long long* worst, unsigned* where) {
  double w = 0.;
  unsigned at = 0;
  for (unsigned long long b = lo + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b <= hi;
       b += (unsigned long long)gridDim.x * blockDim.x) {
    const float x = __uint_as_float((unsigned)b | sign);
    const double xd = (double)x;
    double f, r, s;
    if constexpr (F == F_EXP2) { f = __builtin_amdgcn_exp2f(x); r = exp2(xd); s = r; }
    if constexpr (F == F_LOG2) { f = __builtin_amdgcn_logf(x); r = log2(xd); s = fmax(fabs(r), 1.); }
    if constexpr (F == F_EXPF) { f = expf(x); r = exp(xd); s = r; }
    if constexpr (F == F_LOG1PF) { f = log1pf(x); r = log1p(xd); s = r; }
    if constexpr (F == F_LOGF) { f = logf(x); r = log(xd); s = r > 0. ? r : (f == 0. ? 1. : 0.); }
    if constexpr (F == F_DEMAP_EXP) { f = demap_exp(x); r = exp(xd); s = r; }
    if constexpr (F == F_EXP_CORE) { f = exp_core_f32(x); r = exp(xd); s = r; }
    if constexpr (F == F_LOG_CORE) { f = log_core_f32(x); r = log(xd); s = fmax(fabs(r), 1.); }
    const double err = fabs(f - r) / s * 16777216.;
    if (err > w) { w = err; at = (unsigned)b | sign; }
  }
  // one winner per thread: positive doubles order like their bit patterns
  const unsigned long long bits = (unsigned long long)__double_as_longlong(w);
  if (atomicMax(worst, bits) < bits) *where = at;     // the argument is a hint only (not atomic with the maximum)
}

static unsigned bits_of(float x) { unsigned b; memcpy(&b, &x, 4); return b; }

template <int F>
static int run(const char* name, float a, float b, unsigned long long* dw, unsigned* dat, FILE* out) {
  const unsigned sign = (a < 0.f || b < 0.f) ? 0x80000000u : 0u;
  unsigned lo = bits_of(a) & 0x7fffffffu, hi = bits_of(b) & 0x7fffffffu;
  if (lo > hi) { const unsigned t = lo; lo = hi; hi = t; }
  if (hipMemset(dw, 0, 8) != hipSuccess || hipMemset(dat, 0, 4) != hipSuccess) return 1;
  hipLaunchKernelGGL(sweep<F>, dim3(4096), dim3(256), 0, 0, lo, hi, sign, dw, dat);
  unsigned long long hw = 0;
  unsigned hat = 0;
  if (hipMemcpy(&hw, dw, 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&hat, dat, 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  double w; float x;
  memcpy(&w, &hw, 8); memcpy(&x, &hat, 4);
  for (FILE* f : {stdout, out})
    if (f) fprintf(f, "%-12s [%g, %g]  floats %u  max error %.4f u  (near x = %.9g)\n", name, a, b, hi - lo + 1, w, x);
  return 0;
}

int main(int argc, char** argv) {
  unsigned long long* dw; unsigned* dat;
  if (hipMalloc(&dw, 8) != hipSuccess || hipMalloc(&dat, 4) != hipSuccess) { printf("no device\n"); return 2; }
  FILE* out = argc > 1 ? fopen(argv[1], "w") : nullptr;
  int rc = 0;
  rc |= run<F_EXP2>("exp2", -1.17549435e-38f, -126.f, dw, dat, out);
  rc |= run<F_LOG2>("log2", 1.2037062e-35f, 1024.f, dw, dat, out);           // 2^-116 ... 2^10
  rc |= run<F_EXPF>("expf", -1.17549435e-38f, -87.f, dw, dat, out);
  rc |= run<F_LOG1PF>("log1pf", 1.17549435e-38f, 1.f, dw, dat, out);
  rc |= run<F_LOGF>("logf", 1.f, 1024.f, dw, dat, out);
  rc |= run<F_DEMAP_EXP>("demap_exp", -1.17549435e-38f, -87.f, dw, dat, out);
  rc |= run<F_EXP_CORE>("exp_core", -1.17549435e-38f, -87.f, dw, dat, out);
  rc |= run<F_LOG_CORE>("log_core", 1.2037062e-35f, 1024.f, dw, dat, out);
  if (out) fclose(out);
  return rc;
}
