// The process-wide rocFFT binding and plan cache (defined in ofdm_time.hip): the library is bound lazily with dlopen,
// plans are cached per (device, n, batch, direction, precision) together with their work buffers.
#pragma once
#include "common.h"

namespace samd {

// Batched in-place 1-D complex64 (dbl: complex128) transform of `batch` contiguous rows of length n on `stream`.
// The inverse transform is unnormalised (rocFFT's convention): callers fold the 1/n into their own pass.
int fft_inplace(void* data, int n, int batch, bool inverse, hipStream_t stream, bool dbl = false);

}  // namespace samd
