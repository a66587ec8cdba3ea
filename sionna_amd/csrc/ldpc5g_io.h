// What the hand-written 5G LDPC decoder engines do around their iterations, per codeword: the channel LLRs in (rate
// recovery, clip, logit -> LLR) and the decisions out (info bits or the rate-matched codeword).  One statement of each for
// all engines; the loops over a codeword, their strides and the barriers stay in the kernels.
#pragma once
#include "ldpc5g.h"

namespace samd {

// Channel LLR of VN v from the received row (decoding.py:552-565: clip, then logits -> LLR); 0 for v >= n_vn, the padding
// of the last, partly pruned base column.
// kPlusZero: "+ 0.f" turns -0 into +0, numerically the same LLR.  With it no total and no v2c is ever -0, so the sign bit
// of a v2c equals (v2c < 0): the engines that take a message's sign from its bits need this form - ldpc5g_decode_v2_kernel,
// ldpc5g_decode_ms_kernel, ldpc5g_decode_msg_kernel, ldpc5g_decode_mss_kernel, ldpc5g_decode_ly_kernel and
// ldpc5g_decode_lyrt_kernel.  ldpc5g_decode_bp_kernel uses a message's value alone and keeps the plain form it was written
// with (kPlusZero = false).  (ldpc5g_decode_kernel in ldpc5g.hip has the plain form too, but written out: it calls nothing
// of this header, see profiles/ldpc5g_io_shared_header.md.)
template <bool kPlusZero>
__device__ __forceinline__ float channel_llr(const RateMatch& p, const float* __restrict__ row, int v, int n_vn,
                                             float llr_max) {
  if (kPlusZero) return (v < n_vn) ? (-1.f * clampf(recover_llr(p, row, v, llr_max), -llr_max, llr_max)) + 0.f : 0.f;
  return (v < n_vn) ? -1.f * clampf(recover_llr(p, row, v, llr_max), -llr_max, llr_max) : 0.f;
}

// decision on a marginal x (decoding.py:620-626): clip, then the hard bit or the logit
__device__ __forceinline__ float decide(float x, float llr_max, int hard_out) {
  x = clampf(x, -llr_max, llr_max);
  return hard_out ? ((0.f >= x) ? 1.f : 0.f) : -1.f * x;
}

// Output of codeword b (decoding.py:1486-1531) by the nt threads that hold its marginals, thread tid of them:
// return_infobits: the first k marginals to row b of out[batch][k]; else the n rate-matched positions (output interleaver,
// filler and puncturing undone) to row b of out[batch][n].  marginal: int -> float, the marginal of VN v.
// The row's address is formed inside its branch: with both rows addressed ahead of the branch the kernels come out with
// the same instructions in another order (profiles/ldpc5g_io_shared_header.md).
template <typename Marginal>
__device__ __forceinline__ void store_codeword(const RateMatch& p, float* __restrict__ out, size_t b, Marginal marginal,
                                               float llr_max, int hard_out, int return_infobits, int tid, int nt) {
  if (return_infobits) {
    float* o = out + b * p.k;
    for (int v = tid; v < p.k; v += nt) o[v] = decide(marginal(v), llr_max, hard_out);
  } else {
    float* o = out + b * p.n;
    for (int i = tid; i < p.n; i += nt) o[i] = decide(marginal(short_to_full(p, out_to_short(p, i))), llr_max, hard_out);
  }
}

}  // namespace samd
