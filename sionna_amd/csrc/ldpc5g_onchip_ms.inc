// Body of the explicit-message engine (see ldpc5g_onchip_ms.hip): the kernel template and its launcher for ONE
// check-node rule.  Included by ldpc5g_onchip_ms.hip (min-sum), ldpc5g_onchip_ms_phi.hip and ldpc5g_onchip_ms_tanh.hip -
// one translation unit per rule, so that the three sets of 12 kernels compile in parallel.
#include "ldpc5g_io.h"
#include "bp_math.h"

namespace samd {

// LDS is addressed by plain byte offsets (address space 3): the kernel has no static __shared__ data, so
// the dynamic segment starts at offset 0 (checked once per workgroup) and no base has to be added per access.
typedef __attribute__((address_space(3))) float lds_f32;
// SAMD_MS_ABL (development builds only, `make ablation`; results are WRONG by construction): bit 0 = no node arithmetic
// (values are stored back as loaded), bit 1 = no LDS stores, bit 2 = no LDS loads, bit 3 = no workgroup barriers in the
// iteration loop.  The empty asm statements keep addresses and values alive (no instruction is emitted for them), so
// what remains of the kernel is timed unchanged: tools/gpu_ablation.sh -> where an iteration's time goes.
#ifndef SAMD_MS_ABL
#define SAMD_MS_ABL 0
#endif
__device__ __forceinline__ float lds_ld(unsigned a) {
  if constexpr ((SAMD_MS_ABL & 4) != 0) {
    float v;
    asm volatile("" : "=v"(v) : "v"(a));
    return v;
  } else {
    return *(lds_f32*)(uintptr_t)a;
  }
}
__device__ __forceinline__ void lds_st(unsigned a, float v) {
  if constexpr ((SAMD_MS_ABL & 2) != 0) asm volatile("" : : "v"(a), "v"(v));
  else *(lds_f32*)(uintptr_t)a = v;
}
// full = false: only this wave's LDS operations are waited for before the barrier (a phase exchanges LDS data only; the
// channel LLRs requested from L2 for the next item stay in flight across it)
__device__ __forceinline__ void ms_phase_barrier(bool full = true) {
  if constexpr ((SAMD_MS_ABL & 8) == 0) {
    if (full) __syncthreads();
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
}

__device__ __forceinline__ float ms_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

// min-sum / offset-min-sum check-node arithmetic on the D incoming messages of NCH chunks, in place (v <- c2v):
// second minimum with multiplicity, (m2 - m1) + m1 for a unique minimum (decoding.py:863), no -0 magnitudes.  The layered
// engines (ldpc5g_onchip_ly.hip, ldpc5g_onchip_lyrt.hip) call it; ms_cn_row below holds the same operations (its VAR 1)
// with the fused degree-1 column in.
template <int D, int NCH>
__device__ __forceinline__ void ms_minsum_inplace(float (&v)[NCH][D], float llr_max, float offset) {
  float m1[NCH], m2[NCH];
  unsigned sx[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) { m1[h] = INFINITY; m2[h] = INFINITY; sx[h] = 0u; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      m2[h] = __builtin_amdgcn_fmed3f(m1[h], m2[h], fabsf(v[h][i]));
      m1[h] = __builtin_amdgcn_fmed3f(m1[h], fabsf(v[h][i]), 0.f);
      if (i & 1) sx[h] = __builtin_amdgcn_bitop3_b32(sx[h], __float_as_uint(v[h][i - 1]), __float_as_uint(v[h][i]), 0x96);
      else if (i == D - 1) sx[h] ^= __float_as_uint(v[h][i]);
    }
  float a1[NCH], a2[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const float min_e = (m2[h] > m1[h]) ? ((m2[h] - m1[h]) + m1[h]) : m1[h];
    a1[h] = __builtin_amdgcn_fmed3f(m1[h] - offset, 0.f, llr_max);
    a2[h] = __builtin_amdgcn_fmed3f(min_e - offset, 0.f, llr_max);
    sx[h] &= 0x80000000u;
    a1[h] = __uint_as_float(__float_as_uint(a1[h]) | sx[h]);
    a2[h] = __uint_as_float(__float_as_uint(a2[h]) | sx[h]);
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const float mag = (fabsf(v[h][i]) == m1[h]) ? a2[h] : a1[h];
      v[h][i] = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(mag), __float_as_uint(v[h][i]), 0x80000000u, 0x78));
    }
}

// one check node per lane and chunk: row of exact degree D, its messages are D lane-contiguous blocks from byte a0.
// NCH: consecutive 64-lane chunks of lifted copies handled in one pass (lane z and lane z+64 share every
// scalar and every address register - the second chunk is the same address + 256 bytes): two independent
// dependency chains per wave and half as many work items (their dispatch is scalar overhead).
// FUSE1: the row's last edge goes to a degree-1 variable node of the same lane (identity block of the base
// graph's extension part).  Its VN update - x = c2v + llr, v2c = clip(x - c2v) - is done right here, so
// these columns (42 of C2's 68) never appear in the VN phase; llr_v points at that VN's channel LLR.
// MODE: SAMD_CN_MINSUM (min-sum and, through `offset`, offset-min-sum: the arithmetic below) or one of the boxplus
// rules (bp_math.h's cn_update_col on the D messages of a chunk - the same function, hence the same bits, as the HBM
// engine and ldpc5g_onchip_bp.hip).
// Z4C: 4 Z as a compile-time constant (0: run-time z4) - the D block addresses then are ONE address register plus
// the offset fields of the DS instructions (no address arithmetic, D - 1 registers less).
// VAR 1: gfx950's three-input bit operation (v_bitop3_b32) in the sign arithmetic - the node sign as one xor3 per TWO
// edges, the row sign folded into the two candidate magnitudes once per row, own sign applied with sel ^ (v & msb) in
// one operation: 5.5 instead of 7 vector operations per edge and chunk, the same bits.  The grouped kernel's min-sum bodies
// are VAR 1; the list-walking kernel (ldpc5g_decode_ms_kernel) keeps VAR 0, the two-input form.
template <int D, int NCH, bool FUSE1, int MODE, unsigned Z4C = 0, int VAR = 0>
__device__ __forceinline__ void ms_cn_row(unsigned a0, unsigned z4r, float llr_max, float offset,
                                          float* __restrict__ llr_v, bool last, unsigned phi_base = kPhiNoLds) {
  const unsigned z4 = Z4C ? Z4C : z4r;
  float v[NCH][D];
  unsigned a[D];
  float lf[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) lf[h] = FUSE1 ? llr_v[64 * h] : 0.f;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    a[i] = Z4C ? a0 + (unsigned)i * Z4C : (i ? a[i - 1] + z4 : a0);
#pragma unroll
    for (int h = 0; h < NCH; ++h) v[h][i] = lds_ld(a[i] + 256u * h);
  }
  if constexpr (MODE != SAMD_CN_MINSUM) {
#pragma unroll
    // (boxplus-phi: the table of the defined logarithm is staged in LDS by the kernel, bp_math.h - a compile-time choice:
    // a run-time selection between LDS and global memory inside the gather cost a factor of two, profiles/r05g_phi_rate.txt)
    for (int h = 0; h < NCH; ++h) cn_update_col<MODE, D, PhiTabLds>(v[h], D, llr_max, 0.f, PhiTabLds{phi_base});    // in place: v[h][i] = c2v
#pragma unroll
    for (int i = 0; i < D; ++i) {
      float c2v[NCH];
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        c2v[h] = v[h][i];
        if (FUSE1 && i == D - 1) {
          const float x = c2v[h] + lf[h];
          if (last) llr_v[64 * h] = x;
          c2v[h] = ms_med3(x - c2v[h], -llr_max, llr_max);
        }
      }
#pragma unroll
      for (int h = 0; h < NCH; ++h) lds_st(a[i] + 256u * h, c2v[h]);
    }
    return;
  }
  if constexpr ((SAMD_MS_ABL & 1) != 0) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int h = 0; h < NCH; ++h) lds_st(a[i] + 256u * h, v[h][i] + lf[h]);
    return;
  }
  float m1[NCH], m2[NCH];
  unsigned sx[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) { m1[h] = INFINITY; m2[h] = INFINITY; sx[h] = 0u; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      m2[h] = ms_med3(m1[h], m2[h], fabsf(v[h][i]));      // second smallest, with multiplicity
      m1[h] = ms_med3(m1[h], fabsf(v[h][i]), 0.f);        // = min(m1, |v|) for non-negative values, one operation
      if (VAR == 0) sx[h] ^= __float_as_uint(v[h][i]);    // bit 31 = node sign
      else if (i & 1) sx[h] = __builtin_amdgcn_bitop3_b32(sx[h], __float_as_uint(v[h][i - 1]), __float_as_uint(v[h][i]), 0x96);
      else if (i == D - 1) sx[h] ^= __float_as_uint(v[h][i]);
    }
  float a1[NCH], a2[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    // unique minimum <=> m2 > m1; (m2 - m1) + m1 is the reference's arithmetic (decoding.py:863)
    const float min_e = (m2[h] > m1[h]) ? ((m2[h] - m1[h]) + m1[h]) : m1[h];
    a1[h] = ms_med3(m1[h] - offset, 0.f, llr_max);      // plain min-sum: offset = 0 (exact)
    a2[h] = ms_med3(min_e - offset, 0.f, llr_max);
    if (VAR == 1) {                                      // row sign into both candidates (their sign bits are 0)
      sx[h] &= 0x80000000u;
      a1[h] = __uint_as_float(__float_as_uint(a1[h]) | sx[h]);
      a2[h] = __uint_as_float(__float_as_uint(a2[h]) | sx[h]);
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float c2v[NCH];
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const float mag = (fabsf(v[h][i]) == m1[h]) ? a2[h] : a1[h];
      if (VAR == 1) {
        // mag carries the node sign: c2v = mag ^ (v & msb), truth table 0x78 of (mag, v, msb)
        c2v[h] = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(mag), __float_as_uint(v[h][i]), 0x80000000u, 0x78));
      } else {
        const unsigned sg = (__float_as_uint(v[h][i]) ^ sx[h]) & 0x80000000u;   // own sign x node sign
        c2v[h] = __uint_as_float(sg | __float_as_uint(mag));
      }
      if (FUSE1 && i == D - 1) {
        const float x = c2v[h] + lf[h];             // (0 + c2v) + llr; llr is never -0, so 0 + c2v needs no operation
        if (last) llr_v[64 * h] = x;
        c2v[h] = ms_med3(x - c2v[h], -llr_max, llr_max);   // the slot now holds the next v2c
      }
    }
#pragma unroll
    for (int h = 0; h < NCH; ++h) lds_st(a[i] + 256u * h, c2v[h]);   // adjacent: one ds_write2st64_b32 per pair
  }
}

// one variable node per lane and chunk, column of exact degree D.  ent[2i] = edge block byte offset,
// ent[2i+1] = 4 shift; zwv: 4Z-1 (POW2) or 4Z, in a VGPR so that (t & zw) | base is one v_and_or_b32
// l0 / l1: channel LLRs of the lane's VN in chunk 0 / 1 (fetched by the caller one item ahead)
typedef float ms_f32x2 __attribute__((ext_vector_type(2)));

// X128 (Z = 128, pair items): the second chunk's block position is the first one's with bit 8 flipped -
// ((t + 256) mod 512) = (t mod 512) ^ 256 - one v_xor instead of an add and an and_or
template <int D, int NCH, bool POW2, bool INIT, bool X128 = false>
__device__ __forceinline__ void ms_vn_col(const int32_t* __restrict__ ent, unsigned zz4, unsigned zwv,
                                          float* __restrict__ llr_v, float l0, float l1, float llr_max, bool last) {
  unsigned a[NCH][D];
  float c[NCH][D];
  float l[NCH], x[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) { l[h] = h ? l1 : l0; x[h] = 0.f; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const unsigned t = zz4 + 256u * h - (unsigned)ent[2 * i + 1];
      // edge blocks are aligned to 4Z when Z is a power of two: (t mod 4Z) | base
      // (inline asm: written as C, the compiler re-derives the address from its parts - and, move, v_bitop3 - 5 operations)
      if (X128 && h == 1) asm("v_xor_b32_e32 %0, 0x100, %1" : "=v"(a[h][i]) : "v"(a[0][i]));
      else a[h][i] = POW2 ? ((t & zwv) | (unsigned)ent[2 * i]) : (min(t, t + zwv) + (unsigned)ent[2 * i]);
      if (INIT) lds_st(a[h][i], l[h]);
      else c[h][i] = lds_ld(a[h][i]);
    }
  if (INIT) return;
  if constexpr ((SAMD_MS_ABL & 1) != 0) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int h = 0; h < NCH; ++h) lds_st(a[h][i], c[h][i] + l[h]);
    return;
  }
  if constexpr (NCH == 2) {
    // both chunks of an edge in one packed-fp32 operation (v_pk_add_f32: two IEEE additions per issue slot, the
    // same results as two v_add_f32): x += c and x - c cost one VALU operation per edge instead of two
    ms_f32x2 xv = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < D; ++i) xv += ms_f32x2{c[0][i], c[1][i]};
    xv += ms_f32x2{l[0], l[1]};
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const ms_f32x2 e = xv - ms_f32x2{c[0][i], c[1][i]};
      lds_st(a[0][i], ms_med3(e.x, -llr_max, llr_max));
      lds_st(a[1][i], ms_med3(e.y, -llr_max, llr_max));
    }
    if (last) { llr_v[0] = xv.x; llr_v[64] = xv.y; }
  } else {
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
#pragma unroll
      for (int i = 0; i < D; ++i) x[h] += c[h][i];
      x[h] += l[h];
#pragma unroll
      for (int i = 0; i < D; ++i) lds_st(a[h][i], ms_med3(x[h] - c[h][i], -llr_max, llr_max));
      if (last) llr_v[64 * h] = x[h];
    }
  }
}


template <bool POW2, bool INIT>
__device__ __forceinline__ void ms_vn_item(const int32_t* __restrict__ ent, int d, unsigned zz4, unsigned zwv,
                                           float* __restrict__ llr_v, float l0, float l1, float llr_max, bool last) {
#define SAMD_MS_VN(D) case D: ms_vn_col<D, 1, POW2, INIT>(ent, zz4, zwv, llr_v, l0, l1, llr_max, last); break
#define SAMD_MS_VN2(D) case 32 + D: ms_vn_col<D, 2, POW2, INIT>(ent, zz4, zwv, llr_v, l0, l1, llr_max, last); break
  switch (d) {                                                       // degree | pair << 5
    SAMD_MS_VN(1); SAMD_MS_VN(2); SAMD_MS_VN(3); SAMD_MS_VN(4); SAMD_MS_VN(5); SAMD_MS_VN(6); SAMD_MS_VN(7);
    SAMD_MS_VN(8); SAMD_MS_VN(9); SAMD_MS_VN(10); SAMD_MS_VN(11); SAMD_MS_VN(12); SAMD_MS_VN(13); SAMD_MS_VN(14);
    SAMD_MS_VN(15); SAMD_MS_VN(16); SAMD_MS_VN(17); SAMD_MS_VN(18); SAMD_MS_VN(19); SAMD_MS_VN(20); SAMD_MS_VN(21);
    SAMD_MS_VN(22); SAMD_MS_VN(23); SAMD_MS_VN(24); SAMD_MS_VN(25); SAMD_MS_VN(26); SAMD_MS_VN(27); SAMD_MS_VN(28);
    SAMD_MS_VN(29); SAMD_MS_VN(30);
    SAMD_MS_VN2(1); SAMD_MS_VN2(2); SAMD_MS_VN2(3); SAMD_MS_VN2(4); SAMD_MS_VN2(5); SAMD_MS_VN2(6); SAMD_MS_VN2(7);
    SAMD_MS_VN2(8); SAMD_MS_VN2(9); SAMD_MS_VN2(10); SAMD_MS_VN2(11); SAMD_MS_VN2(12);
    default: break;
  }
#undef SAMD_MS_VN
#undef SAMD_MS_VN2
}

// single-chunk columns only: the call sites of packed-tail items, whose edge table pointer is a per-lane value (the
// loads of ms_vn_col then become vector loads - the same function, inlined a second time)
template <bool POW2, bool INIT>
__device__ __forceinline__ void ms_vn_item_single(const int32_t* __restrict__ ent, int d, unsigned zz4, unsigned zwv,
                                                  float* __restrict__ llr_v, float l0, float llr_max, bool last) {
#define SAMD_MS_VN(D) case D: ms_vn_col<D, 1, POW2, INIT>(ent, zz4, zwv, llr_v, l0, 0.f, llr_max, last); break
  switch (d) {
    SAMD_MS_VN(1); SAMD_MS_VN(2); SAMD_MS_VN(3); SAMD_MS_VN(4); SAMD_MS_VN(5); SAMD_MS_VN(6); SAMD_MS_VN(7);
    SAMD_MS_VN(8); SAMD_MS_VN(9); SAMD_MS_VN(10); SAMD_MS_VN(11); SAMD_MS_VN(12); SAMD_MS_VN(13); SAMD_MS_VN(14);
    SAMD_MS_VN(15); SAMD_MS_VN(16); SAMD_MS_VN(17); SAMD_MS_VN(18); SAMD_MS_VN(19); SAMD_MS_VN(20); SAMD_MS_VN(21);
    SAMD_MS_VN(22); SAMD_MS_VN(23); SAMD_MS_VN(24); SAMD_MS_VN(25); SAMD_MS_VN(26); SAMD_MS_VN(27); SAMD_MS_VN(28);
    SAMD_MS_VN(29); SAMD_MS_VN(30);
    default: break;
  }
#undef SAMD_MS_VN
}

// list entries are self-contained (no dependent table look-ups) and the next one is fetched while the current
// item runs:  VN (c | chunk<<8 | degree<<16,  dword offset of the column's edge table),
//             CN (row block byte offset | degree<<18 | fused<<23 | pair<<24,  r | chunk<<8 | fused column<<16)
// a pair item covers chunks (chunk, chunk+1), all 128 lanes valid; VN degree field = degree | pair<<5
// vn_ptr = [NW+1 offsets of the per-iteration lists | NW+1 offsets of the fused degree-1 columns (init only)]
#if defined(SAMD_MS_TRACE) && defined(SAMD_MS_MAIN_TU)
// Development aid (tools/ms_trace.py; not part of the product build): per-wave timestamps of workgroup 0 at the phase
// boundaries of iterations 2..5 -> where the time of an iteration goes (CN items, barrier wait, VN items, barrier wait).
__device__ unsigned long long* g_ms_trace = nullptr;
#define SAMD_TRACE_MARK(slot)                                                                               \
  if (g_ms_trace && blockIdx.x == 0 && it >= 2 && it < 6 && lane == 0)                                        \
    g_ms_trace[((it - 2) * 5 + (slot)) * NW + w] = __builtin_readcyclecounter();
// item-level trace of the grouped kernel (iteration 3 of workgroup 0): per wave up to 24 records (tag, time) behind the
// phase marks above; tag = 1000 CN phase start, KEY after a CN item, 2000 VN phase start, 2000 + KEY after a VN item,
// 3000 after the second barrier
#define SAMD_ITRACE(tag)                                                                                    \
  if (g_ms_trace && blockIdx.x == 0 && it == 3 && lane == 0 && itr_slot < 24) {                               \
    g_ms_trace[320 + (w * 24 + itr_slot) * 2] = (unsigned long long)(tag);                                    \
    g_ms_trace[320 + (w * 24 + itr_slot) * 2 + 1] = __builtin_readcyclecounter();                             \
    ++itr_slot;                                                                                             \
  }
#else
#define SAMD_TRACE_MARK(slot)
#define SAMD_ITRACE(tag)
#endif

// PACK: the lists contain packed-tail items (lifting sizes that are not multiples of 64).  A template argument, not a
// run-time branch: with the packed paths merely present, the ordinary items of C2 ran 5 % slower.
template <bool POW2, int NW, bool LLRG, int MODE, bool PACK>
__global__ __launch_bounds__(NW * 64) void ldpc5g_decode_ms_kernel(
    const float* __restrict__ llr_in, float* __restrict__ out, float* __restrict__ llr_ws, RateMatch p, int n_cn,
    int nbu, int batch, int num_iter, float llr_max, float offset, int hard_out, int return_infobits,
    int msg_floats, const int32_t* __restrict__ col_ent, const int32_t* __restrict__ cn_ptr,
    const int2* __restrict__ cn_list, const int32_t* __restrict__ vn_ptr, const int2* __restrict__ vn_list,
    const int2* __restrict__ tail_tab, int tail_sh, const int2* __restrict__ vtail_tab, int phi_lds) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((unsigned)(size_t)(lds_f32*)smem != 0u) __builtin_trap();      // see lds_ld
  constexpr int NT = NW * 64;
  // boxplus-phi: the 512-byte table of the defined logarithm behind the messages (and the LLRs) when the launch reserved it
  const unsigned phi_base = (MODE == SAMD_CN_BOXPLUS_PHI && phi_lds) ? 4u * (unsigned)(msg_floats + (LLRG ? 0 : nbu * p.z)) : kPhiNoLds;
  if (phi_base != kPhiNoLds) { phi_tab_stage(phi_base, (int)threadIdx.x); __syncthreads(); }
  const unsigned z = (unsigned)p.z, z4 = 4u * z;
  const unsigned zw = POW2 ? z4 - 1u : z4;
  unsigned zwv;
  asm volatile("v_mov_b32 %0, %1" : "=v"(zwv) : "s"(zw));
  const int n_vn = p.n_vn;
  const int nx = nbu * (int)z;
  float* llr = LLRG ? llr_ws + (size_t)blockIdx.x * nx : smem + msg_floats;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = cn_ptr[w], c1 = cn_ptr[w + 1];
  const int v0 = vn_ptr[w], v1 = vn_ptr[w + 1];
  const int f0 = vn_ptr[NW + 1 + w], f1 = vn_ptr[NW + 2 + w];

  // packed-tail VN item (bit 22 of its first dword): lane group g = lane >> tail_sh works for column vtail_tab[base + g]
  // (x = dword offset of the column's edge table, y = column or 0xFF); returns the lane's VN index or -1
  auto vtail = [&](int d0, int d1, unsigned& zz, const int32_t*& ent) __attribute__((always_inline)) -> int {
    const int2 te = vtail_tab[d1 + (int)((unsigned)lane >> tail_sh)];
    const int c = te.y & 0xFF;
    zz = (unsigned)(((d0 >> 8) & 0xFF) * 64) + ((unsigned)lane & ((1u << tail_sh) - 1u));
    ent = col_ent + te.x;
    const int vn = c * (int)z + (int)zz;
    return (c != 0xFF && zz < z && vn < n_vn) ? vn : -1;
  };

  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    const float* row = llr_in + (size_t)b * p.n;
    for (int v = tid; v < nx; v += NT) llr[v] = channel_llr<true>(p, row, v, n_vn, llr_max);
    __syncthreads();
    for (int seg = 0; seg < 2; ++seg) {                              // v2c of iteration 0 = channel LLR, all columns
      const int t0 = seg ? f0 : v0, t1 = seg ? f1 : v1;
      for (int t = t0; t < t1; ++t) {
        const int2 e = vn_list[t];
        const int d0 = __builtin_amdgcn_readfirstlane(e.x), d1 = __builtin_amdgcn_readfirstlane(e.y);
        if (PACK && ((d0 >> 22) & 1)) {
          unsigned zp;
          const int32_t* entp;
          const int vp = vtail(d0, d1, zp, entp);
          if (vp >= 0) ms_vn_item_single<POW2, true>(entp, (d0 >> 16) & 31, 4u * zp, zwv, llr + vp, llr[vp], llr_max, false);
          continue;
        }
        const int c = d0 & 0xFF;
        const unsigned zz = (unsigned)(((d0 >> 8) & 0xFF) * 64 + lane);
        const int vn = c * (int)z + (int)zz;
        const bool pr = (d0 >> 21) & 1;
        if (pr || (zz < z && vn < n_vn))
          ms_vn_item<POW2, true>(col_ent + d1, (d0 >> 16) & 63, 4u * zz, zwv, llr + vn, llr[vn], pr ? llr[vn + 64] : 0.f, llr_max, false);
      }
    }
    __syncthreads();

    for (int it = 0; it < num_iter; ++it) {
      const bool last = (it == num_iter - 1);
      SAMD_TRACE_MARK(0)
      // vn_fetch: descriptor and channel LLRs of this wave's first VN item, in flight during the CN phase
      int2 vfirst = make_int2(0, 0);
      float lf0 = 0.f, lf1 = 0.f;
      if (v0 < v1) {
        vfirst = vn_list[v0];
        const int e0 = __builtin_amdgcn_readfirstlane(vfirst.x);
        if (PACK && ((e0 >> 22) & 1)) {
          unsigned zp;
          const int32_t* entp;
          const int vp = vtail(e0, __builtin_amdgcn_readfirstlane(vfirst.y), zp, entp);
          if (vp >= 0) lf0 = llr[vp];
        } else {
          const int vn2 = (e0 & 0xFF) * (int)z + ((e0 >> 8) & 0xFF) * 64 + lane;
          const bool pr2 = (e0 >> 21) & 1;
          if (pr2 || vn2 < n_vn) lf0 = llr[vn2];
          if (pr2) lf1 = llr[vn2 + 64];
        }
      }
      {
        int2 nxt = c0 < c1 ? cn_list[c0] : make_int2(0, 0);
        for (int t = c0; t < c1; ++t) {
          const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(nxt.x);
          const int d1 = __builtin_amdgcn_readfirstlane(nxt.y);
          if (t + 1 < c1) nxt = cn_list[t + 1];
          onchip_setprio(d1 >> 24);
#define SAMD_MS_CN(D) case D: ms_cn_row<D, 1, false, MODE>(a0, z4, llr_max, offset, lv, last, phi_base); break
#define SAMD_MS_CNF(D) case 32 + D: ms_cn_row<D, 1, true, MODE>(a0, z4, llr_max, offset, lv, last, phi_base); break
#define SAMD_MS_CN2(D) case 64 + D: ms_cn_row<D, 2, false, MODE>(a0, z4, llr_max, offset, lv, last, phi_base); break
#define SAMD_MS_CNF2(D) case 96 + D: ms_cn_row<D, 2, true, MODE>(a0, z4, llr_max, offset, lv, last, phi_base); break
#define SAMD_MS_SINGLES                                                                                             \
  SAMD_MS_CN(3); SAMD_MS_CN(4); SAMD_MS_CN(5); SAMD_MS_CN(6); SAMD_MS_CN(7); SAMD_MS_CN(8); SAMD_MS_CN(9);            \
  SAMD_MS_CN(10); SAMD_MS_CN(19);                                                                                   \
  SAMD_MS_CNF(3); SAMD_MS_CNF(4); SAMD_MS_CNF(5); SAMD_MS_CNF(6); SAMD_MS_CNF(7); SAMD_MS_CNF(8); SAMD_MS_CNF(9);     \
  SAMD_MS_CNF(10);
          if (PACK && ((d1 >> 26) & 1)) {
            // packed tails (Z not a multiple of 64): the last, partial chunks of up to 64 / gw rows of the same degree
            // share one pass - lane group g = lane / gw works for row tail_tab[base + g] (row block offset, r | fused
            // column).  Its own copy of the single-chunk bodies: row and column are per-lane values here, and the
            // scalar ones of the ordinary items must stay scalar (C2 lost 4 % when the two shared the code).
            const unsigned gl = (unsigned)lane & ((1u << tail_sh) - 1u);
            const int2 te = tail_tab[(ro & 0x3FFFFu) + ((unsigned)lane >> tail_sh)];
            const unsigned r = (unsigned)te.y & 0xFFu;
            const unsigned zz = (unsigned)(((d1 >> 8) & 0xFF) * 64) + gl;
            const unsigned a0 = (unsigned)te.x + 4u * zz;
            if (r != 0xFFu && zz < z) {
              if (r * z + zz < (unsigned)n_cn) {
                float* lv = llr + (int)(((unsigned)te.y >> 16) & 0xFFu) * (int)z + (int)zz;
                switch ((ro >> 18) & 63u) {                          // degree | fused << 5
                  SAMD_MS_SINGLES
                  default: break;
                }
              } else {
                for (unsigned i = 0; i < ((ro >> 18) & 31u); ++i) lds_st(a0 + i * z4, 0.f);   // pruned check node, see below
              }
            }
          } else {
            const int r = d1 & 0xFF;
            const unsigned zz = (unsigned)(((d1 >> 8) & 0xFF) * 64 + lane);
            const unsigned a0 = (ro & 0x3FFFFu) + 4u * zz;
            if (((ro >> 24) & 1u) || (zz < z && (unsigned)r * z + zz < (unsigned)n_cn)) {
              float* lv = llr + ((d1 >> 16) & 0xFF) * (int)z + (int)zz;   // channel LLR of the fused degree-1 VN
              switch (ro >> 18) {                                    // degree | fused << 5 | pair << 6
                SAMD_MS_SINGLES
                SAMD_MS_CN2(3); SAMD_MS_CN2(4); SAMD_MS_CN2(5); SAMD_MS_CN2(6); SAMD_MS_CN2(7); SAMD_MS_CN2(8);
                SAMD_MS_CN2(9); SAMD_MS_CN2(10); SAMD_MS_CN2(19);
                SAMD_MS_CNF2(3); SAMD_MS_CNF2(4); SAMD_MS_CNF2(5); SAMD_MS_CNF2(6); SAMD_MS_CNF2(7); SAMD_MS_CNF2(8);
                SAMD_MS_CNF2(9); SAMD_MS_CNF2(10);
                default: break;
              }
            } else if (zz < z) {
              // pruned check node of the last, partial base row: its edges do not exist - keep their slots at 0
              for (unsigned i = 0; i < ((ro >> 18) & 31u); ++i) lds_st(a0 + i * z4, 0.f);
            }
          }
#undef SAMD_MS_SINGLES
#undef SAMD_MS_CN2
#undef SAMD_MS_CNF2
#undef SAMD_MS_CN
#undef SAMD_MS_CNF
        }
      }
      SAMD_TRACE_MARK(1)
      __syncthreads();
      SAMD_TRACE_MARK(2)
      {
        // the channel LLRs of an item are fetched one item ahead (the first item's before the CN phase, see
        // vn_fetch above): an L2 round trip is longer than a whole VN item
        int2 cur = vfirst;
        float l0 = lf0, l1 = lf1;
        for (int t = v0; t < v1; ++t) {
          const int d0 = __builtin_amdgcn_readfirstlane(cur.x), d1 = __builtin_amdgcn_readfirstlane(cur.y);
          int2 nxt = make_int2(0, 0);
          float n0 = 0.f, n1 = 0.f;
          if (t + 1 < v1) {
            nxt = vn_list[t + 1];
            const int e0 = __builtin_amdgcn_readfirstlane(nxt.x);
            if (PACK && ((e0 >> 22) & 1)) {
              unsigned zp;
              const int32_t* entp;
              const int vp = vtail(e0, __builtin_amdgcn_readfirstlane(nxt.y), zp, entp);
              if (vp >= 0) n0 = llr[vp];
            } else {
              const int vn2 = (e0 & 0xFF) * (int)z + ((e0 >> 8) & 0xFF) * 64 + lane;
              const bool pr2 = (e0 >> 21) & 1;
              if (pr2 || vn2 < n_vn) n0 = llr[vn2];
              if (pr2) n1 = llr[vn2 + 64];
            }
          }
          onchip_setprio(d0 >> 24);
          if (PACK && ((d0 >> 22) & 1)) {
            unsigned zp;
            const int32_t* entp;
            const int vp = vtail(d0, d1, zp, entp);
            if (vp >= 0) ms_vn_item_single<POW2, false>(entp, (d0 >> 16) & 31, 4u * zp, zwv, llr + vp, l0, llr_max, last);
          } else {
            const int c = d0 & 0xFF;
            const unsigned zz = (unsigned)(((d0 >> 8) & 0xFF) * 64 + lane);
            const int vn = c * (int)z + (int)zz;
            if (((d0 >> 21) & 1) || (zz < z && vn < n_vn))
              ms_vn_item<POW2, false>(col_ent + d1, (d0 >> 16) & 63, 4u * zz, zwv, llr + vn, l0, l1, llr_max, last);
          }
          cur = nxt; l0 = n0; l1 = n1;
        }
      }
      SAMD_TRACE_MARK(3)
      __syncthreads();
      SAMD_TRACE_MARK(4)
    }
    // llr[] now holds the marginals
    store_codeword(p, out, (size_t)b, [&](int v) { return llr[v]; }, llr_max, hard_out,
                   return_infobits, tid, NT);
    __syncthreads();
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// Grouped dispatch (round 3).  In the kernel above every work item pays for finding its body: the `switch` over
// (degree, fused, pair) is a compare-and-branch tree (AMDGPU has no jump tables) - 7 levels, ~10 taken branches and ~45
// scalar instructions per item against 130-300 vector instructions of the body itself, 14 items per wave and
// iteration, issued in order by the one wave that needs them.  Here the host sorts the items of a wave by body type and
// hands over GROUPS (type, first item, last item): the tree is walked once per group (3-5 per wave and phase), the items
// of a group run in a loop around ONE body whose per-item cost is a descriptor (fetched one item ahead), two address
// adds and - only when it changes - the issue priority.  Same bodies (ms_cn_row / ms_vn_col), same arithmetic, same
// lists of work per wave as the LPT split above, hence the same bits.  Engine of the codes whose items are all full
// chunk pairs: Z a multiple of 128, no partially pruned base row (n_cn, n_vn multiples of Z), 16 waves - config C2.
//   CN item  x = row block byte offset + 256 * chunk | priority << 24,  y = element offset of the fused degree-1 VN
//   VN item  x = element offset of the VN chunk (c Z + 64 chunk) | pair << 23 | priority << 24,  y = dword offset of the column's
//            edge table | chunk << 20
//   group    x = body type (CN: degree | fused << 5; VN: degree | pair << 5),  y = first item | (last + 1) << 16
// ZM: 0 = any Z (multiple of 128), 1 = Z a power of two, 2 = Z = 128 (block stride and chunk flip at compile time)
template <int ZM, bool LLRG, int MODE>
__global__ __launch_bounds__(1024) void ldpc5g_decode_msg_kernel(
    const float* __restrict__ llr_in, float* __restrict__ out, float* __restrict__ llr_ws, RateMatch p, int n_cn,
    int nbu, int batch, int num_iter, float llr_max, float offset, int hard_out, int return_infobits,
    int msg_floats, const int32_t* __restrict__ col_ent, const int32_t* __restrict__ vn_ptr,
    const int2* __restrict__ vn_list, const int32_t* __restrict__ g_ptr, const int2* __restrict__ g_cn,
    const int2* __restrict__ g_vn, const int2* __restrict__ i_cn, const int2* __restrict__ i_vn, int lds_bar, int phi_lds
    ) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((unsigned)(size_t)(lds_f32*)smem != 0u) __builtin_trap();      // see lds_ld
  constexpr int NW = 16, NT = NW * 64;
  const unsigned phi_base = (MODE == SAMD_CN_BOXPLUS_PHI && phi_lds) ? 4u * (unsigned)(msg_floats + (LLRG ? 0 : nbu * p.z)) : kPhiNoLds;
  if (phi_base != kPhiNoLds) { phi_tab_stage(phi_base, (int)threadIdx.x); __syncthreads(); }
  constexpr bool POW2 = ZM >= 1;
  constexpr int VAR = MODE == SAMD_CN_MINSUM ? 1 : 0;                  // the bit-operation variant exists for min-sum only
  constexpr unsigned Z4C = ZM == 2 ? 512u : 0u;
  const unsigned z = ZM == 2 ? 128u : (unsigned)p.z, z4 = 4u * z;
  const unsigned zw = POW2 ? z4 - 1u : z4;
  unsigned zwv;
  asm volatile("v_mov_b32 %0, %1" : "=v"(zwv) : "s"(zw));
  const int n_vn = p.n_vn;
  const int nx = nbu * (int)z;
  float* llr = LLRG ? llr_ws + (size_t)blockIdx.x * nx : smem + msg_floats;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned lane4 = 4u * (unsigned)lane;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int v0 = vn_ptr[w], v1 = vn_ptr[w + 1];
  const int f0 = vn_ptr[NW + 1 + w], f1 = vn_ptr[NW + 2 + w];
  const int gc0 = g_ptr[w], gc1 = g_ptr[w + 1];                        // this wave's CN groups
  const int gv0 = g_ptr[NW + 1 + w], gv1 = g_ptr[NW + 2 + w];          // ... and VN groups
  // first VN item of the wave (its channel LLRs are requested before the CN phase)
  const int vfirst_i = gv0 < gv1 ? (__builtin_amdgcn_readfirstlane(g_vn[gv0].y) & 0xFFFF) : -1;
  const int vend_i = gv0 < gv1 ? (int)((unsigned)__builtin_amdgcn_readfirstlane(g_vn[gv1 - 1].y) >> 16) : -1;   // one past the wave's last VN item

  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    const float* row = llr_in + (size_t)b * p.n;
    for (int v = tid; v < nx; v += NT) llr[v] = channel_llr<true>(p, row, v, n_vn, llr_max);
    __syncthreads();
    for (int seg = 0; seg < 2; ++seg) {                              // v2c of iteration 0 = channel LLR, all columns
      const int t0 = seg ? f0 : v0, t1 = seg ? f1 : v1;
      for (int t = t0; t < t1; ++t) {
        const int2 e = vn_list[t];
        const int d0 = __builtin_amdgcn_readfirstlane(e.x), d1 = __builtin_amdgcn_readfirstlane(e.y);
        const int c = d0 & 0xFF;
        const unsigned zz = (unsigned)(((d0 >> 8) & 0xFF) * 64 + lane);
        const int vn = c * (int)z + (int)zz;
        const bool pr = (d0 >> 21) & 1;
        if (pr || (zz < z && vn < n_vn))
          ms_vn_item<POW2, true>(col_ent + d1, (d0 >> 16) & 63, 4u * zz, zwv, llr + vn, llr[vn], pr ? llr[vn + 64] : 0.f, llr_max, false);
      }
    }
    __syncthreads();

    int cur_prio = -1;
    [[maybe_unused]] int itr_slot = 0;
    for (int it = 0; it < num_iter; ++it) {
      const bool last = (it == num_iter - 1);
      float lf0 = 0.f, lf1 = 0.f;
      int2 vfirst = make_int2(0, 0), vsecond = make_int2(0, 0);
      SAMD_ITRACE(1000)
      if (vfirst_i >= 0) {
        vfirst = i_vn[vfirst_i];
        if (vfirst_i + 1 < vend_i) vsecond = i_vn[vfirst_i + 1];
        const int e0 = __builtin_amdgcn_readfirstlane(vfirst.x);
        lf0 = llr[(e0 & 0x7FFFFF) + lane];
        if ((e0 >> 23) & 1) lf1 = llr[(e0 & 0x7FFFFF) + lane + 64];   // pair item: the second chunk's channel LLR
      }
      // ---------------- CN phase
      for (int g = gc0; g < gc1; ++g) {
        const int2 G = g_cn[g];
        const int key = __builtin_amdgcn_readfirstlane(G.x);
        const int gy = __builtin_amdgcn_readfirstlane(G.y);
        const int tb = gy & 0xFFFF, te = (unsigned)gy >> 16;
#define SAMD_MSG_CN_(KEY, D, F, NCHC)                                                                             \
  case KEY: {                                                                                                     \
    int2 nxt = i_cn[tb];                                                                                          \
    for (int t = tb; t < te; ++t) {                                                                               \
      const unsigned ix = (unsigned)__builtin_amdgcn_readfirstlane(nxt.x);                                        \
      const int iy = __builtin_amdgcn_readfirstlane(nxt.y);                                                       \
      if (t + 1 < te) nxt = i_cn[t + 1];                                                                          \
      const int pr = (int)(ix >> 24);                                                                             \
      if (pr != cur_prio) { onchip_setprio(pr); cur_prio = pr; }                                                  \
      ms_cn_row<D, NCHC, F, MODE, Z4C, VAR>((ix & 0xFFFFFFu) + lane4, z4, llr_max, offset, llr + iy + lane, last, phi_base); \
      SAMD_ITRACE(KEY)                                                                                            \
    }                                                                                                             \
  } break;
        // (key + 64: one chunk of the row - the host cuts pair items of the busiest wave where that balances the phase;
        // only for the fused rows of degree 4 ... 7, the small items that fill gaps: with all 17 single-chunk bodies in
        // the kernel the items that do not use them ran 2 % slower, profiles/r03b/ms_refine_cn_r03z.txt)
#define SAMD_MSG_CN(KEY, D, F) SAMD_MSG_CN_(KEY, D, F, 2)
        switch (key) {
          SAMD_MSG_CN_(64 + 37, 5, true, 1) SAMD_MSG_CN_(64 + 38, 6, true, 1)
          SAMD_MSG_CN(3, 3, false) SAMD_MSG_CN(4, 4, false) SAMD_MSG_CN(5, 5, false) SAMD_MSG_CN(6, 6, false)
          SAMD_MSG_CN(7, 7, false) SAMD_MSG_CN(8, 8, false) SAMD_MSG_CN(9, 9, false) SAMD_MSG_CN(10, 10, false)
          SAMD_MSG_CN(19, 19, false)
          SAMD_MSG_CN(35, 3, true) SAMD_MSG_CN(36, 4, true) SAMD_MSG_CN(37, 5, true) SAMD_MSG_CN(38, 6, true)
          SAMD_MSG_CN(39, 7, true) SAMD_MSG_CN(40, 8, true) SAMD_MSG_CN(41, 9, true) SAMD_MSG_CN(42, 10, true)
          default: break;
        }
#undef SAMD_MSG_CN
#undef SAMD_MSG_CN_
      }
      ms_phase_barrier(last || !lds_bar);
      SAMD_ITRACE(2000)
      // ---------------- VN phase: the channel LLRs of an item are fetched one item ahead (across group boundaries: the
      // items of a wave are consecutive in i_vn), its list entry two ahead - the entry then sits in scalar registers when
      // the LLR request needs its address, instead of a scalar-cache round trip at the top of every item
      {
        int2 cur = vfirst, nxt = vsecond;
        float l0 = lf0, l1 = lf1;
        for (int g = gv0; g < gv1; ++g) {
          const int2 G = g_vn[g];
          const int key = __builtin_amdgcn_readfirstlane(G.x);
          const int gy = __builtin_amdgcn_readfirstlane(G.y);
          const int tb = gy & 0xFFFF, te = (unsigned)gy >> 16;
#define SAMD_MSG_VN(KEY, D, NCHV)                                                                                \
  case KEY: {                                                                                                     \
    for (int t = tb; t < te; ++t) {                                                                               \
      const unsigned ix = (unsigned)__builtin_amdgcn_readfirstlane(cur.x);                                        \
      const int iy = __builtin_amdgcn_readfirstlane(cur.y);                                                       \
      int2 nxt2 = make_int2(0, 0);                                                                                \
      float n0 = 0.f, n1 = 0.f;                                                                                   \
      if (t + 2 < vend_i) nxt2 = i_vn[t + 2];                                                                     \
      if (t + 1 < vend_i) {                                                                                       \
        const int e0 = __builtin_amdgcn_readfirstlane(nxt.x);                                                     \
        n0 = llr[(e0 & 0x7FFFFF) + lane];                                                                         \
        if ((e0 >> 23) & 1) n1 = llr[(e0 & 0x7FFFFF) + lane + 64];                                                \
      }                                                                                                           \
      const int pr = (int)(ix >> 24);                                                                             \
      if (pr != cur_prio) { onchip_setprio(pr); cur_prio = pr; }                                                  \
      const unsigned zz4 = ((unsigned)iy >> 20) * 256u + lane4;                                                    \
      ms_vn_col<D, NCHV, POW2, false, (ZM == 2 && NCHV == 2)>(col_ent + (iy & 0xFFFFF), zz4, zwv,                 \
                                                              llr + (ix & 0x7FFFFFu) + lane, l0, l1, llr_max, last); \
      SAMD_ITRACE(2000 + KEY)                                                                                     \
      cur = nxt; nxt = nxt2; l0 = n0; l1 = n1;                                                                    \
    }                                                                                                             \
  } break;
          switch (key) {
            SAMD_MSG_VN(1, 1, 1) SAMD_MSG_VN(2, 2, 1) SAMD_MSG_VN(3, 3, 1) SAMD_MSG_VN(4, 4, 1) SAMD_MSG_VN(5, 5, 1)
            SAMD_MSG_VN(6, 6, 1) SAMD_MSG_VN(7, 7, 1) SAMD_MSG_VN(8, 8, 1) SAMD_MSG_VN(9, 9, 1) SAMD_MSG_VN(10, 10, 1)
            SAMD_MSG_VN(11, 11, 1) SAMD_MSG_VN(12, 12, 1) SAMD_MSG_VN(13, 13, 1) SAMD_MSG_VN(14, 14, 1)
            SAMD_MSG_VN(15, 15, 1) SAMD_MSG_VN(16, 16, 1) SAMD_MSG_VN(17, 17, 1) SAMD_MSG_VN(18, 18, 1)
            SAMD_MSG_VN(19, 19, 1) SAMD_MSG_VN(20, 20, 1) SAMD_MSG_VN(21, 21, 1) SAMD_MSG_VN(22, 22, 1)
            SAMD_MSG_VN(23, 23, 1) SAMD_MSG_VN(24, 24, 1) SAMD_MSG_VN(25, 25, 1) SAMD_MSG_VN(26, 26, 1)
            SAMD_MSG_VN(27, 27, 1) SAMD_MSG_VN(28, 28, 1) SAMD_MSG_VN(29, 29, 1) SAMD_MSG_VN(30, 30, 1)
            SAMD_MSG_VN(33, 1, 2) SAMD_MSG_VN(34, 2, 2) SAMD_MSG_VN(35, 3, 2) SAMD_MSG_VN(36, 4, 2) SAMD_MSG_VN(37, 5, 2)
            SAMD_MSG_VN(38, 6, 2) SAMD_MSG_VN(39, 7, 2) SAMD_MSG_VN(40, 8, 2) SAMD_MSG_VN(41, 9, 2)
            SAMD_MSG_VN(42, 10, 2) SAMD_MSG_VN(43, 11, 2) SAMD_MSG_VN(44, 12, 2)
            default: break;
          }
#undef SAMD_MSG_VN
        }
      }
      ms_phase_barrier(last || !lds_bar);
      SAMD_ITRACE(3000)
    }
    // llr[] now holds the marginals
    store_codeword(p, out, (size_t)b, [&](int v) { return llr[v]; }, llr_max, hard_out,
                   return_infobits, tid, NT);
    __syncthreads();
  }
}

#if defined(SAMD_MS_TRACE) && defined(SAMD_MS_MAIN_TU)
}  // namespace samd
extern "C" int samd_debug_set_ms_trace(unsigned long long* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(samd::g_ms_trace), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
namespace samd {
#endif

template <int MODE>
static int launch_onchip_ms_mode(const samd_ldpc5g* h, const float* llr, float* out, int batch, int num_iter, int cn_mode,
                     float llr_max, float offset, int hard_out, int return_infobits, void* workspace,
                     size_t workspace_bytes, hipStream_t st) {
  if (!h->bp.ok || !h->ms.col_ent.get() || !h->ms.cn_list.get() || !h->ms.vn_list.get() || !h->ms.vn_ptr.get()) {
    set_error("messages of this code do not fit in LDS");
    return SAMD_ERR_UNSUPPORTED;
  }
  float* llr_ws = nullptr;
  if (h->bp.llr_global) {
    const int rc = decode_workspace(workspace, workspace_bytes, onchip_bp_workspace_bytes(h, batch), &llr_ws);
    if (rc != SAMD_OK) return rc;
  }
  const bool pow2 = (h->z & (h->z - 1)) == 0;
  if (h->ms.g_ok && h->bp.waves == 16) {
    // grouped dispatch: the same items, sorted by body type per wave (see ldpc5g_decode_msg_kernel)
    typedef void (*gkern_t)(const float*, float*, float*, RateMatch, int, int, int, int, float, float, int, int, int,
                            const int32_t*, const int32_t*, const int2*, const int32_t*, const int2*, const int2*,
                            const int2*, const int2*, int, int);
    static const gkern_t gk[6] = {ldpc5g_decode_msg_kernel<0, false, MODE>, ldpc5g_decode_msg_kernel<1, false, MODE>,
                                  ldpc5g_decode_msg_kernel<2, false, MODE>, ldpc5g_decode_msg_kernel<0, true, MODE>,
                                  ldpc5g_decode_msg_kernel<1, true, MODE>,  ldpc5g_decode_msg_kernel<2, true, MODE>};
    const int zm = h->z == 128 ? 2 : (pow2 ? 1 : 0);
    const gkern_t fn = gk[(h->bp.llr_global ? 3 : 0) + zm];
    SAMD_SET_MAX_LDS(fn, 160 * 1024);
    const RateMatch rm_g = make_rate_match(h);
    const float off_g = (cn_mode == SAMD_CN_OFFSET_MINSUM) ? offset : 0.f;
    // boxplus-phi: 512 bytes behind the messages for the table of the defined logarithm when they fit (else global memory)
    const int phi_lds_g = MODE == SAMD_CN_BOXPLUS_PHI ? 1 : 0;
    if (phi_lds_g && onchip_bp_lds_bytes(h) + 512 > 160 * 1024) {
      set_error("no room for the boxplus-phi table beside the messages");
      return SAMD_ERR_UNSUPPORTED;                             // the caller runs the first boxplus kernel (table from global memory)
    }
    hipLaunchKernelGGL(fn, dim3(onchip_bp_grid(h, batch)), dim3(1024), onchip_bp_lds_bytes(h) + (phi_lds_g ? 512 : 0), st,
                       llr, out, llr_ws, rm_g, h->n_cn, used_cols(h), batch, num_iter, llr_max, off_g, hard_out, return_infobits,
                       h->bp.edges * h->z, h->ms.col_ent.get(), h->ms.vn_ptr.get(),
                       reinterpret_cast<const int2*>(h->ms.vn_list.get()), h->ms.g_ptr.get(),
                       reinterpret_cast<const int2*>(h->ms.g_cn.get()), reinterpret_cast<const int2*>(h->ms.g_vn.get()),
                       reinterpret_cast<const int2*>(h->ms.i_cn.get()), reinterpret_cast<const int2*>(h->ms.i_vn.get()),
                       /* lds_bar: always the full barrier - the argument stays because the kernels' register allocation
                          moves without it */ 0, phi_lds_g);
    return launch_status();
  }
  typedef void (*kern_t)(const float*, float*, float*, RateMatch, int, int, int, int, float, float, int, int, int,
                         const int32_t*, const int32_t*, const int2*, const int32_t*, const int2*, const int2*, int, const int2*, int);
#define SAMD_MS_K(NWV, G, P) ldpc5g_decode_ms_kernel<false, NWV, G, MODE, P>, ldpc5g_decode_ms_kernel<true, NWV, G, MODE, P>
#define SAMD_MS_TAB(P) {SAMD_MS_K(16, false, P), SAMD_MS_K(8, false, P), SAMD_MS_K(4, false, P), \
                        SAMD_MS_K(2, false, P),  SAMD_MS_K(1, false, P), SAMD_MS_K(16, true, P)}
  static const kern_t kerns2[2][12] = {SAMD_MS_TAB(false), SAMD_MS_TAB(true)};
#undef SAMD_MS_TAB
#undef SAMD_MS_K
  const kern_t* kerns = kerns2[h->ms.tail_sh < 6 ? 1 : 0];     // packed-tail items in the lists
  const int nw = h->bp.waves;
  const int wi = h->bp.llr_global ? 5 : (nw == 16 ? 0 : nw == 8 ? 1 : nw == 4 ? 2 : nw == 2 ? 3 : 4);
  const int ki = 2 * wi + (pow2 ? 1 : 0);
  SAMD_SET_MAX_LDS(kerns[ki], 160 * 1024);
  const RateMatch rm = make_rate_match(h);
  const float off = (cn_mode == SAMD_CN_OFFSET_MINSUM) ? offset : 0.f;
  // (several workgroups may share a CU here: the table's 512 bytes count per workgroup)
  const size_t per_cu_wg = onchip_wgs_per_cu(nw, onchip_bp_lds_bytes(h));
  const int phi_lds = MODE == SAMD_CN_BOXPLUS_PHI ? 1 : 0;
  if (phi_lds && (onchip_bp_lds_bytes(h) + 512) * per_cu_wg > 160 * 1024) {
    set_error("no room for the boxplus-phi table beside the messages");
    return SAMD_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(kerns[ki], dim3(onchip_bp_grid(h, batch)), dim3(nw * 64), onchip_bp_lds_bytes(h) + (phi_lds ? 512 : 0),
                     st, llr, out, llr_ws, rm, h->n_cn, used_cols(h), batch, num_iter, llr_max, off, hard_out, return_infobits,
                     h->bp.edges * h->z, h->ms.col_ent.get(), h->ms.cn_ptr.get(),
                     reinterpret_cast<const int2*>(h->ms.cn_list.get()),
                     h->ms.vn_ptr.get(), reinterpret_cast<const int2*>(h->ms.vn_list.get()),
                     reinterpret_cast<const int2*>(h->ms.tail_tab.get()), h->ms.tail_sh,
                     reinterpret_cast<const int2*>(h->ms.vtail_tab.get()), phi_lds);
  return launch_status();
}

}  // namespace samd
