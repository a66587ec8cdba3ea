// On-chip LAYERED decoder with RUNNING TOTALS for 5G-NR LDPC codes, min-sum family (LDPC5GDecoder.layered_totals = "running").
//
// Replaces the same reference path as ldpc5g_onchip_ly.hip - LDPC5GDecoder(cn_schedule="layered").call, reference
// src/sionna/phy/fec/ldpc/decoding.py:1383-1390 (one sub-iteration per base row), _bp_iter with an array schedule :463-520,
// vn_update_sum :681-732, cn_update_offset_minsum / cn_update_minsum :755-953, rate recovery and output mapping :1427-1536 -
// in the textbook form of a layered decoder: one running total per variable node, every edge touched once per layer,
//     t = xtot[v] - c_old[e];   v2c = clip(t);   c_new = cn_update(v2c of the row);   xtot[v] = t + c_new[e].
// In exact arithmetic that is the reference's function; in float32 it rounds differently from "re-sum every variable node
// after every layer", so it is NOT the bits of ldpc5g_onchip_ly.hip / the oracle.  Its bits are defined by
// tests/ldpc_layered_rt_f32.py, which this kernel matches bit for bit; how close that specification stays to the reference
// is a CPU question about that file (tests/test_layered_rt_host.py).
//
// State of one codeword = one SLOT of the workgroup's LDS, nothing anywhere else:
//   blk[c][z]    one float per variable node, column-major like the lifted graph: the running total of a core column; the
//                channel LLR of a degree-1 column of the extension part (its total is llr + c, so t = llr exactly: never
//                written inside the loop; the last iteration leaves llr + c_new there for the output phase)
//   rec[r][3][z] per check node 12 bytes instead of 4 per edge: the messages a min-sum check node sends take two
//                magnitudes, a2 on the edge that delivered the unique minimum and a1 on all others - (a1, a2, word) with
//                the sign bits of the sent messages in bits 0..18 and the index of the a2 edge in bits 24..28.  Zeroed at
//                the start: every message +0.
// Schedule: one step per group of consecutive base rows that share no column (layered_row_groups, ldpc5g.h), one workgroup
// barrier per step, no re-sum steps and no prefixes.  Inside a step every variable node belongs to one check node, so
// the items (row, 64-lane chunk) of a step run on any wave in any order, without atomics.  A workgroup holds `slots`
// codewords that walk the same step list in lockstep and share its barriers: the host flattens (slot, row, chunk) into
// one item list per step, wave w takes items w, w + NW, ...  The batch tail is masked per item (slot >= live: no body);
// every wave still reaches every barrier.
#include "ldpc5g_onchip_ms.inc"

namespace samd {

enum { LYRT_IDX_SHIFT = 24 };

// the message a check node sent on its edge i, from its record
__device__ __forceinline__ float lyrt_sent(float a1, float a2, unsigned word, int i) {
  const float mag = ((word >> LYRT_IDX_SHIFT) == (unsigned)i) ? a2 : a1;
  return __uint_as_float(__float_as_uint(mag) | ((word << (31 - i)) & 0x80000000u));
}

// check nodes (row r, lifted copies 64 chunk + lane) of one codeword: D edges, the last one to a degree-1 column when F.
// ra: byte address of the record (a1; a2 and the word follow at + 4 Z, + 8 Z); ent: (byte offset of the column's block in the
// slot, 4 shift) per edge; sbase: the slot's byte offset; zq4 = 4 (64 chunk + lane)
template <int D, bool F, bool POW2>
__device__ __forceinline__ void lyrt_cn_row(unsigned ra, unsigned z4, const int32_t* __restrict__ ent, unsigned sbase, unsigned zq4,
                                            unsigned zwv, float llr_max, float offset, bool last) {
  constexpr int NF = F ? D - 1 : D;
  const float a1o = lds_ld(ra), a2o = lds_ld(ra + z4);
  const unsigned wo = __float_as_uint(lds_ld(ra + 2u * z4));
  unsigned ax[D];
  float t[D], v[1][D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const unsigned s = zq4 + (unsigned)ent[2 * i + 1];
    const unsigned base = sbase + (unsigned)ent[2 * i];
    ax[i] = POW2 ? ((s & zwv) | base) : (min(s, s - zwv) + base);
    t[i] = lds_ld(ax[i]);
  }
#pragma unroll
  for (int i = 0; i < NF; ++i) t[i] = t[i] - lyrt_sent(a1o, a2o, wo, i);     // unclipped (a degree-1 node: t = llr as loaded)
#pragma unroll
  for (int i = 0; i < D; ++i) v[0][i] = ms_med3(t[i], -llr_max, llr_max);
  ms_minsum_inplace<D, 1>(v, llr_max, offset);                             // v <- the messages sent now
  // their record: smaller / larger magnitude, first edge with the larger one, sign bits
  float a1 = fabsf(v[0][0]), a2 = a1;
  unsigned idx = 0u, sg = __float_as_uint(v[0][0]) >> 31;
#pragma unroll
  for (int i = 1; i < D; ++i) {
    const float m = fabsf(v[0][i]);
    idx = (m > a2) ? (unsigned)i : idx;
    a2 = fmaxf(a2, m);
    a1 = fminf(a1, m);
    sg |= (__float_as_uint(v[0][i]) >> 31) << i;
  }
  lds_st(ra, a1);
  lds_st(ra + z4, a2);
  lds_st(ra + 2u * z4, __uint_as_float(sg | (idx << LYRT_IDX_SHIFT)));
#pragma unroll
  for (int i = 0; i < NF; ++i) lds_st(ax[i], t[i] + v[0][i]);
  if (F && last) lds_st(ax[D - 1], t[D - 1] + v[0][D - 1]);                  // marginal of the degree-1 node = llr + c
}

// items: x = row degree | fused << 5 | chunk << 8, y = byte offset of the row's record block in the slot, z = byte offset of
// the row's entries in ent_tab, w = slot.  step_ptr[s] .. step_ptr[s + 1]: the items of step s, all slots.
template <bool POW2>
__global__ __launch_bounds__(1024) void ldpc5g_decode_lyrt_kernel(
    const float* __restrict__ llr_in, float* __restrict__ out, RateMatch p, int nbu, int ncu, int batch, int num_iter,
    float llr_max, float offset, int hard_out, int return_infobits, int slots, int slot_bytes, int nsteps,
    const int32_t* __restrict__ step_ptr, const int4* __restrict__ items, const int32_t* __restrict__ ent_tab) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((unsigned)(size_t)(lds_f32*)smem != 0u) __builtin_trap();      // LDS addressed by plain byte offsets (lds_ld)
  const int NT = (int)blockDim.x, NW = NT >> 6;
  const unsigned z = (unsigned)p.z, z4 = 4u * z;
  const unsigned zw = POW2 ? z4 - 1u : z4;
  unsigned zwv;
  asm volatile("v_mov_b32 %0, %1" : "=v"(zwv) : "s"(zw));
  const int nx = nbu * (int)z, nrec = 3 * ncu * (int)z, slot_floats = slot_bytes >> 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned lane4 = 4u * (unsigned)lane;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (long b0 = (long)blockIdx.x * slots; b0 < batch; b0 += (long)gridDim.x * slots) {
    const int live = (long)batch - b0 < (long)slots ? (int)((long)batch - b0) : slots;
    // decoding.py:552-565 (clip, logits -> LLR; + 0.f: no -0 anywhere); every sent message starts at +0 (:575-578)
    for (int s = 0; s < live; ++s) {
      float* blk = smem + (size_t)s * slot_floats;
      const float* row = llr_in + (size_t)(b0 + s) * p.n;
      for (int v = tid; v < nx; v += NT) blk[v] = channel_llr<true>(p, row, v, p.n_vn, llr_max);
      for (int i = tid; i < nrec; i += NT) blk[nx + i] = 0.f;
    }
    __syncthreads();
    for (int it = 0; it < num_iter; ++it) {
      const bool last = it == num_iter - 1;
      int j1 = step_ptr[0];
      for (int st = 0; st < nsteps; ++st) {
        const int j0 = j1;
        j1 = step_ptr[st + 1];
        for (int j = j0 + w; j < j1; j += NW) {
          const int4 I = items[j];
          const int ix = __builtin_amdgcn_readfirstlane(I.x), slot = __builtin_amdgcn_readfirstlane(I.w);
          const unsigned zq4 = ((unsigned)(ix >> 8) & 0xFFu) * 256u + lane4;    // 4 (64 chunk + lane)
          // a slot past the batch's end has no body; lanes past the lifting size (partly filled last chunk) neither
          if (slot < live && (zq4 >> 2) < z) {
            const unsigned sbase = (unsigned)slot * (unsigned)slot_bytes;
            const unsigned ra = sbase + (unsigned)__builtin_amdgcn_readfirstlane(I.y) + zq4;
            const int32_t* ent = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(ent_tab) + __builtin_amdgcn_readfirstlane(I.z));
#define SAMD_LYRT_CN(KEY, D, F) \
  case KEY: lyrt_cn_row<D, F, POW2>(ra, z4, ent, sbase, zq4, zwv, llr_max, offset, last); break;
            switch (ix & 63) {
              SAMD_LYRT_CN(3, 3, false) SAMD_LYRT_CN(4, 4, false) SAMD_LYRT_CN(5, 5, false) SAMD_LYRT_CN(6, 6, false)
              SAMD_LYRT_CN(7, 7, false) SAMD_LYRT_CN(8, 8, false) SAMD_LYRT_CN(9, 9, false) SAMD_LYRT_CN(10, 10, false)
              SAMD_LYRT_CN(19, 19, false)
              SAMD_LYRT_CN(35, 3, true) SAMD_LYRT_CN(36, 4, true) SAMD_LYRT_CN(37, 5, true) SAMD_LYRT_CN(38, 6, true)
              SAMD_LYRT_CN(39, 7, true) SAMD_LYRT_CN(40, 8, true) SAMD_LYRT_CN(41, 9, true) SAMD_LYRT_CN(42, 10, true)
              default: break;
            }
#undef SAMD_LYRT_CN
          }
        }
        __syncthreads();
      }
    }
    // ---------------- output (decoding.py:620-626, 1486-1531): blk[] holds the marginals
    for (int s = 0; s < live; ++s) {
      const float* blk = smem + (size_t)s * slot_floats;
      store_codeword(p, out, (size_t)(b0 + s), [&](int v) { return blk[v]; }, llr_max,
                     hard_out, return_infobits, tid, NT);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ host tables
int build_onchip_lyrt_tables(samd_ldpc5g* h, const BaseRows& by_row) {
  h->lyrt.ok = 0;
  const int z = h->z;
  const int ncu = (h->n_cn + z - 1) / z, nbu = (h->n_vn + z - 1) / z;
  // whole base rows and columns only (a partially pruned row stays with the other engines)
  if (h->n_cn % z != 0 || h->n_vn % z != 0 || z > 64 * 255 || ncu < 1) return SAMD_OK;
  std::vector<int> col_deg(h->nb, 0);
  for (int r = 0; r < ncu; ++r)
    for (auto& e : by_row[r]) {
      if (e.first >= nbu) return SAMD_OK;
      ++col_deg[e.first];
    }
  // every row degree needs a compiled body (lyrt_cn_row: 3..10 and 19 plain, 3..10 with a degree-1 last edge), and a
  // degree-1 column may only be its row's last edge
  std::vector<char> col_private(h->nb, 0);
  std::vector<int> key(ncu, 0);
  for (int r = 0; r < ncu; ++r) {
    const int d = (int)by_row[r].size();
    if (!((d >= 3 && d <= 10) || d == 19)) return SAMD_OK;
    for (int i = 0; i + 1 < d; ++i)
      if (col_deg[by_row[r][i].first] == 1) return SAMD_OK;
    const int f = col_deg[by_row[r][d - 1].first] == 1 ? 1 : 0;
    if (f && d == 19) return SAMD_OK;
    if (f) col_private[by_row[r][d - 1].first] = 1;
    key[r] = d | (f << 5);
  }
  const std::vector<std::vector<int>> groups = layered_row_groups(by_row, ncu, h->nb, col_private);
  const int chunks = (z + 63) / 64;                          // (the last one partly filled when Z is not a multiple of 64)
  // one slot: a block per column, three per row - a multiple of 4 Z bytes, which keeps every block aligned to 4 Z (the
  // power-of-two lifting sizes form an address as (position mod 4 Z) | block offset)
  const size_t slot_bytes = ((size_t)nbu + 3 * (size_t)ncu) * z * 4;
  const int per_cu = (int)std::min<size_t>(16, (160 * 1024) / slot_bytes);
  if (per_cu < 1) return SAMD_OK;
  // Workgroup = the waves one step of one codeword can use (its largest group's items, a power of two, 2 ... 16);
  // 16 waves per CU (launch bound: 128 registers each), so 16 / waves workgroups share a CU and the codewords LDS has room
  // for are dealt to them as slots.
  int items_max = 1;
  for (auto& g : groups) items_max = std::max(items_max, (int)g.size() * chunks);
  int nw = 2;
  while (nw < items_max && nw < 16) nw *= 2;
  const int wg_per_cu = std::min(16 / nw, per_cu);
  const int slots = std::max(1, std::min(8, per_cu / wg_per_cu));
  // the rows' entries and the steps' item lists
  std::vector<int32_t> ent_tab, row_start(ncu, 0), step_ptr(1, 0), items;
  for (int r = 0; r < ncu; ++r) {
    row_start[r] = (int32_t)ent_tab.size();
    for (auto& e : by_row[r]) {
      ent_tab.push_back(e.first * z * 4);
      ent_tab.push_back(4 * e.second);
    }
  }
  ent_tab.resize(ent_tab.size() + 64, 0);
  for (auto& g : groups) {
    // slot-minor: the waves of a step start on different rows AND the slots of one row sit on neighbouring waves
    for (int r : g)
      for (int q = 0; q < chunks; ++q)
        for (int s = 0; s < slots; ++s) {
          items.push_back(key[r] | (q << 8));
          items.push_back((nbu + 3 * r) * z * 4);
          items.push_back(4 * row_start[r]);
          items.push_back(s);
        }
    step_ptr.push_back((int32_t)(items.size() / 4));
  }
  h->lyrt.slots = slots;
  h->lyrt.slot_bytes = (int)slot_bytes;
  h->lyrt.waves = nw;
  h->lyrt.wg_per_cu = wg_per_cu;
  h->lyrt.steps = (int)groups.size();
  int rc = h->lyrt.step_ptr.assign(step_ptr);
  if (rc == SAMD_OK) rc = h->lyrt.items.assign(items);
  if (rc == SAMD_OK) rc = h->lyrt.ent_tab.assign(ent_tab);
  if (rc == SAMD_OK) h->lyrt.ok = 1;
  return rc;
}

int launch_onchip_lyrt(const samd_ldpc5g* h, const float* llr, float* out, int batch, int num_iter, int cn_mode, float llr_max,
                       float offset, int hard_out, int return_infobits, hipStream_t st) {
  const samd::Ldpc5gLayeredRt& t = h->lyrt;
  if (!t.ok || !(cn_mode == SAMD_CN_MINSUM || cn_mode == SAMD_CN_OFFSET_MINSUM)) {
    set_error("layered running-total engine: code or rule not covered");
    return SAMD_ERR_UNSUPPORTED;
  }
  int grid = std::min((batch + t.slots - 1) / t.slots, device_cus() * t.wg_per_cu);
  if (h->opt.onchip_grid > 0) grid = std::min(grid, h->opt.onchip_grid);
  const bool pow2 = (h->z & (h->z - 1)) == 0;
  typedef void (*kern_t)(const float*, float*, RateMatch, int, int, int, int, float, float, int, int, int, int, int,
                         const int32_t*, const int4*, const int32_t*);
  const kern_t fn = pow2 ? ldpc5g_decode_lyrt_kernel<true> : ldpc5g_decode_lyrt_kernel<false>;
  SAMD_SET_MAX_LDS(fn, 160 * 1024);
  const int nbu = used_cols(h), ncu = (h->n_cn + h->z - 1) / h->z;
  const float off = (cn_mode == SAMD_CN_OFFSET_MINSUM) ? offset : 0.f;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * t.waves), (size_t)t.slots * (size_t)t.slot_bytes, st, llr, out,
                     make_rate_match(h), nbu, ncu, batch, num_iter, llr_max, off, hard_out, return_infobits, t.slots,
                     t.slot_bytes, t.steps, t.step_ptr.get(), reinterpret_cast<const int4*>(t.items.get()), t.ent_tab.get());
  return launch_status();
}

}  // namespace samd
