// On-chip flooding decoder for 5G-NR LDPC codes with the boxplus-phi (reference default) and
// boxplus (tanh) check-node rules: one float per edge, resident in LDS for all iterations.
//
// Replaces LDPC5GDecoder.call = rate recovery + LDPCBPDecoder._bp_iter x num_iter + cn_update_phi /
// cn_update_tanh + vn_update_sum + output mapping (reference src/sionna/phy/fec/ldpc/decoding.py:
// 1427-1536, 416-524, 681-732, 955-1166) for codes whose E 4-byte messages fit in 160 KB - C2
// (n=8448, rate 1/3, Z=128: 316 Z edges = 158 KB, channel LLRs in an L2 workspace row) and everything
// smaller.  The HBM-resident engine (ldpc_bp_generic.hip) moves 16 E + 4 N bytes per codeword and
// iteration through HBM and sits at ~41 % of the HBM roofline; here the messages never leave the CU.
//
// Layout: edge block e = (row r, position i in the row) holds msg[e][zr], zr = lifted copy of the
// CHECK node - the CN phase reads/writes lane-contiguous rows, the VN phase of column c reads the block
// rotated by the edge's shift.  A message slot holds v2c after the VN phase and c2v after the CN phase
// (in place, like the HBM engine).  Arithmetic and summation order are those of ldpc_bp_generic.hip
// (bp_math.h: ascending VN inside a CN, ascending CN inside a VN, channel LLR last), so the two engines
// return the same bits.
//
// Work split: (row, 64-lane chunk) and (column, chunk) items are assigned to the waves on the host
// (longest-processing-time first); every item is an instantiation for the row's exact degree / the
// column's degree class, all table entries are wave-uniform scalars.
#include "ldpc5g_io.h"
#include "ldpc5g_jit.h"

#include <cmath>
#include "bp_math.h"

namespace samd {

template <bool POW2>
__device__ __forceinline__ unsigned bp_wrap_sub(unsigned zz4, unsigned s4, unsigned zw) {
  const unsigned t = zz4 - s4;
  return POW2 ? (t & zw) : min(t, t + zw);
}

// one check node per lane: row of exact degree D; its messages are D lane-contiguous blocks
template <int MODE, int D>
__device__ __forceinline__ void bp_cn_row(char* __restrict__ msg_b, unsigned a0, unsigned z4, float llr_max) {
  float v[D];
#pragma unroll
  for (int i = 0; i < D; ++i) v[i] = *reinterpret_cast<const float*>(msg_b + a0 + (unsigned)i * z4);
  cn_update_col<MODE, D>(v, D, llr_max, 0.f);
#pragma unroll
  for (int i = 0; i < D; ++i) *reinterpret_cast<float*>(msg_b + a0 + (unsigned)i * z4) = v[i];
}

// one variable node per lane: column of degree d <= DMAX.  ent[i] = block byte offset | (4 shift) << 18.
// INIT: v2c of iteration 0 = channel LLR (decoding.py:571).  LAST: the marginal replaces the channel LLR.
template <int DMAX, bool POW2, bool INIT>
__device__ __forceinline__ void bp_vn_col(const int32_t* __restrict__ ent, int d, unsigned zz4, unsigned zw,
                                          char* __restrict__ msg_b, float* __restrict__ llr_v, float llr_max,
                                          bool last) {
  unsigned a[DMAX];
  float c[DMAX];
  const float l = *llr_v;
  float x = 0.f;
#pragma unroll
  for (int i = 0; i < DMAX; ++i)
    if (i < d) {
      const unsigned e = (unsigned)ent[i];
      a[i] = (e & 0x3FFFFu) + bp_wrap_sub<POW2>(zz4, e >> 18, zw);
      if (INIT) {
        *reinterpret_cast<float*>(msg_b + a[i]) = l;
      } else {
        c[i] = *reinterpret_cast<const float*>(msg_b + a[i]);
        x += c[i];
      }
    }
  if (INIT) return;
  x += l;
#pragma unroll
  for (int i = 0; i < DMAX; ++i)
    if (i < d) *reinterpret_cast<float*>(msg_b + a[i]) = clampf(-1.f * c[i] + x, -llr_max, llr_max);
  if (last) *llr_v = x;
}

template <bool POW2, bool INIT>
__device__ __forceinline__ void bp_vn_item(const int32_t* __restrict__ ent, int d, unsigned zz4, unsigned zw,
                                           char* __restrict__ msg_b, float* __restrict__ llr_v, float llr_max,
                                           bool last) {
  if (d <= 1) bp_vn_col<1, POW2, INIT>(ent, d, zz4, zw, msg_b, llr_v, llr_max, last);
  else if (d <= 3) bp_vn_col<3, POW2, INIT>(ent, d, zz4, zw, msg_b, llr_v, llr_max, last);
  else if (d <= 6) bp_vn_col<6, POW2, INIT>(ent, d, zz4, zw, msg_b, llr_v, llr_max, last);
  else if (d <= 10) bp_vn_col<10, POW2, INIT>(ent, d, zz4, zw, msg_b, llr_v, llr_max, last);
  else if (d <= 16) bp_vn_col<16, POW2, INIT>(ent, d, zz4, zw, msg_b, llr_v, llr_max, last);
  else bp_vn_col<kColStride, POW2, INIT>(ent, d, zz4, zw, msg_b, llr_v, llr_max, last);
}

// NW waves per workgroup, one codeword per workgroup at a time.  LLRG: channel LLRs (and, after the last
// iteration, the marginals) in a workspace row (L2) instead of LDS.
template <int MODE, bool POW2, int NW, bool LLRG>
__global__ __launch_bounds__(NW * 64) void ldpc5g_decode_bp_kernel(
    const float* __restrict__ llr_in, float* __restrict__ out, float* __restrict__ llr_ws, RateMatch p, int n_cn,
    int nbu, int batch, int num_iter, float llr_max, int hard_out, int return_infobits, int msg_floats,
    const int32_t* __restrict__ row_off, const int32_t* __restrict__ col_ent,
    const int32_t* __restrict__ col_deg, const int32_t* __restrict__ cn_ptr, const int32_t* __restrict__ cn_list,
    const int32_t* __restrict__ vn_ptr, const int32_t* __restrict__ vn_list) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = NW * 64;
  const unsigned z = (unsigned)p.z, z4 = 4u * z;
  const unsigned zw = POW2 ? z4 - 1u : z4;
  const int n_vn = p.n_vn;
  const int nx = nbu * (int)z;
  float* llr = LLRG ? llr_ws + (size_t)blockIdx.x * nx : smem + msg_floats;
  char* msg_b = reinterpret_cast<char*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = cn_ptr[w], c1 = cn_ptr[w + 1];
  const int v0 = vn_ptr[w], v1 = vn_ptr[w + 1];

  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    const float* row = llr_in + (size_t)b * p.n;
    for (int v = tid; v < nx; v += NT) llr[v] = channel_llr<false>(p, row, v, n_vn, llr_max);
    __syncthreads();
    for (int t = v0; t < v1; ++t) {                                // v2c of iteration 0
      const int desc = __builtin_amdgcn_readfirstlane(vn_list[t]);  // c | chunk<<8
      const int c = desc & 0xFF;
      const unsigned zz = (unsigned)(((desc >> 8) & 0xFF) * 64 + lane);
      const int vn = c * (int)z + (int)zz;
      if (zz < z && vn < n_vn)
        bp_vn_item<POW2, true>(col_ent + c * kColStride, __builtin_amdgcn_readfirstlane(col_deg[c]), 4u * zz, zw,
                               msg_b, llr + vn, llr_max, false);
    }
    __syncthreads();

    for (int it = 0; it < num_iter; ++it) {
      for (int t = c0; t < c1; ++t) {
        const int desc = __builtin_amdgcn_readfirstlane(cn_list[t]);  // r | chunk<<8 | priority<<24
        const int r = desc & 0xFF;
        onchip_setprio(desc >> 24);                                   // longest remaining work first (ldpc5g.h)
        const unsigned zz = (unsigned)(((desc >> 8) & 0xFF) * 64 + lane);
        if (zz < z && (unsigned)r * z + zz < (unsigned)n_cn) {
          const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(row_off[r]);
          const unsigned a0 = (ro & 0x3FFFFu) + 4u * zz;
#define SAMD_BP_CN(D) case D: bp_cn_row<MODE, D>(msg_b, a0, z4, llr_max); break
          switch (ro >> 18) {
            SAMD_BP_CN(3); SAMD_BP_CN(4); SAMD_BP_CN(5); SAMD_BP_CN(6); SAMD_BP_CN(7); SAMD_BP_CN(8); SAMD_BP_CN(9);
            SAMD_BP_CN(10); SAMD_BP_CN(19);
            default: break;
          }
#undef SAMD_BP_CN
        } else if (zz < z) {
          // pruned check node of the last, partial base row (decoding.py:1330-1370 prunes by node count): its
          // edges do not exist - keep their slots at 0 so that the VN sums of the neighbouring columns skip them
          const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(row_off[r]);
          for (unsigned i = 0; i < (ro >> 18); ++i)
            *reinterpret_cast<float*>(msg_b + (ro & 0x3FFFFu) + 4u * zz + i * z4) = 0.f;
        }
      }
      __syncthreads();
      const bool last = (it == num_iter - 1);
      for (int t = v0; t < v1; ++t) {
        const int desc = __builtin_amdgcn_readfirstlane(vn_list[t]);
        const int c = desc & 0xFF;
        onchip_setprio(desc >> 24);
        const unsigned zz = (unsigned)(((desc >> 8) & 0xFF) * 64 + lane);
        const int vn = c * (int)z + (int)zz;
        if (zz < z && vn < n_vn)
          bp_vn_item<POW2, false>(col_ent + c * kColStride, __builtin_amdgcn_readfirstlane(col_deg[c]), 4u * zz, zw,
                                  msg_b, llr + vn, llr_max, last);
      }
      __syncthreads();
    }
    // llr[] now holds the marginals
    store_codeword(p, out, (size_t)b, [&](int v) { return llr[v]; }, llr_max, hard_out,
                   return_infobits, tid, NT);
    __syncthreads();
  }
}

static const int kBpCnDegrees[] = {3, 4, 5, 6, 7, 8, 9, 10, 19};

// ---- cost model of the explicit-message schedule, stated once.  Costs are ~ instructions; lpt_schedule balances their
// sum per wave.
// Fixed cost per CN / VN item: measured at C2 in round 2, a fixed cost of ~20 edges per item balances best.
constexpr int kMsCnOvh = 400, kMsVnOvh = 200;
// Cost per edge of a CN pair item (a single-chunk item: half).  Round 3, item trace of the grouped kernel
// (tools/ms_itrace.py, profiles/r03b/ms_itrace_r03d.txt): a CN pair item takes 127 d + 1790 cycles, a VN pair item
// 115 d + 2240, a single-chunk VN item 111 d + 1040 - one chunk has one dependency chain, so its edges cost what a pair's
// edge PAIRS cost.  18: the model of round 2; 36 for the codes of the grouped kernel: +1.7 % at C2
// (profiles/r03b/ms_cost_r03f.txt) - the other lifting sizes lose 2-3 % with it (profiles/r03b/ldpc_sweep_r03_s36.json
// vs ..._s18.json)
constexpr int kMsCnSlope = 18, kMsCnSlopeGrouped = 36;
// Granularity: C2 has 29 variable-node items for 16 waves - the four single-chunk items of the degree-30 / 28 columns
// are a wave's whole phase and leave it under-loaded, the other waves carry two pair items.  A pair item of the busiest
// wave is cut into its two single-chunk items (a little more work in total: one dependency chain each) as long as
// that shortens the longest wave under the LPT rule, at most kMsVnRefineTries times: +0.5 % at C2,
// profiles/r03b/ms_refine_r03z.txt.  A half costs half the pair + kMsVnRefineCost (item trace: V12 pair 3.6 k cycles, a
// single-chunk item of that degree ~2.4 k).
// Lifting sizes of two chunks only (Z = 128: +1.3 % at C2, +1.1 % at k=2816 n=5632; codes of three or four chunks have
// enough items per wave and lose 5 % - ms_refine_codes_r03z.txt).
constexpr int kMsVnRefineTries = 8, kMsVnRefineCost = 70;
// The same for the check-node pair items (the grouped kernel has the single-chunk bodies under key + 64): C2 +2 %,
// profiles/r03b/ms_refine_cn3_r03z.txt; rows of degree 5 / 6 with a fused column only - every further single-chunk body
// in the kernel slows the items that do not use it: all 17 bodies -2 %, four -1.4 %, two -0.3 %
constexpr int kMsCnRefineTries = 4, kMsCnRefineCost = 150;

typedef std::vector<std::pair<int, int32_t>> MsItems;            // (cost, id) as lpt_schedule takes them

// What the steps of build_onchip_bp_tables hand on, in the order they fill it
struct MsBuild {
  int z = 0, ncu = 0, nbu = 0, chunks = 0;
  // 1. message layout (both engines)
  int edges = 0;
  std::vector<int32_t> row_off, col_ent, col_deg;
  // 2. compact column tables, fused columns, packed tails
  std::vector<int32_t> col_ent2, col_start;
  std::vector<int> fused_col;                                 // per row: its fused degree-1 column or -1
  std::vector<char> col_fused;
  int groups = 1, tail_sh = 6;                                // rows per packed-tail item, log2 of its lane-group width
  std::vector<std::vector<int>> packed, vpacked;              // rows / columns of every packed-tail item
  std::vector<int> packed_key, vpacked_deg;                   // degree | fused << 5 / column degree of the item
  // 3. items and their per-wave lists (VN: per-iteration lists, then the fused columns)
  MsItems ci2, vi2;
  std::vector<int32_t> mcp, mcl, mvp, mvl;
  std::vector<int> cprio, vprio;
};

// 1. Message layout: one block of Z floats per edge, row-major; waves per workgroup from the LDS footprint.  False: the
// code is left to the other engines.
static bool bp_message_layout(samd_ldpc5g* h, const BaseRows& by_row, MsBuild& b) {
  const int z = b.z;
  b.row_off.assign(h->mb, 0); b.col_ent.assign((size_t)h->nb * kColStride, 0); b.col_deg.assign(h->nb, 0);
  int edges = 0;
  for (int r = 0; r < b.ncu; ++r) {
    const int d = (int)by_row[r].size();
    if (std::find(std::begin(kBpCnDegrees), std::end(kBpCnDegrees), d) == std::end(kBpCnDegrees)) return false;
    b.row_off[r] = (edges * z * 4) | (d << 18);             // byte offset of the first edge block | degree << 18
    for (int i = 0; i < d; ++i) {
      const int c = by_row[r][i].first, s = by_row[r][i].second;
      if (c >= b.nbu || b.col_deg[c] >= kColStride) return false;
      b.col_ent[(size_t)c * kColStride + b.col_deg[c]++] = ((edges + i) * z * 4) | ((s * 4) << 18);   // rows ascending
    }
    edges += d;
  }
  const size_t msg_bytes = (size_t)edges * z * 4;
  if (msg_bytes > 160 * 1024 || msg_bytes >= (1u << 18)) return false;   // the HBM-resident engine takes it
  b.edges = h->bp.edges = edges;
  size_t lds = msg_bytes + (size_t)b.nbu * z * 4;
  h->bp.llr_global = 0;
  if (lds > 160 * 1024) { h->bp.llr_global = 1; lds = msg_bytes; }
  h->bp.waves = 16;
  if (!h->bp.llr_global)
    for (int nwc : {8, 4, 2, 1})
      if (lds * (size_t)(kDecWaves / nwc) <= 160 * 1024) h->bp.waves = nwc;
  return true;
}

// The first boxplus kernel's own lists: one item per (row, chunk) / (column, chunk)
static void bp_item_lists(const samd_ldpc5g* h, const BaseRows& by_row, const MsBuild& b, std::vector<int32_t>& cp,
                          std::vector<int32_t>& cl, std::vector<int32_t>& vp, std::vector<int32_t>& vl) {
  // items: CN cost ~ degree (two phi evaluations per edge), VN cost ~ degree
  MsItems ci, vi;
  for (int r = 0; r < b.ncu; ++r)
    for (int q = 0; q < b.chunks; ++q)
      ci.push_back({8 * (int)by_row[r].size(), r | (q << 8)});   // also chunks of pruned check nodes only: the item keeps their slots at 0
  for (int c = 0; c < b.nbu; ++c)
    for (int q = 0; q < b.chunks; ++q)
      if (c * b.z + q * 64 < h->n_vn) vi.push_back({b.col_deg[c] + 2, c | (q << 8)});
  lpt_schedule(ci, h->bp.waves, &cp, &cl);
  lpt_schedule(vi, h->bp.waves, &vp, &vl);
  const std::vector<int> pc = item_priorities(ci, cp, cl), pv = item_priorities(vi, vp, vl);   // see ldpc5g.h
  for (size_t j = 0; j < cl.size(); ++j) cl[j] |= pc[j] << 24;
  for (size_t j = 0; j < vl.size(); ++j) vl[j] |= pv[j] << 24;
}

// 2. ldpc5g_onchip_ms.hip: compact per-column edge tables, the fused degree-1 columns and the packed tails
static void ms_fused_and_tails(const samd_ldpc5g* h, const BaseRows& by_row, MsBuild& b) {
  const int z = b.z, ncu = b.ncu, nbu = b.nbu, chunks = b.chunks;
  // compact per-column edge tables (block byte offset, 4 shift) - a few KB, they stay in the scalar cache
  b.col_start.assign(h->nb, 0);
  for (int c = 0; c < h->nb; ++c) {
    b.col_start[c] = (int32_t)b.col_ent2.size();
    for (int i = 0; i < b.col_deg[c]; ++i) {
      const int32_t e = b.col_ent[(size_t)c * kColStride + i];
      b.col_ent2.push_back(e & 0x3FFFF);
      b.col_ent2.push_back((int32_t)((uint32_t)e >> 18));
    }
  }
  b.col_ent2.resize(b.col_ent2.size() + 64, 0);                // wide scalar loads may run past the last edge
  // rows whose last edge is the only edge of its column with shift 0 (extension part of the base graph): that
  // degree-1 VN is updated inside the CN phase (ms_cn_row<D, true>) and leaves the per-iteration VN lists
  b.fused_col.assign(h->mb, -1);
  b.col_fused.assign(h->nb, 0);
  for (int r = 0; r < ncu; ++r) {
    const int d = (int)by_row[r].size();
    const int c = by_row[r][d - 1].first, sft = by_row[r][d - 1].second;
    if (b.col_deg[c] == 1 && sft == 0 && d >= 3 && d <= 10) { b.fused_col[r] = c; b.col_fused[c] = 1; }
  }
  // Z not a multiple of 64: the last chunk of a row has `tail` < 64 lifted copies.  With tail <= 32 the tails of
  // 64 / gw rows of the same degree (and fused flag) are packed into one item (lane group g works for row g) - at
  // Z = 80 the 16-lane tails of four rows share a pass instead of running at 25 % lane utilisation each
  const int tail = z - 64 * (chunks - 1);
  int gw = 64;
  while (gw / 2 >= tail && gw > 8) gw /= 2;
  const int groups = b.groups = 64 / gw;
  b.tail_sh = 0;
  while ((1 << b.tail_sh) < gw) ++b.tail_sh;
  {
    std::vector<std::vector<int>> bucket(64);
    if (groups >= 2)
      for (int r = 0; r < ncu; ++r) bucket[(int)by_row[r].size() | ((b.fused_col[r] >= 0) << 5)].push_back(r);
    for (int key = 0; key < 64; ++key)
      for (size_t i = 0; i < bucket[key].size(); i += groups) {
        b.packed.emplace_back(bucket[key].begin() + i, bucket[key].begin() + std::min(bucket[key].size(), i + groups));
        b.packed_key.push_back(key);
      }
  }
  // the same packing for the tails of the (not fused) columns, by column degree
  {
    std::vector<std::vector<int>> bucket(64);
    if (groups >= 2)
      for (int c = 0; c < nbu; ++c)
        if (!b.col_fused[c] && c * z + (chunks - 1) * 64 < h->n_vn && b.col_deg[c] >= 1 && b.col_deg[c] <= 30)
          bucket[b.col_deg[c]].push_back(c);
    for (int dg = 0; dg < 64; ++dg)
      for (size_t i = 0; i < bucket[dg].size(); i += groups) {
        b.vpacked.emplace_back(bucket[dg].begin() + i, bucket[dg].begin() + std::min(bucket[dg].size(), i + groups));
        b.vpacked_deg.push_back(dg);
      }
  }
}

// Cuts pair items of the busiest wave into their two single-chunk items while that shortens the longest wave under the LPT
// rule (see kMsVnRefineTries): a half costs half the pair + extra; may_cut(row or column) says which pairs may be cut.
template <typename MayCut>
static void ms_refine(MsItems& items, int nw, int tries, int extra, MayCut&& may_cut) {
  auto makespan = [&](const MsItems& its, std::vector<int>* owner) {
    std::vector<size_t> order(its.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return its[a].first > its[b].first; });
    std::vector<double> load(nw, 0.0);
    if (owner) owner->assign(its.size(), 0);
    for (size_t i : order) {
      int w = 0;
      for (int q = 1; q < nw; ++q)
        if (load[q] + its[i].first + 3 < load[w] + its[i].first + 3) w = q;
      load[w] += its[i].first + 3;
      if (owner) (*owner)[i] = w;
    }
    int mw = 0;
    for (int q = 1; q < nw; ++q) if (load[q] > load[mw]) mw = q;
    return std::make_pair(load[mw], mw);
  };
  for (int t = 0; t < tries; ++t) {
    std::vector<int> owner;
    const auto base = makespan(items, &owner);
    int best = -1;
    double best_m = base.first;
    for (size_t i = 0; i < items.size(); ++i) {
      if (owner[i] != base.second || !((items[i].second >> 24) & 1) || !may_cut(items[i].second & 0xFF)) continue;
      auto trial = items;
      const int c = trial[i].second & 0xFF, q = (trial[i].second >> 8) & 0xFF, half = trial[i].first / 2 + extra;
      trial[i] = {half, c | (q << 8)};
      trial.push_back({half, c | ((q + 1) << 8)});
      const double m = makespan(trial, nullptr).first;
      if (m < best_m) { best_m = m; best = (int)i; }
    }
    if (best < 0) break;
    const int c = items[best].second & 0xFF, q = (items[best].second >> 8) & 0xFF, half = items[best].first / 2 + extra;
    items[best] = {half, c | (q << 8)};
    items.push_back({half, c | ((q + 1) << 8)});
  }
}

// 3. Items and their lists.  Two consecutive fully valid chunks of a row / column (degree <= 12) form one pair item
// (bit 24), a packed tail is one item (bit 25); weights ~ instructions: 9 (CN) / 5 (VN) per edge and chunk + the item's
// dispatch (kMsCnOvh / kMsVnOvh).
static void ms_item_lists(const samd_ldpc5g* h, const BaseRows& by_row, MsBuild& b) {
  const int z = b.z, ncu = b.ncu, nbu = b.nbu, chunks = b.chunks, groups = b.groups, nw = h->bp.waves;
  const std::vector<int>& fused_col = b.fused_col;
  const bool grouped_code = z % 128 == 0 && h->n_cn % z == 0 && h->n_vn % z == 0;
  const int cn_slope = grouped_code ? kMsCnSlopeGrouped : kMsCnSlope;
  MsItems& ci2 = b.ci2;
  MsItems& vi2 = b.vi2;
  MsItems vf2;                                                // fused columns: v2c of iteration 0 only
  for (int r = 0; r < ncu; ++r)
    for (int q = 0; q < chunks; ++q) {
      const int d = (int)by_row[r].size();                    // chunks of pruned check nodes only still get an item (it zeroes their slots)
      if (groups >= 2 && q == chunks - 1) continue;           // the tail goes into a packed item
      const bool pair = (q + 2) * 64 <= z && r * z + (q + 2) * 64 <= h->n_cn &&
                        (fused_col[r] < 0 || fused_col[r] * z + (q + 2) * 64 <= h->n_vn);
      if (pair) { ci2.push_back({cn_slope * d + kMsCnOvh, r | (q << 8) | (1 << 24)}); ++q; }
      else ci2.push_back({cn_slope / 2 * d + kMsCnOvh, r | (q << 8)});
    }
  for (size_t i = 0; i < b.packed.size(); ++i)
    ci2.push_back({9 * (b.packed_key[i] & 31) + kMsCnOvh, (int32_t)i | (1 << 25)});
  for (int c = 0; c < nbu; ++c)
    for (int q = 0; q < chunks; ++q) {
      if (c * z + q * 64 >= h->n_vn) continue;
      if (groups >= 2 && q == chunks - 1 && !b.col_fused[c] && b.col_deg[c] >= 1 && b.col_deg[c] <= 30) continue;   // packed below
      const bool pair = b.col_deg[c] <= 12 && (q + 2) * 64 <= z && c * z + (q + 2) * 64 <= h->n_vn;
      auto& dst = b.col_fused[c] ? vf2 : vi2;
      if (pair) { dst.push_back({10 * b.col_deg[c] + kMsVnOvh, c | (q << 8) | (1 << 24)}); ++q; }
      else dst.push_back({5 * b.col_deg[c] + kMsVnOvh, c | (q << 8)});
    }
  for (size_t i = 0; i < b.vpacked.size(); ++i) vi2.push_back({5 * b.vpacked_deg[i] + kMsVnOvh, (int32_t)i | (1 << 25)});
  ms_refine(vi2, nw, chunks == 2 ? kMsVnRefineTries : 0, kMsVnRefineCost, [](int) { return true; });
  ms_refine(ci2, nw, chunks == 2 ? kMsCnRefineTries : 0, kMsCnRefineCost,
            [&](int r) { const int d = (int)by_row[r].size(); return fused_col[r] >= 0 && d >= 5 && d <= 6; });
  std::vector<int32_t> mfp, mfl;
  lpt_schedule(ci2, nw, &b.mcp, &b.mcl);
  lpt_schedule(vi2, nw, &b.mvp, &b.mvl);
  b.cprio = item_priorities(ci2, b.mcp, b.mcl);
  b.vprio = item_priorities(vi2, b.mvp, b.mvl);
  lpt_schedule(vf2, nw, &mfp, &mfl);
  for (int32_t o : mfp) b.mvp.push_back(o + (int32_t)b.mvl.size());
  b.mvl.insert(b.mvl.end(), mfl.begin(), mfl.end());
}

// 4. The lists as the list-walking kernel reads them: self-contained two-dword entries in the order of step 3, and the
// tables of the packed tails
static void ms_encode_lists(const BaseRows& by_row, const MsBuild& b, std::vector<int32_t>& cl2, std::vector<int32_t>& vl2,
                            std::vector<int32_t>& tail_tab, std::vector<int32_t>& vtail_tab) {
  const int chunks = b.chunks, groups = b.groups;
  const std::vector<int>& fused_col = b.fused_col;
  const std::vector<int>& cprio = b.cprio;
  const std::vector<int>& vprio = b.vprio;
  for (size_t i = 0; i < b.packed.size(); ++i)
    for (int g = 0; g < groups; ++g) {
      if (g < (int)b.packed[i].size()) {
        const int r = b.packed[i][g];
        tail_tab.push_back(b.row_off[r] & 0x3FFFF);
        tail_tab.push_back(r | ((fused_col[r] >= 0 ? fused_col[r] : 0) << 16));
      } else {
        tail_tab.push_back(0);
        tail_tab.push_back(0xFF);
      }
    }
  tail_tab.resize(tail_tab.size() + 2, 0);
  for (size_t j = 0; j < b.mcl.size(); ++j) {
    const int32_t d = b.mcl[j];
    if ((d >> 25) & 1) {                                      // packed tails: table base | key, last chunk | flag
      const int i = d & 0xFFFF;
      cl2.push_back((int32_t)(i * groups) | (b.packed_key[i] << 18));
      cl2.push_back(((chunks - 1) << 8) | (1 << 26) | (cprio[j] << 24));
      continue;
    }
    const int r = d & 0xFF, f = fused_col[r] >= 0, pr = (d >> 24) & 1;
    cl2.push_back((b.row_off[r] & 0x3FFFF) | (((int)by_row[r].size() | (f << 5) | (pr << 6)) << 18));
    cl2.push_back((d & 0xFFFF) | ((f ? fused_col[r] : 0) << 16) | (cprio[j] << 24));
  }
  for (size_t i = 0; i < b.vpacked.size(); ++i)
    for (int g = 0; g < groups; ++g) {
      const bool has = g < (int)b.vpacked[i].size();
      vtail_tab.push_back(has ? b.col_start[b.vpacked[i][g]] : 0);
      vtail_tab.push_back(has ? b.vpacked[i][g] : 0xFF);
    }
  vtail_tab.resize(vtail_tab.size() + 2, 0);
  for (size_t j = 0; j < b.mvl.size(); ++j) {
    const int32_t d = b.mvl[j];
    if ((d >> 25) & 1) {                                      // packed tails: last chunk | degree | flag, table base
      const int i = d & 0xFFFF;
      vl2.push_back(((chunks - 1) << 8) | (b.vpacked_deg[i] << 16) | (1 << 22) | ((j < vprio.size() ? vprio[j] : 0) << 24));
      vl2.push_back(i * groups);
      continue;
    }
    const int c = d & 0xFF, pr = (d >> 24) & 1;
    vl2.push_back((d & 0xFFFF) | ((b.col_deg[c] | (pr << 5)) << 16) | ((j < vprio.size() ? vprio[j] : 0) << 24));
    vl2.push_back(b.col_start[c]);
  }
  cl2.resize(cl2.size() + 2, 0); vl2.resize(vl2.size() + 2, 0);
}

// 5. Grouped dispatch (ldpc5g_decode_msg_kernel): the items of every wave sorted by body type, and the same schedule as
// data for the source generator of the specialised kernel (JitPlan, ldpc5g_jit.cpp).  Only for codes whose items are all
// full chunk pairs (Z a multiple of 128, no partially pruned base row) on 16 waves; the caller has checked that.
// Returns g_ok and, with it, the plan (else null).
static int ms_grouped_dispatch(const samd_ldpc5g* h, const BaseRows& by_row, const MsBuild& b, std::vector<int32_t>& g_ptr,
                               std::vector<int32_t>& g_cn, std::vector<int32_t>& g_vn, std::vector<int32_t>& i_cn,
                               std::vector<int32_t>& i_vn, JitPlan** plan_out) {
  const int z = b.z, ncu = b.ncu, nbu = b.nbu;
  const std::vector<int>& fused_col = b.fused_col;
  bool ok = true;
  struct It { int cost, key; int32_t x, y; int idx, pr, q; };
  JitPlan* plan = new JitPlan();
  plan->cn.resize(h->bp.waves); plan->vn.resize(h->bp.waves);
  auto cost_in = [](const MsItems& items, int32_t id) {
    for (auto& it : items)
      if (it.second == id) return it.first;
    return 0;
  };
  const int nwv = h->bp.waves;
  for (int phase = 0; phase < 2 && ok; ++phase) {
    const std::vector<int32_t>& lp = phase ? b.mvp : b.mcp;
    const std::vector<int32_t>& ll = phase ? b.mvl : b.mcl;
    std::vector<std::vector<It>> per(nwv);
    double longest = 1.0;
    for (int wv = 0; wv < nwv; ++wv) {
      double tot = 0.0;
      for (int j = lp[wv]; j < lp[wv + 1]; ++j) {
        const int32_t d = ll[j];
        if ((d >> 25) & 1) { ok = false; break; }
        const int idx = d & 0xFF, q = (d >> 8) & 0xFF, pr = (d >> 24) & 1;
        It it;
        it.idx = idx; it.pr = pr; it.q = q;
        it.cost = cost_in(phase ? b.vi2 : b.ci2, d) + 3;
        if (!phase) {
          const int f = fused_col[idx] >= 0;
          it.key = (int)by_row[idx].size() | (f << 5) | (pr ? 0 : 64);      // (64: a single chunk of the row)
          it.x = (b.row_off[idx] & 0x3FFFF) + 256 * q;
          it.y = f ? fused_col[idx] * z + q * 64 : 0;
        } else {
          it.key = b.col_deg[idx] | (pr << 5);
          it.x = (idx * z + q * 64) | (pr << 23);
          it.y = b.col_start[idx] | (q << 20);
          if (b.col_start[idx] >= (1 << 20) || idx * z + q * 64 >= (1 << 23)) ok = false;
        }
        // every key must have a compiled body in ldpc5g_decode_msg_kernel (its switches end in `default: break`, which
        // would skip the item silently): CN degrees 3..10 and 19, plain or with a fused degree-1 column (+32, up to 10),
        // single-chunk CN items only as 64+37 / 64+38; VN degrees 1..30, chunk pairs (+32) up to degree 12
        if (!phase) {
          const int dgr = it.key & 31, fz = (it.key >> 5) & 1, single = (it.key >> 6) & 1;
          const bool body = single ? (fz && (dgr == 5 || dgr == 6)) : ((dgr >= 3 && dgr <= 10) || (dgr == 19 && !fz));
          if (!body) ok = false;
        } else {
          const int dgr = it.key & 31, pair = (it.key >> 5) & 1;
          if (dgr < 1 || dgr > 30 || (pair && dgr > 12)) ok = false;
        }
        tot += it.cost;
        per[wv].push_back(it);
      }
      longest = std::max(longest, tot);
    }
    if (!ok) break;
    std::vector<int32_t>& gl = phase ? g_vn : g_cn;
    std::vector<int32_t>& il = phase ? i_vn : i_cn;
    for (int wv = 0; wv < nwv; ++wv) {
      g_ptr.push_back((int32_t)gl.size() / 2);
      // groups by type, the type with the most expensive items first; the group order is rotated by the wave's index
      // on its SIMD so that the four waves of a SIMD start a phase in different bodies (cf. lpt_schedule)
      std::stable_sort(per[wv].begin(), per[wv].end(), [](const It& a, const It& b) {
        return a.cost != b.cost ? a.cost > b.cost : a.key > b.key; });
      std::vector<std::vector<It>> grp;
      for (const It& it : per[wv]) {
        if (grp.empty() || grp.back().front().key != it.key) {
          size_t k2 = 0;
          for (; k2 < grp.size(); ++k2)
            if (grp[k2].front().key == it.key) break;
          if (k2 == grp.size()) grp.emplace_back();
          grp[k2].push_back(it);
        } else {
          grp.back().push_back(it);
        }
      }
      if (grp.size() > 1) std::rotate(grp.begin(), grp.begin() + ((wv >> 2) % grp.size()), grp.end());
      double rem = 0.0;
      for (auto& gq : grp)
        for (auto& it : gq) rem += it.cost;
      for (auto& gq : grp) {
        const size_t first = il.size() / 2;
        for (auto& it : gq) {
          const int prio = std::max(0, std::min(3, (int)std::ceil(4.0 * rem / longest) - 1));   // as item_priorities, ldpc5g.h
          rem -= it.cost;
          il.push_back(it.x | (prio << 24));
          il.push_back(it.y);
          (phase ? plan->vn : plan->cn)[wv].push_back(JitItem{it.idx, it.q, it.pr ? 2 : 1, prio});
        }
        gl.push_back(gq.front().key);
        gl.push_back((int32_t)(first | ((il.size() / 2) << 16)));
      }
    }
    g_ptr.push_back((int32_t)gl.size() / 2);
    if (il.size() / 2 >= 65536) ok = false;
  }
  const int g_ok = ok && g_ptr.size() == (size_t)(2 * (nwv + 1)) ? 1 : 0;
  if (g_ok) {
    plan->z = z; plan->edges = b.edges; plan->ncu = ncu; plan->nbu = nbu;
    plan->row_off.resize(ncu); plan->row_deg.resize(ncu); plan->fused_col.assign(fused_col.begin(), fused_col.begin() + ncu);
    for (int r = 0; r < ncu; ++r) { plan->row_off[r] = b.row_off[r] & 0x3FFFF; plan->row_deg[r] = (int)by_row[r].size(); }
    plan->col_edges.resize(nbu); plan->col_fused.assign(b.col_fused.begin(), b.col_fused.begin() + nbu);
    for (int c = 0; c < nbu; ++c)
      for (int i = 0; i < b.col_deg[c]; ++i)
        plan->col_edges[c].push_back({b.col_ent2[b.col_start[c] + 2 * i], b.col_ent2[b.col_start[c] + 2 * i + 1]});
    *plan_out = plan;
  } else {
    delete plan;
  }
  g_cn.resize(g_cn.size() + 2, 0); g_vn.resize(g_vn.size() + 2, 0);
  i_cn.resize(i_cn.size() + 4, 0); i_vn.resize(i_vn.size() + 4, 0);
  if (!g_ok) g_ptr.assign(2 * (nwv + 1), 0);
  return g_ok;
}

int build_onchip_bp_tables(samd_ldpc5g* h, const BaseRows& by_row) {
  MsBuild b;
  b.z = h->z;
  b.ncu = (h->n_cn + b.z - 1) / b.z; b.nbu = (h->n_vn + b.z - 1) / b.z;
  b.chunks = (b.z + 63) / 64;
  h->bp.ok = 0;
  if (h->mb > 255 || h->nb > 255 || b.chunks > 255) return SAMD_OK;
  if (!bp_message_layout(h, by_row, b)) return SAMD_OK;
  std::vector<int32_t> cp, cl, vp, vl;
  bp_item_lists(h, by_row, b, cp, cl, vp, vl);
  ms_fused_and_tails(h, by_row, b);
  ms_item_lists(h, by_row, b);
  std::vector<int32_t> cl2, vl2, tail_tab, vtail_tab;
  ms_encode_lists(by_row, b, cl2, vl2, tail_tab, vtail_tab);
  h->ms.tail_sh = b.tail_sh;
  std::vector<int32_t> g_ptr, g_cn, g_vn, i_cn, i_vn;
  h->ms.g_ok = 0;
  if (b.z % 128 == 0 && h->n_cn % b.z == 0 && h->n_vn % b.z == 0 && h->bp.waves == 16 && b.groups < 2)
    h->ms.g_ok = ms_grouped_dispatch(h, by_row, b, g_ptr, g_cn, g_vn, i_cn, i_vn, &h->jit_plan);
  int rc = h->bp.row_off.assign(b.row_off);
  if (rc == SAMD_OK && h->ms.g_ok) rc = h->ms.g_ptr.assign(g_ptr);
  if (rc == SAMD_OK && h->ms.g_ok) rc = h->ms.g_cn.assign(g_cn);
  if (rc == SAMD_OK && h->ms.g_ok) rc = h->ms.g_vn.assign(g_vn);
  if (rc == SAMD_OK && h->ms.g_ok) rc = h->ms.i_cn.assign(i_cn);
  if (rc == SAMD_OK && h->ms.g_ok) rc = h->ms.i_vn.assign(i_vn);
  if (rc == SAMD_OK) rc = h->bp.col_ent.assign(b.col_ent);
  if (rc == SAMD_OK) rc = h->ms.col_ent.assign(b.col_ent2);
  if (rc == SAMD_OK) rc = h->ms.cn_ptr.assign(b.mcp);
  if (rc == SAMD_OK) rc = h->ms.vn_ptr.assign(b.mvp);
  if (rc == SAMD_OK) rc = h->ms.cn_list.assign(cl2);
  if (rc == SAMD_OK) rc = h->ms.vn_list.assign(vl2);
  if (rc == SAMD_OK) rc = h->ms.tail_tab.assign(tail_tab);
  if (rc == SAMD_OK) rc = h->ms.vtail_tab.assign(vtail_tab);
  if (rc == SAMD_OK) rc = h->bp.col_deg.assign(b.col_deg);
  if (rc == SAMD_OK) rc = h->bp.cn_ptr.assign(cp);
  if (rc == SAMD_OK) rc = h->bp.cn_list.assign(cl);
  if (rc == SAMD_OK) rc = h->bp.vn_ptr.assign(vp);
  if (rc == SAMD_OK) rc = h->bp.vn_list.assign(vl);
  if (rc == SAMD_OK) h->bp.ok = 1;
  return rc;
}

size_t onchip_bp_lds_bytes(const samd_ldpc5g* h) {
  return (size_t)h->bp.edges * h->z * 4 + (h->bp.llr_global ? 0 : (size_t)used_cols(h) * h->z * 4);
}

int onchip_bp_grid(const samd_ldpc5g* h, int batch) {
  size_t grid = std::min<size_t>((size_t)batch, (size_t)device_cus() * onchip_wgs_per_cu(h->bp.waves, onchip_bp_lds_bytes(h)));
  // SAMD_ONCHIP_GRID=<n>: fewer workgroups than the chip holds (test hook: every workgroup then decodes several
  // codewords in sequence, which exercises the grid-stride loop and the reuse of its workspace row on small batches)
  if (h->opt.onchip_grid > 0) grid = std::min<size_t>(grid, (size_t)h->opt.onchip_grid);
  return (int)grid;
}

size_t onchip_bp_workspace_bytes(const samd_ldpc5g* h, int batch) {
  if (!h->bp.ok || !h->bp.llr_global || batch <= 0) return 0;
  return (size_t)onchip_bp_grid(h, batch) * used_cols(h) * h->z * sizeof(float) + 256;
}

int launch_onchip_bp(const samd_ldpc5g* h, const float* llr, float* out, int batch, int num_iter, int cn_mode,
                     float llr_max, int hard_out, int return_infobits, void* workspace, size_t workspace_bytes,
                     hipStream_t st) {
  if (!h->bp.ok) {
    set_error("messages of this code do not fit in LDS");
    return SAMD_ERR_UNSUPPORTED;
  }
  float* llr_ws = nullptr;
  if (h->bp.llr_global) {
    const int rc = decode_workspace(workspace, workspace_bytes, onchip_bp_workspace_bytes(h, batch), &llr_ws);
    if (rc != SAMD_OK) return rc;
  }
  const bool pow2 = (h->z & (h->z - 1)) == 0;
  const bool phi = (cn_mode == SAMD_CN_BOXPLUS_PHI);
  typedef void (*kern_t)(const float*, float*, float*, RateMatch, int, int, int, int, float, int, int, int,
                         const int32_t*, const int32_t*, const int32_t*, const int32_t*, const int32_t*,
                         const int32_t*, const int32_t*);
#define SAMD_BP_K(M, NWV, G) ldpc5g_decode_bp_kernel<M, false, NWV, G>, ldpc5g_decode_bp_kernel<M, true, NWV, G>
  static const kern_t kerns[24] = {
      SAMD_BP_K(SAMD_CN_BOXPLUS_PHI, 16, false), SAMD_BP_K(SAMD_CN_BOXPLUS_PHI, 8, false),
      SAMD_BP_K(SAMD_CN_BOXPLUS_PHI, 4, false),  SAMD_BP_K(SAMD_CN_BOXPLUS_PHI, 2, false),
      SAMD_BP_K(SAMD_CN_BOXPLUS_PHI, 1, false),  SAMD_BP_K(SAMD_CN_BOXPLUS_PHI, 16, true),
      SAMD_BP_K(SAMD_CN_BOXPLUS, 16, false),     SAMD_BP_K(SAMD_CN_BOXPLUS, 8, false),
      SAMD_BP_K(SAMD_CN_BOXPLUS, 4, false),      SAMD_BP_K(SAMD_CN_BOXPLUS, 2, false),
      SAMD_BP_K(SAMD_CN_BOXPLUS, 1, false),      SAMD_BP_K(SAMD_CN_BOXPLUS, 16, true)};
#undef SAMD_BP_K
  const int nw = h->bp.waves;
  const int wi = h->bp.llr_global ? 5 : (nw == 16 ? 0 : nw == 8 ? 1 : nw == 4 ? 2 : nw == 2 ? 3 : 4);
  const int ki = (phi ? 0 : 12) + 2 * wi + (pow2 ? 1 : 0);
  // set on every launch: the attribute is per device and a process may drive several
  SAMD_SET_MAX_LDS(kerns[ki], 160 * 1024);
  const RateMatch rm = make_rate_match(h);
  hipLaunchKernelGGL(kerns[ki], dim3(onchip_bp_grid(h, batch)), dim3(nw * 64), onchip_bp_lds_bytes(h), st, llr, out, llr_ws, rm,
                     h->n_cn, used_cols(h), batch, num_iter, llr_max, hard_out, return_infobits, h->bp.edges * h->z,
                     h->bp.row_off.get(), h->bp.col_ent.get(), h->bp.col_deg.get(), h->bp.cn_ptr.get(), h->bp.cn_list.get(),
                     h->bp.vn_ptr.get(), h->bp.vn_list.get());
  return launch_status();
}

}  // namespace samd
