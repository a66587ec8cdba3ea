// Ordered-statistics decoding of binary linear block codes.
//   OSDecoder.call       reference src/sionna/phy/fec/linear/decoding.py:415-478
//   OSDecoder._find_mrb  :318-402 (pivot method), _find_min_dist :272-316, _get_dist :237-270
// The specification is tests/osd_f32.py: clip to +-100, stable descending sort by |llr|, the reference's pivot
// elimination, candidates in the order of itertools.combinations with the first of equal distances winning, and the
// distance of a candidate taken relative to the order-0 word c0 as an exact integer sum: every clipped LLR is rounded
// once to a multiple of 2^-40 (rint(llr * 2^40) as int64) and flipping position i of c0 costs +-q_i.  Float32 inputs
// reproduce the reference's overflow of exp: a candidate that disagrees with the LLR's sign where |llr| > kSat32 has
// an infinite distance (key INT64_MAX).  All candidate arithmetic is integer, so the search and every reduction are
// independent of the order of additions and of how candidates are split over lanes and workgroups.
//
// Three kernels per trip of at most kTrip codewords (the host entry loops over trips, reusing the workspace):
//   osd_mrb_kernel     one wave per codeword, GF(2) rows bit-packed in LDS (64 columns per word): rank |llr|, permute the
//                      columns, pivot elimination with the rows spread over the lanes (a lane tests the pivot bit of its
//                      rows and XORs the pivot row), then the parity part of the basis, c0 and the flip costs
//   osd_search_kernel  256 lanes x nb workgroups per codeword: each lane owns a contiguous range of candidate indices,
//                      unranks its first pattern from binomials and steps combinations from there; a candidate is the
//                      XOR of the prefix rows and the last row, its cost the prefix cost + the last row's cost + one LDS
//                      table entry per CB parity bits (table[chunk][bits] = sum of the flip costs of the set bits)
//   osd_final_kernel   one wave per codeword: fixed-order reduction of the workgroups' (key, index) minima with order 0,
//                      rebuilds the winner from its index, undoes the permutation, writes [n] in the caller's dtype
#include "common.h"

namespace samd {
namespace {

constexpr int kTrip = 4096;                    // codewords per launch (grid.y of the search); larger batches loop
constexpr int kLdsBudget = 64 * 1024 - 256;      // dynamic LDS; the rest is the kernels' few static words
constexpr int kMaxParityWords = 8;             // n - k <= 512
constexpr int64_t kInf = INT64_MAX;            // key of an infinite distance; also marks a saturated information position
constexpr float kSat32 = 88.72283172607422f;   // largest float32 x with a finite float32 exp(x)
constexpr uint64_t kPerLane = 128;             // candidates a search lane aims for

struct Lay {
  int k, n, W, P, t, tw;                       // W words per full row, P per parity part, t clamped to k, tw = t + 1
  int nb;                                      // search workgroups per codeword (0: no search)
  uint64_t N, per;                             // candidates after order 0; candidates per search lane
  size_t o_cw, stride;                         // first codeword slab, bytes per slab (the binomials sit at offset 0)
  size_t o_rows, o_ic, o_pc, o_sm, o_ds, o_key0, o_res, o_perm, o_c0;   // offsets within a slab
};

__device__ __forceinline__ uint64_t choose(const uint64_t* bt, int tw, int m, int j) { return bt[(size_t)m * tw + j]; }

// combination number r (0-based, order of itertools.combinations(range(k), i)) -> idx[0 .. i-1] (stride elements apart)
__device__ __forceinline__ void unrank(const uint64_t* bt, int tw, int k, int i, uint64_t r, uint16_t* idx, int stride) {
  int x = 0;
  for (int j = 0; j < i; ++j) {
    while (x < k - 1) {
      const uint64_t c = choose(bt, tw, k - 1 - x, i - 1 - j);
      if (r < c) break;
      r -= c;
      ++x;
    }
    idx[j * stride] = (uint16_t)x;
    ++x;
  }
}

// candidate index g >= 1 -> its order i and the rank within that order
__device__ __forceinline__ int order_of(const uint64_t* bt, int tw, int k, int t, uint64_t g, uint64_t* rank) {
  uint64_t r = g - 1;
  int i = 1;
  while (i < t && r >= choose(bt, tw, k, i)) {
    r -= choose(bt, tw, k, i);
    ++i;
  }
  *rank = r;
  return i;
}

// Pascal's triangle bt[m][j] = C(m, j), m = 0..k, j = 0..t, one lane per column
__global__ __launch_bounds__(64) void osd_binom_kernel(uint64_t* __restrict__ bt, int k, int tw) {
  const int lane = threadIdx.x;
  unsigned long long v = lane == 0 ? 1 : 0;
  for (int m = 0; m <= k; ++m) {
    if (lane < tw) bt[(size_t)m * tw + lane] = v;
    const unsigned long long up = __shfl_up(v, 1);
    v += lane ? up : 0;
  }
}

__device__ __forceinline__ uint64_t wave_xor(uint64_t v) {
  for (int o = 32; o; o >>= 1) v ^= (uint64_t)__shfl_xor((unsigned long long)v, o);
  return v;
}

template <typename T>
__global__ __launch_bounds__(64) void osd_mrb_kernel(const T* __restrict__ llr, const uint64_t* __restrict__ gm, Lay L,
                                                     uint8_t* __restrict__ ws) {
  extern __shared__ uint64_t sh[];
  const int k = L.k, n = L.n, W = L.W, P = L.P, lane = threadIdx.x;
  uint64_t* rows = sh;                                   // [W][k]: word w of row r at w * k + r
  uint64_t* c0par = rows + (size_t)W * k;                // [P]
  T* l = (T*)(c0par + kMaxParityWords);                  // [n] clipped
  T* a = l + n;                                          // [n] magnitudes
  uint16_t* perm1 = (uint16_t*)(a + n);                  // [n] sorted column -> input position
  uint16_t* idx2 = perm1 + n;                            // [n] final column -> sorted column
  uint16_t* piv = idx2 + n;                              // [k]
  uint8_t* flag = (uint8_t*)(piv + k);                   // [n] pivot columns, then the hard decisions
  uint8_t* satb = flag + n;                              // [n]
  uint8_t* slab = ws + L.o_cw + (size_t)blockIdx.x * L.stride;
  const T* in = llr + (size_t)blockIdx.x * n;

  for (int j = lane; j < n; j += 64) {
    const T x = fmin(fmax(in[j], (T)-100), (T)100);
    l[j] = x;
    a[j] = fabs(x);
    idx2[j] = 0;
    flag[j] = 0;
  }
  __syncthreads();
  for (int j = lane; j < n; j += 64) {                   // stable descending rank
    const T aj = a[j];
    int r = 0;
    for (int i = 0; i < n; ++i) {
      const T ai = a[i];
      r += (ai > aj) || (ai == aj && i < j);
    }
    perm1[r] = (uint16_t)j;                              // r < n: at most n - 1 others precede j
  }
  __syncthreads();
  for (int item = lane; item < k * W; item += 64) {      // G with its columns in reliability order
    const int r = item % k, w = item / k;
    const uint64_t* g = gm + (size_t)r * W;
    uint64_t word = 0;
    for (int b = 0; b < 64; ++b) {
      const int col = w * 64 + b;
      if (col < n) {
        const int j = perm1[col];
        word |= ((g[j >> 6] >> (j & 63)) & 1ull) << b;
      }
    }
    rows[w * k + r] = word;
  }
  for (int r = 0; r < k; ++r) {                          // pivot method
    __syncthreads();
    int p = -1;
    for (int w = 0; w < W; ++w) {
      const uint64_t x = rows[w * k + r];
      if (x && p < 0) p = w * 64 + __builtin_ctzll(x);
    }
    if (p < 0) p = 0;                                    // a zero row (rank-deficient G): argmax of zeros; nothing to clear
    if (lane == 0) piv[r] = (uint16_t)p;
    const int pw = p >> 6, pb = p & 63;
    for (int r2 = lane; r2 < k; r2 += 64)
      if (r2 != r && ((rows[pw * k + r2] >> pb) & 1))
        for (int w = 0; w < W; ++w) rows[w * k + r2] ^= rows[w * k + r];
  }
  __syncthreads();
  for (int r = lane; r < k; r += 64) {
    flag[piv[r]] = 1;
    idx2[r] = piv[r];
  }
  __syncthreads();
  int base = k;
  for (int j0 = 0; j0 < n; j0 += 64) {                   // the other columns, ascending
    const int j = j0 + lane;
    const bool f = j < n && !flag[j];
    const unsigned long long m = __ballot(f);
    const int pos = base + __popcll(m & ((1ull << lane) - 1));
    if (f && pos < n) idx2[pos] = (uint16_t)j;
    base += __popcll(m);
  }
  __syncthreads();
  uint16_t* perm = (uint16_t*)(slab + L.o_perm);
  for (int i = lane; i < n; i += 64) {
    const int j = perm1[idx2[i]];
    perm[i] = (uint16_t)j;
    const T x = l[j];
    flag[i] = x > 0;                                     // hard decision of sorted position i
    satb[i] = sizeof(T) == 4 && a[j] > (T)kSat32;
  }
  uint64_t* grows = (uint64_t*)(slab + L.o_rows);        // parity part of the basis, [k][P]
  for (int item = lane; item < k * P; item += 64) {
    const int r = item % k, w = item / k;
    uint64_t word = 0;
    for (int b = 0; b < 64; ++b) {
      const int i = k + w * 64 + b;
      if (i < n) {
        const int col = idx2[i];
        word |= ((rows[(col >> 6) * k + r] >> (col & 63)) & 1ull) << b;
      }
    }
    grows[(size_t)r * P + w] = word;
  }
  __threadfence_block();
  __syncthreads();
  for (int w = 0; w < P; ++w) {                          // c0 = u G_mrb
    uint64_t acc = 0;
    for (int r = lane; r < k; r += 64)
      if (flag[r]) acc ^= grows[(size_t)r * P + w];
    acc = wave_xor(acc);
    if (lane == 0) c0par[w] = acc;
  }
  __syncthreads();
  int64_t* ic = (int64_t*)(slab + L.o_ic);
  int64_t* pc = (int64_t*)(slab + L.o_pc);
  uint8_t* c0b = slab + L.o_c0;
  for (int i = lane; i < n; i += 64) {
    const long long q = __double2ll_rn((double)l[perm1[idx2[i]]] * 0x1p40);
    const int c = i < k ? flag[i] : (int)((c0par[(i - k) >> 6] >> ((i - k) & 63)) & 1);
    const int64_t cost = c ? q : -q;
    c0b[i] = (uint8_t)c;
    if (i < k) ic[i] = satb[i] ? kInf : cost;
    else pc[i - k] = cost;
  }
  uint64_t* sm = (uint64_t*)(slab + L.o_sm);
  uint64_t* ds = (uint64_t*)(slab + L.o_ds);
  bool any = false;
  for (int w = 0; w < P; ++w) {
    const int i = k + w * 64 + lane;
    const bool s = i < n && satb[i];
    const bool d = s && (int)((c0par[w] >> lane) & 1) != flag[i];
    const unsigned long long ms = __ballot(s), md = __ballot(d);
    if (lane == 0) {
      sm[w] = ms;
      ds[w] = md;
    }
    any |= md != 0;
  }
  if (lane == 0) *(int64_t*)(slab + L.o_key0) = any ? kInf : 0;
}

__device__ __forceinline__ void take_min(int64_t& key, uint64_t& g, int64_t key2, uint64_t g2) {
  if (key2 < key || (key2 == key && g2 < g)) {
    key = key2;
    g = g2;
  }
}

template <int PMAX, int CB>
__global__ __launch_bounds__(256) void osd_search_kernel(Lay L, uint8_t* __restrict__ ws) {
  extern __shared__ uint64_t sh[];
  constexpr int kChunks = 64 / CB;                       // table chunks per parity word
  const int k = L.k, P = L.P, t = L.t, tw = L.tw, tid = threadIdx.x;
  uint64_t* rows = sh;                                   // [k][P]
  int64_t* ic = (int64_t*)(rows + (size_t)k * P);        // [k]
  int64_t* tab = ic + k;                                 // [P * kChunks][1 << CB]
  const int tabn = (P * kChunks) << CB;
  uint16_t* idx = (uint16_t*)(tab + tabn) + tid;         // [t][256]: this lane's pattern, 256 apart
  __shared__ int64_t red_key[4];
  __shared__ uint64_t red_g[4];
  const uint64_t* bt = (const uint64_t*)ws;
  uint8_t* slab = ws + L.o_cw + (size_t)blockIdx.y * L.stride;
  const uint64_t* grows = (const uint64_t*)(slab + L.o_rows);
  const int64_t* gic = (const int64_t*)(slab + L.o_ic);
  const int64_t* pc = (const int64_t*)(slab + L.o_pc);
  const int np = L.n - k;
  for (int e = tid; e < k * P; e += 256) rows[e] = grows[e];
  for (int e = tid; e < k; e += 256) ic[e] = gic[e];
  for (int e = tid; e < tabn; e += 256) {
    const int c = e >> CB, v = e & ((1 << CB) - 1);
    uint64_t s = 0;
    for (int b = 0; b < CB; ++b) {
      const int pos = c * CB + b;
      if (((v >> b) & 1) && pos < np) s += (uint64_t)pc[pos];
    }
    tab[e] = (int64_t)s;
  }
  uint64_t sm[PMAX], ds[PMAX];
#pragma unroll
  for (int w = 0; w < PMAX; ++w) {
    sm[w] = w < P ? ((const uint64_t*)(slab + L.o_sm))[w] : 0;
    ds[w] = w < P ? ((const uint64_t*)(slab + L.o_ds))[w] : 0;
  }
  __syncthreads();

  int64_t best = kInf;
  uint64_t bestg = ~0ull;
  const uint64_t lane_id = (uint64_t)blockIdx.x * 256 + tid;
  uint64_t g = 1 + lane_id * L.per;
  const uint64_t hi = g + L.per < L.N + 1 ? g + L.per : L.N + 1;
  if (g < hi) {
    uint64_t rank;
    int i = order_of(bt, tw, k, t, g, &rank);
    unrank(bt, tw, k, i, rank, idx, 256);
    for (;;) {
      uint64_t base[PMAX];
#pragma unroll
      for (int w = 0; w < PMAX; ++w) base[w] = 0;
      uint64_t bcost = 0;
      bool binf = false;
      for (int j = 0; j < i - 1; ++j) {
        const int r = idx[j * 256];
        const int64_t v = ic[r];
        binf |= v == kInf;
        bcost += (uint64_t)v;
#pragma unroll
        for (int w = 0; w < PMAX; ++w)
          if (w < P) base[w] ^= rows[r * P + w];
      }
      int last = idx[(i - 1) * 256];
      for (; last < k && g < hi; ++last, ++g) {
        const int64_t v = ic[last];
        uint64_t cost = bcost + (uint64_t)v;
        bool inf = binf | (v == kInf);
#pragma unroll
        for (int w = 0; w < PMAX; ++w)
          if (w < P) {
            const uint64_t e = base[w] ^ rows[last * P + w];
            inf |= (e & sm[w]) != ds[w];
#pragma unroll
            for (int c = 0; c < kChunks; ++c)
              cost += (uint64_t)tab[((w * kChunks + c) << CB) + (int)((e >> (c * CB)) & ((1 << CB) - 1))];
          }
        const int64_t key = inf ? kInf : (int64_t)cost;
        if (key < best) {                                // g ascends: the first of equal keys stays
          best = key;
          bestg = g;
        }
      }
      if (g >= hi) break;
      int j = i - 2;                                     // next prefix in lexicographic order
      while (j >= 0 && idx[j * 256] >= k - i + j) --j;
      if (j < 0) {
        ++i;                                             // g < hi <= N + 1, so i <= t
        for (int m = 0; m < i; ++m) idx[m * 256] = (uint16_t)m;
      } else {
        int x = idx[j * 256] + 1;
        for (int m = j; m < i; ++m) idx[m * 256] = (uint16_t)x++;
      }
    }
  }
  for (int o = 32; o; o >>= 1) {
    const int64_t k2 = (int64_t)__shfl_xor((unsigned long long)best, o);
    const uint64_t g2 = (uint64_t)__shfl_xor((unsigned long long)bestg, o);
    take_min(best, bestg, k2, g2);
  }
  if ((tid & 63) == 0) {
    red_key[tid >> 6] = best;
    red_g[tid >> 6] = bestg;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) take_min(best, bestg, red_key[w], red_g[w]);
    uint64_t* res = (uint64_t*)(slab + L.o_res) + 2 * (size_t)blockIdx.x;
    res[0] = (uint64_t)best;
    res[1] = bestg;
  }
}

template <typename T>
__global__ __launch_bounds__(64) void osd_final_kernel(Lay L, const uint8_t* __restrict__ ws, T* __restrict__ out) {
  extern __shared__ uint64_t sh[];
  uint16_t* idx = (uint16_t*)sh;                         // [t]
  __shared__ int order;
  const int k = L.k, n = L.n, P = L.P, lane = threadIdx.x;
  const uint64_t* bt = (const uint64_t*)ws;
  const uint8_t* slab = ws + L.o_cw + (size_t)blockIdx.x * L.stride;
  const uint64_t* res = (const uint64_t*)(slab + L.o_res);
  int64_t best = kInf;
  uint64_t bestg = ~0ull;
  if (lane == 0) {
    best = *(const int64_t*)(slab + L.o_key0);
    bestg = 0;
  }
  for (int b = lane; b < L.nb; b += 64) take_min(best, bestg, (int64_t)res[2 * b], res[2 * b + 1]);
  for (int o = 32; o; o >>= 1) {
    const int64_t k2 = (int64_t)__shfl_xor((unsigned long long)best, o);
    const uint64_t g2 = (uint64_t)__shfl_xor((unsigned long long)bestg, o);
    take_min(best, bestg, k2, g2);
  }
  if (lane == 0) {
    int i = 0;
    if (bestg > 0 && bestg <= L.N) {
      uint64_t rank;
      i = order_of(bt, L.tw, k, L.t, bestg, &rank);
      unrank(bt, L.tw, k, i, rank, idx, 1);
    }
    order = i;
  }
  __syncthreads();
  const int ord = order;
  const uint64_t* grows = (const uint64_t*)(slab + L.o_rows);
  const uint16_t* perm = (const uint16_t*)(slab + L.o_perm);
  const uint8_t* c0b = slab + L.o_c0;
  T* o = out + (size_t)blockIdx.x * n;
  for (int i = lane; i < n; i += 64) {
    int bit = c0b[i];
    for (int j = 0; j < ord; ++j) {
      const int r = idx[j];
      bit ^= i < k ? (r == i) : (int)((grows[(size_t)r * P + ((i - k) >> 6)] >> ((i - k) & 63)) & 1);
    }
    o[perm[i]] = (T)bit;                                 // perm[i] < n by construction
  }
}

size_t mrb_lds(const Lay& L, size_t elem) {
  return ((size_t)L.W * L.k + kMaxParityWords) * 8 + 2 * (size_t)L.n * elem + (2 * (size_t)L.n + L.k) * 2 + 2 * (size_t)L.n + 8;
}

size_t search_lds(const Lay& L, int cb) {
  return ((size_t)L.k * L.P + L.k + ((size_t)(L.P * (64 / cb)) << cb)) * 8 + (size_t)L.t * 256 * 2 + 8;
}

int plan(int k, int n, int t, Lay* out) {
  SAMD_REQUIRE(k >= 1 && n >= k && t >= 0, "OSDecoder: need 1 <= k <= n and t >= 0");
  SAMD_REQUIRE(n <= 65535, "OSDecoder: n too large");
  Lay L{};
  L.k = k;
  L.n = n;
  L.W = (n + 63) / 64;
  L.P = (n - k + 63) / 64;
  L.t = t < k ? t : k;
  L.tw = L.t + 1;
  SAMD_REQUIRE(L.P <= kMaxParityWords, "OSDecoder: n - k above 512 is not supported");
  unsigned __int128 N = 0, c = 1;                        // sum of C(k, i), i = 1..t
  const unsigned __int128 cap = (unsigned __int128)1 << 62;
  for (int i = 1; i <= L.t; ++i) {
    c = c * (unsigned)(k - i + 1) / (unsigned)i;
    N += c;
    SAMD_REQUIRE(c < cap && N < cap, "OSDecoder: the number of candidates does not fit 62 bits; use a smaller t");
  }
  L.N = (uint64_t)N;
  SAMD_REQUIRE(L.tw <= 64, "OSDecoder: the binomial table is built by one lane per order, t <= 63");
  const uint64_t want = (L.N + 256 * kPerLane - 1) / (256 * kPerLane);
  L.nb = (int)(want < 1024 ? want : 1024);
  L.per = L.nb ? (L.N + (uint64_t)L.nb * 256 - 1) / ((uint64_t)L.nb * 256) : 0;
  SAMD_REQUIRE(mrb_lds(L, 8) <= (size_t)kLdsBudget, "OSDecoder: the bit-packed generator matrix does not fit the 64 KB LDS budget");
  SAMD_REQUIRE(search_lds(L, 4) <= (size_t)kLdsBudget, "OSDecoder: basis, cost tables and patterns do not fit the 64 KB LDS budget");
  size_t o = 0;
  auto put = [&o](size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes, 8);
    return at;
  };
  L.o_rows = put((size_t)k * L.P * 8);
  L.o_ic = put((size_t)k * 8);
  L.o_pc = put((size_t)(n - k) * 8);
  L.o_sm = put((size_t)L.P * 8);
  L.o_ds = put((size_t)L.P * 8);
  L.o_key0 = put(8);
  L.o_res = put((size_t)L.nb * 16);
  L.o_perm = put((size_t)n * 2);
  L.o_c0 = put((size_t)n);
  L.stride = align_up(o, 64);
  L.o_cw = align_up((size_t)(k + 1) * L.tw * 8, 64);
  *out = L;
  return SAMD_OK;
}

template <int PMAX>
int launch_search(const Lay& L, int64_t cws, uint8_t* ws, hipStream_t s) {
  const dim3 grid((unsigned)L.nb, (unsigned)cws);
  if (search_lds(L, 8) <= (size_t)kLdsBudget)
    hipLaunchKernelGGL((osd_search_kernel<PMAX, 8>), grid, dim3(256), search_lds(L, 8), s, L, ws);
  else
    hipLaunchKernelGGL((osd_search_kernel<PMAX, 4>), grid, dim3(256), search_lds(L, 4), s, L, ws);
  return launch_status();
}

template <typename T>
int decode(const T* llr, const uint64_t* gm, int64_t batch, int k, int n, int t, T* out, void* workspace, size_t workspace_bytes,
           void* stream) {
  SAMD_REQUIRE(llr && gm && out && batch >= 0, "OSDecoder: bad argument");
  Lay L;
  const int rc = plan(k, n, t, &L);
  if (rc != SAMD_OK) return rc;
  if (batch == 0) return SAMD_OK;
  const int64_t trip = batch < kTrip ? batch : kTrip;
  SAMD_REQUIRE(workspace && workspace_bytes >= L.o_cw + (size_t)trip * L.stride, "OSDecoder: workspace too small");
  SAMD_REQUIRE(((uintptr_t)workspace & 7) == 0, "OSDecoder: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  hipLaunchKernelGGL(osd_binom_kernel, dim3(1), dim3(64), 0, s, (uint64_t*)ws, k, L.tw);
  for (int64_t b0 = 0; b0 < batch; b0 += kTrip) {
    const int64_t cws = batch - b0 < kTrip ? batch - b0 : kTrip;
    hipLaunchKernelGGL((osd_mrb_kernel<T>), dim3((unsigned)cws), dim3(64), mrb_lds(L, sizeof(T)), s, llr + (size_t)b0 * n, gm, L, ws);
    if (L.nb) {
      int rs;
      if (L.P <= 1) rs = launch_search<1>(L, cws, ws, s);
      else if (L.P <= 2) rs = launch_search<2>(L, cws, ws, s);
      else if (L.P <= 4) rs = launch_search<4>(L, cws, ws, s);
      else rs = launch_search<8>(L, cws, ws, s);
      if (rs != SAMD_OK) return rs;
    }
    hipLaunchKernelGGL((osd_final_kernel<T>), dim3((unsigned)cws), dim3(64), align_up((size_t)L.tw * 2, 8), s, L, ws,
                       out + (size_t)b0 * n);
  }
  return launch_status();
}

}  // namespace
}  // namespace samd

extern "C" size_t samd_osd_workspace_bytes(int k, int n, int t, int64_t batch) {
  samd::Lay L;
  if (batch <= 0 || samd::plan(k, n, t, &L) != SAMD_OK) return 0;
  return L.o_cw + (size_t)(batch < samd::kTrip ? batch : samd::kTrip) * L.stride;
}
extern "C" int samd_osd_decode_f32(const float* llr, const uint64_t* gm_rows, int64_t batch, int k, int n, int t, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return samd::decode<float>(llr, gm_rows, batch, k, n, t, out, workspace, workspace_bytes, stream);
}
extern "C" int samd_osd_decode_f64(const double* llr, const uint64_t* gm_rows, int64_t batch, int k, int n, int t, double* out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return samd::decode<double>(llr, gm_rows, batch, k, n, t, out, workspace, workspace_bytes, stream);
}
