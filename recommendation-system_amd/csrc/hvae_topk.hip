// hvae_topk.hip -- fused exact top-K over all items (full-ranking eval, /recommend core; K16 of SURVEY §2.1).
//
// Reference: RecommendationEvaluator.get_user_recommendations (src/ml/evaluate.py:137-147), HybridVAE.recommend
// (src/ml/model.py:236-256) and the /recommend handler (src/api/server.py:115-183) score ALL N items of a user
// in fp32 (u E^T), mask the seen ones to -inf and take np.argsort(scores)[::-1][:top_k]. Here the [R, N] score
// matrix never exists. With K_u = K + |seen_u| (seen items excluded) or K, s the fp32 score, s~ the bf16 MFMA
// score and eps_u >= |s~ - s| for every item of user u:
//
//   k_topk_seed        s~ of a strided sample of <= 4096 items per user (128 tiles of 32), and
//   k_topk_seed_select per user the K_u-th largest sample score r: t = r - eps_u <= T, the K_u-th largest fp32
//                      score over all items (K_u sample items have s >= r - eps_u); t is the user's starting bound;
//   k_topk_scan        one sweep of s~ over E (32 items x 32 users per 32x32x16 chain, E's fragments straight from
//                      global memory, u in registers). An item is a candidate when s~ >= t - eps_u: every true
//                      top-K_u item has s >= T >= t, hence s~ >= t - eps_u, so the candidates are a superset. The
//                      bound tightens during the sweep: a wave keeps, per user, a min-heap (LDS) of its K_u largest
//                      per-tile maxima of s~ (K_u distinct items, so root - eps_u <= T too) and publishes it with an
//                      atomic max per user (a larger t is still a lower bound, and a stale read only loosens the
//                      filter, so no ordering between blocks is needed);
//   k_topk_select      one block per user: exact fp32 rescore of the candidates against fp32 E (the score the
//                      reference ranks), seen items dropped, bitonic sort by (score desc, item desc) -- the order
//                      hvae_topk uses -- and the first K out.
// eps_u = ||u|| max||E|| (2^-7 + 2^-16 + 4 D 2^-24) x 1.02 (bf16 rounding of u and E, each off by up to 2^-8
// relative, so a product by up to 2^-7 + 2^-16; fp32 accumulation on both
// sides). Users whose candidate lists overflow (or that have fewer than K unseen items, or K_u > 256) are flagged
// and left to the caller's exact path.
//
// d = 1024: all of u as B fragments would be D / 4 = 256 VGPRs per lane, so the k axis is cut in two halves. The
// seed pass runs the halves one after the other (k_topk_seed_split), the LDS scan gives the halves to the two
// waves of a pair (k_topk_scan_lds, KH = 2). A score is then half 0's MFMA chain + half 1's, one fp32 add more
// than the single chain. eps_u keeps its formula: its 4 D 2^-24 term bounds the fp32 rounding of a D-term sum
// in ANY association (every summation tree of D terms has depth <= D - 1, so its error is at most
// (D - 1) 2^-24 sum |u_k e_k| <= D 2^-24 ||u|| ||e||; the term allows twice that for each of s~ and s), and
// two chains of D / 2 plus one add are such a tree.
//
// Host side: tk_plan(R, N, D, K, ab) is a pure function that decides a call once -- the scan, the user mapping,
// the splits and how the tiles are dealt over them (evenly: no split without a tile), both grids, the sample, the
// scan's LDS and the workspace as named offsets (hvae_topk_plan, include/hvae.h). hvae_topk_fused_workspace, hvae_topk_fused and the host query hvae_topk_fused_plan all take
// their numbers from it; kTkWidths is the one list of served widths, behind tk_serves and the one dispatch over D.
// The product library ships k_topk_scan_lds at every D % 128 == 0 and the global-load k_topk_scan at D = 64 only,
// always with wave_users = 1. The global-load scan at the other widths, the tile-split mapping (wave_users = 0)
// and the tau period are A/B switches (TkAb): read from the environment, instantiated and planned in builds with
// -DHVAE_AB=1 only (tests/ab_checks.py runs them).
#include <climits>
#include <cstdlib>
#include <type_traits>

#include "hvae_common.h"

namespace hvae {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kTkHeap = 256;    // per-user heap capacity (K_u <= 256)
// LDS heaps of one wave's 32 users sit cap + 1 floats apart, so that the same slot of every user's heap is on a
// different bank (a stride of cap floats put the 32 lanes' root reads on one bank: 32-way conflicts every tile)
constexpr int kTkHeapPad = 1;
constexpr int kTkSegCap = 256;  // candidates per (user, wave instance, lane half)
constexpr int kTkMaxCand = 4096;
constexpr int kTkMaxSeen = 2048;
constexpr int kTkSeedTiles = 128;
constexpr int kTkSeed = kTkSeedTiles * 32;

__device__ __forceinline__ uint32_t tk_pack_bf16x2(float lo, float hi) {
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}
// float <-> int with the same order (for atomicMax on signed ints)
__device__ __forceinline__ int tk_ord(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : (i ^ 0x7FFFFFFF);
}
__device__ __forceinline__ float tk_unord(int i) { return __int_as_float(i >= 0 ? i : (i ^ 0x7FFFFFFF)); }

// eps_u of the header from ||u||^2 and max ||E||
template <int D>
__device__ __forceinline__ float tk_eps(float usq, float emax) {
  return sqrtf(usq) * emax * (0x1p-7f + 0x1p-16f + 4.0f * D * 0x1p-24f) * 1.02f;
}

// S~^T of tile t (a 32x32 MFMA result): register r of lane half h holds this item
template <typename T>
__device__ __forceinline__ T tk_item(T t, int r, int h) {
  return t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
}

// bitonic network over P2 (a power of two) LDS slots by the block's 256 threads; cas(i, p, up) compares slots
// i < p and swaps them into the order of an `up` run
template <typename CAS>
__device__ __forceinline__ void tk_bitonic(int P2, int tid, CAS cas) {
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += 256) {
        const int p = i ^ j;
        if (p > i) cas(i, p, (i & k) == 0);
      }
      __syncthreads();
    }
}

struct TkScanArgs {
  const float* U;
  int64_t ldu;
  const bf16_t* E;         // bf16 [N, D] row-major
  const float* e_maxnorm;  // max_i ||E32_i||
  int64_t R, N;
  const int64_t* ex_row_ptr;  // exclude: CSR of the R users (nullable)
  const int32_t* ex_rows;
  const int64_t* ex_rows_offset;
  int K;
  int splits;
  int64_t tiles_per_split;  // of the first full_splits splits; the others take one fewer
  int full_splits;
  int* g_tau;          // [R] ordered-int lower bound t of the K_u-th fp32 score
  float* g_eps;        // [R] eps_u
  float* seed;         // [R][kTkSeed] sampled bf16 scores
  int32_t* cand;       // [R][nseg][kTkSegCap]
  int32_t* cand_cnt;   // [R][nseg]
  int nseg;            // segments per user: splits * 8 (wave_users 0) or splits * 2 (wave_users 1)
  int wave_users;      // 1: a block's 4 waves take 4 user groups over the same tiles (E read once per block
                       // from L2, the repeats served by the CU's L1); 0: one user group, waves split the tiles
  int tau_mask;        // other waves' bounds are read every tau_mask + 1 tiles (a power of two minus one)
};

// first tile of a split: the first full_splits splits take tiles_per_split tiles each and the others one fewer, so
// the tiles are dealt evenly and no split is empty while there are at least as many tiles as splits
__device__ __forceinline__ int64_t tk_split_begin(const TkScanArgs& a, int split) {
  return (int64_t)split * a.tiles_per_split - max(0, split - a.full_splits);
}

__device__ __forceinline__ int tk_ku(const TkScanArgs& a, int64_t r) {
  int ku = a.K;
  if (a.ex_row_ptr) {
    const int64_t m = batch_row(a.ex_rows, a.ex_rows_offset, r);
    ku += (int)(a.ex_row_ptr[m + 1] - a.ex_row_ptr[m]);
  }
  return ku;
}

// One wave's 32 users: u in registers as bf16 MFMA B fragments, in a permuted k order (group g of 64 k's,
// step j, lane half h -> k = 64 g + 32 h + 8 j .. + 7, the same order for E's A fragments, so a lane reads
// 64 contiguous bytes of an E row per group), and S~^T tiles of 32 items. With DK < D the scorer holds the DK
// k's from K0 on only: score() is then that part of the sum and usq that part of ||u||^2 (eps is unused).
template <int D, int DK = D, int K0 = 0>
struct TkScorer {
  static constexpr int NG = DK / 64;
  static_assert(DK % 64 == 0 && K0 % 64 == 0 && K0 + DK <= D, "TkScorer k range");
  uint4 uf[NG][4];
  float eps, usq;
  int h, col;

  __device__ __forceinline__ void load(const TkScanArgs& a, int64_t user, bool live, int lane) {
    h = lane >> 5;
    col = lane & 31;
    usq = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if (live) {
          const float* p = a.U + user * a.ldu + K0 + 64 * g + 32 * h + 8 * j;
          x = *reinterpret_cast<const float4*>(p);
          y = *reinterpret_cast<const float4*>(p + 4);
        }
        usq += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w) + (y.x * y.x + y.y * y.y) +
               (y.z * y.z + y.w * y.w);
        uf[g][j] = make_uint4(tk_pack_bf16x2(x.x, x.y), tk_pack_bf16x2(x.z, x.w), tk_pack_bf16x2(y.x, y.y),
                              tk_pack_bf16x2(y.z, y.w));
        __builtin_amdgcn_sched_barrier(0);
      }
    usq += __shfl_xor(usq, 32, 64);
    eps = tk_eps<D>(usq, *a.e_maxnorm);
  }

  // S~^T of tile t: lane (col = user, h) holds items 32 t + (r & 3) + 8 (r >> 2) + 4 h; past N: -inf
  __device__ __forceinline__ f32x16_t score(const TkScanArgs& a, int64_t t) const {
    f32x16_t s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const int64_t row = min(t * 32 + col, a.N - 1);  // rows past N: clamped, masked below
    const unsigned char* er = reinterpret_cast<const unsigned char*>(a.E) + row * (int64_t)(D * 2) + 2 * K0 + 64 * h;
    uint4 ea[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ea[0][j] = *reinterpret_cast<const uint4*>(er + 16 * j);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g + 1 < NG) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          ea[(g + 1) & 1][j] = *reinterpret_cast<const uint4*>(er + 128 * (g + 1) + 16 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ea[g & 1][j]),
                                                   __builtin_bit_cast(bf16x8_t, uf[g][j]), s, 0, 0, 0);
    }
    if (t * 32 + 32 > a.N) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (tk_item(t, r, h) >= a.N) s[r] = -INFINITY;
    }
    return s;
  }
};

// seed pass: s~ of sample tiles j * stride (j < nsample) -> seed[user][32 j + item in tile]; eps_u -> g_eps
template <int D>
__global__ void __launch_bounds__(256) k_topk_seed(TkScanArgs a, int64_t stride, int nsample) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t user = (int64_t)blockIdx.x * 32 + (lane & 31);
  const bool live = user < a.R;
  TkScorer<D> sc;
  sc.load(a, user, live, lane);
  if (live && w == 0 && sc.h == 0) a.g_eps[user] = sc.eps;
  for (int j = w; j < nsample; j += 4) {
    const f32x16_t s = sc.score(a, j * stride);
    if (live) {
#pragma unroll
      for (int r = 0; r < 16; ++r) a.seed[user * kTkSeed + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * sc.h] = s[r];
    }
  }
}

// The seed pass at d = 1024: the two D-halves one after the other, each over all of the wave's sample tiles.
// Half 0 stores its partial scores to seed[], half 1 adds its own to them (half 0 + half 1, the scan's order):
// the same lane wrote the address it reads back, so nothing has to be synchronised.
template <int D, int K0>
__device__ __forceinline__ float tk_seed_half(const TkScanArgs& a, int64_t user, bool live, int lane, int w,
                                              int64_t stride, int nsample) {
  TkScorer<D, D / 2, K0> sc;
  sc.load(a, user, live, lane);
  for (int j = w; j < nsample; j += 4) {
    const f32x16_t s = sc.score(a, j * stride);
    if (live) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* p = a.seed + user * kTkSeed + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * sc.h;
        *p = K0 == 0 ? s[r] : *p + s[r];
      }
    }
  }
  return sc.usq;
}

template <int D>
__global__ void __launch_bounds__(256) k_topk_seed_split(TkScanArgs a, int64_t stride, int nsample) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t user = (int64_t)blockIdx.x * 32 + (lane & 31);
  const bool live = user < a.R;
  float usq = tk_seed_half<D, 0>(a, user, live, lane, w, stride, nsample);
  usq += tk_seed_half<D, D / 2>(a, user, live, lane, w, stride, nsample);
  if (live && w == 0 && lane < 32) a.g_eps[user] = tk_eps<D>(usq, *a.e_maxnorm);
}

// per user: t = (K_u-th largest sample s~) - eps_u, or the lowest bound when the sample holds fewer than K_u items
__global__ void __launch_bounds__(256) k_topk_seed_select(TkScanArgs a, int nsample) {
  __shared__ float v[kTkSeed];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = nsample * 32;
  const int ku = tk_ku(a, r);
  int P2 = 1;
  while (P2 < n) P2 <<= 1;
  for (int i = tid; i < P2; i += 256) v[i] = i < n ? a.seed[r * kTkSeed + i] : -INFINITY;
  __syncthreads();
  tk_bitonic(P2, tid, [&](int i, int p, bool up) {  // descending
    const float x = v[i], y = v[p];
    if ((y > x) == up) { v[i] = y; v[p] = x; }
  });
  if (tid == 0) {
    const float kth = ku <= n ? v[ku - 1] : -INFINITY;
    a.g_tau[r] = kth > -INFINITY ? tk_ord(kth - a.g_eps[r]) : INT_MIN;
  }
}

// The per-tile selection of one wave's 32 users (shared by both scans): the heap of per-tile maxima (the pair's
// h == 0 lane), the bound t (own heap root - eps_u, other waves' via the atomic max), candidate emission.
struct TkSelect {
  float* hp;
  int cap, ku, h, sgw;
  int64_t user, seg;
  bool live;
  float eps, tau;
  int cnt = 0;
  __device__ __forceinline__ TkSelect(const TkScanArgs& a, float* heap, int cap_, int64_t user_, bool live_, int h_,
                                      float eps_, int ku_, int sgw_)
      : hp(heap), cap(cap_), ku(ku_ <= cap_ ? ku_ : 0), h(h_), sgw(sgw_), user(user_), live(live_), eps(eps_) {
    if (h == 0)
      for (int i = 0; i < cap; ++i) hp[i] = -INFINITY;
    tau = live ? tk_unord(a.g_tau[user]) : -INFINITY;  // bound t; the filter is s~ >= t - eps_u
    seg = (user * a.nseg + sgw + h) * kTkSegCap;
  }
  __device__ __forceinline__ void consume(const TkScanArgs& a, const f32x16_t& s, int64_t t, int64_t j) {
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, s[r]);
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (h == 0 && ku > 0 && m > hp[0]) {  // replace the root, sift down
      int i = 0;
      while (true) {
        const int l = 2 * i + 1;
        if (l >= ku) break;
        const int rr = l + 1;
        const int c = (rr < ku && hp[rr] < hp[l]) ? rr : l;
        if (hp[c] >= m) break;
        hp[i] = hp[c];
        i = c;
      }
      hp[i] = m;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the h == 0 lane's writes land before the pair reads
    const float root = ku > 0 ? hp[0] : -INFINITY;
    // a tighter own bound is published without waiting for the atomic's return; other waves' bounds are read
    // every tau_mask + 1 tiles (a returned atomic holds the wave for a device round trip). A stale bound only
    // loosens the filter, so neither needs ordering.
    if (live && root - eps > tau) {
      tau = root - eps;
      __hip_atomic_fetch_max(a.g_tau + user, tk_ord(tau), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (live && (j & a.tau_mask) == a.tau_mask)
      tau = fmaxf(tau, tk_unord(atomicMax(a.g_tau + user, INT_MIN)));  // other waves' bounds
    if (live) {
      const float thr = tau - eps;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (s[r] >= thr) {
          if (cnt < kTkSegCap) a.cand[seg + cnt] = (int32_t)tk_item(t, r, h);
          ++cnt;
        }
    }
  }
};

template <int D>
__global__ void __launch_bounds__(256) k_topk_scan(TkScanArgs a) {
  extern __shared__ float heap_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x % a.splits;
  const int64_t user = a.wave_users ? (int64_t)(blockIdx.x / a.splits) * 128 + 32 * w + (lane & 31)
                                    : (int64_t)(blockIdx.x / a.splits) * 32 + (lane & 31);
  const bool live = user < a.R;
  const int64_t ntiles = (a.N + 31) / 32;
  const int64_t t0 = tk_split_begin(a, split);
  const int64_t t1 = min(ntiles, tk_split_begin(a, split + 1));
  // this wave's tiles: t0 + tw, t0 + tw + ts, ... (every tile of the split with wave_users)
  const int tw = a.wave_users ? 0 : w, ts = a.wave_users ? 1 : 4;
  const int64_t nw = t1 > t0 + tw ? (t1 - t0 - tw + ts - 1) / ts : 0;
  const int sgw = a.wave_users ? split * 2 : (split * 4 + w) * 2;  // the wave's first segment of the user
  TkScorer<D> sc;
  sc.load(a, user, live, lane);
  const int h = sc.h;
  const int ku = live ? min(tk_ku(a, user), kTkHeap) : 0;  // K_u > kTkHeap: flagged by k_topk_select
  const float eps = sc.eps;

  TkSelect sel(a, heap_lds + (size_t)(w * 32 + (lane & 31)) * (kTkHeap + kTkHeapPad), kTkHeap, user, live, h, eps, ku,
               sgw);
  for (int64_t j = 0; j < nw; ++j) {
    const int64_t t = t0 + tw + ts * j;
    sel.consume(a, sc.score(a, t), t, j);
  }
  const int cnt = sel.cnt;
  if (live) a.cand_cnt[user * a.nseg + sgw + h] = cnt;
}


// ---- LDS-staged scan (D a multiple of 128): a block's 4 waves take 4 groups of 32 users over the same tiles;
// each 32-item E tile arrives once per block by LDS-DMA (three-slot ring, the decoder's image and piece map,
// one barrier per tile) and the 32x32x16 A operands are ds_read_b128 row reads of it. Per-user heaps of up to
// tkl_heap - 1 tile maxima (a user with K_u beyond it keeps the seed / other waves' bound, which is still valid).
// ring slots and heap capacity per D (LDS: slots x the tile + 4 waves x 32 users x the heap): d = 768 keeps two
// slots (the next tile's DMA overlaps the current tile's MFMAs) so that K_u up to 64 keeps its heap.
// d = 1024 (KH = 2): the 4 waves are 2 groups of 32 users x 2 D-halves, so a block takes 64 users. A wave holds
// the B fragments of its 512 k's (128 VGPRs) and runs its half of the chain over the tile; the odd wave of a pair
// hands its partial S~^T to the even wave through LDS (4 KiB per group, a second barrier per tile), which adds it
// (half 0 + half 1) and selects, so both of its lane halves see the same summed scores. LDS: 2 slots x 64 KiB
// + 8 KiB exchange + 2 x 32 heaps of 63 floats (16 KiB set aside) = 152 KiB.
constexpr int tkl_kh(int64_t D) { return D >= 1024 ? 2 : 1; }          // D-halves (waves per user group)
constexpr int tkl_block_users(int64_t D) { return 128 / tkl_kh(D); }  // users per block
constexpr int tkl_ns(int64_t D) { return D >= 768 ? 2 : 3; }
constexpr int tkl_heap(int64_t D) { return D >= 768 ? 64 : 128; }
constexpr int tkl_xchg_bytes(int64_t D) { return tkl_kh(D) == 2 ? (4 / tkl_kh(D)) * 4096 : 0; }
constexpr int64_t tkl_lds_bytes(int64_t D) {  // the plan's too, hence functions of a runtime D
  return tkl_ns(D) * ((D / 128) * 8192) + tkl_xchg_bytes(D) + tkl_block_users(D) * tkl_heap(D) * 4;
}

__device__ __forceinline__ uint32_t tk_lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
template <int n>
__device__ __forceinline__ void tk_wait_vmcnt() {
  static_assert(n >= 0 && n < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14));
}

template <int D>
__global__ void __launch_bounds__(256) k_topk_scan_lds(TkScanArgs a) {
  constexpr int NSEG = D / 128, TB = NSEG * 8192, PW = NSEG * 8 / 4, NS = tkl_ns(D);
  constexpr int KH = tkl_kh(D), KS = D / 16 / KH;  // a wave's k-steps: its D-half with KH = 2
  constexpr int HC = tkl_heap(D) - 1;  // heap capacity = stride: odd, so the 32 users' slots fall on 32 banks
  static_assert(D % 128 == 0 && tkl_lds_bytes(D) <= 160 * 1024, "k_topk_scan_lds shape");
  static_assert(KH == 1 || KS / 2 == PW, "the D-split chain issues one DMA piece every second k-step");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* heaps = reinterpret_cast<float*>(lds + NS * TB + tkl_xchg_bytes(D));
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, col = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ug = w / KH, kh = w % KH;  // the wave's user group and D-half (KH = 1: ug = w, kh = 0)
  const int split = blockIdx.x % a.splits;
  const int64_t user = (int64_t)(blockIdx.x / a.splits) * tkl_block_users(D) + 32 * ug + col;
  const bool live = user < a.R;
  const bool sel_live = live && kh == 0;  // the wave that selects for the group
  const int64_t ntiles = (a.N + 31) / 32;
  const int64_t t0 = tk_split_begin(a, split);
  const int64_t t1 = min(ntiles, tk_split_begin(a, split + 1));
  const int64_t nt = t1 > t0 ? t1 - t0 : 0;
  const float emax = *a.e_maxnorm;  // before any LDS-DMA is in flight

  // u as the B operand: lane holds U[user][16 (KS kh + ks) + 8 h .. + 7]
  const float* up = a.U + user * a.ldu + 16 * KS * kh + 8 * h;
  uint4 uf[KS];
  float usq = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
    if (live) {
      x = *reinterpret_cast<const float4*>(up + 16 * ks);
      y = *reinterpret_cast<const float4*>(up + 16 * ks + 4);
    }
    usq += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w) + (y.x * y.x + y.y * y.y) + (y.z * y.z + y.w * y.w);
    uf[ks] = make_uint4(tk_pack_bf16x2(x.x, x.y), tk_pack_bf16x2(x.z, x.w), tk_pack_bf16x2(y.x, y.y),
                        tk_pack_bf16x2(y.z, y.w));
    __builtin_amdgcn_sched_barrier(0);  // a few k-steps' loads in flight, not all (register peak)
  }
  usq += __shfl_xor(usq, 32, 64);
  if constexpr (KH == 2) {
    // ||u||^2 = half 0's part + half 1's, handed over through the pair's exchange area (free until the first
    // tile's barrier); only the selecting wave uses eps
    float* xu = reinterpret_cast<float*>(lds + NS * TB) + ug * 1024 + lane;
    if (kh == 1) *xu = usq;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kh == 0) usq += *xu;
  }
  const float eps = tk_eps<D>(usq, emax);
  const int ku = sel_live ? tk_ku(a, user) : 0;

  // LDS-DMA (the decoder's version-2 image: 8-row x 32-column subtiles, 2-bit chunk XOR)
  int vlane[2];
#pragma unroll
  for (int pb = 0; pb < 2; ++pb) {
    const int row = 8 * pb + ((lane >> 2) & 7);
    vlane[pb] = ((lane >> 2) & 7) * (D * 2) + 64 * (lane >> 5) + 16 * ((lane & 3) ^ ((row >> 2) & 3));
  }
  // the resource covers this split's items only (its extent is a 32-bit byte count: a whole E of more than
  // 2^31 bytes would wrap, and the bounds check would then read real items as zeros); tile offsets are split-relative
  const int64_t i_end = min(a.N, t1 * 32);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(a.E) + t0 * 32 * D, (short)0, (int)(i_end > t0 * 32 ? (i_end - t0 * 32) * D * 2 : 0),
      0x00020000);
  const uint32_t ring0 = tk_lds_addr(lds) + (uint32_t)(w * PW * 1024);
  auto issue_pieces = [&](uint32_t soff, int slot_i, int i0, int i1, bool fresh) {
    const uint32_t lb = ring0 + (uint32_t)(slot_i * TB);
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      const int p = w * PW + i;  // wave-uniform; PW need not be a multiple of 4 here, so p's own bits
      const uint32_t so = soff + (uint32_t)(8 * ((p >> 1) & 3) * (D * 2) + 256 * (p >> 3) + 128 * (p & 1));
      const int vo = ((p >> 1) & 1) ? vlane[1] : vlane[0];
      if (fresh && i == i0)
        asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                     :: "s"(lb + (uint32_t)(i * 1024)), "v"(vo), "s"(rsrc), "s"(so) : "memory");
      else
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                     :: "s"(lb + (uint32_t)(i * 1024)), "v"(vo), "s"(rsrc), "s"(so) : "memory");
    }
  };
  auto tile_soff = [&](int64_t t) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)((t - t0) * (int64_t)(32 * D * 2)));
  };
  auto barrier = [&] {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  const int laneA0 = ((col >> 3) << 11) + ((col & 7) << 6) + (((0 + h) ^ ((col >> 2) & 3)) << 4);
  const int laneA1 = ((col >> 3) << 11) + ((col & 7) << 6) + (((2 + h) ^ ((col >> 2) & 3)) << 4);

  // KH = 2: the odd wave of a pair builds the same (unused) selector on the pair's heap; its writes of -inf land
  // before the first tile's barrier, and it neither consumes nor counts
  TkSelect sel(a, heaps + (ug * 32 + col) * HC, HC, user, sel_live, h, eps, ku, split * 2);
  float4* xchg = reinterpret_cast<float4*>(lds + NS * TB) + ug * 256 + lane;  // KH = 2: [4][64 lanes] per group
  if (nt > 0) {
    issue_pieces(tile_soff(t0), 0, 0, PW, true);
    if (NS == 3) issue_pieces(tile_soff(min(t0 + 1, t1 - 1)), 1, 0, PW, true);
  }
  for (int64_t j = 0; j < nt; ++j) {
    const int64_t t = t0 + j;
    const int cur = (int)(j % NS), s_dma = (int)((j + NS - 1) % NS);
    // tile t has landed (three slots: issued two iterations back, younger ops may stay in flight; two slots:
    // issued in the previous iteration, so everything is waited for)
    if constexpr (NS == 3) tk_wait_vmcnt<PW>();
    else tk_wait_vmcnt<0>();
    barrier();  // every wave's pieces of t; every wave is done with the slot the next DMA reuses
    const uint32_t soff_dma = tile_soff(min(t + NS - 1, t1 - 1));
    const unsigned char* b0 = lds + cur * TB + kh * (TB / KH) + laneA0;  // the wave's D-half of the tile
    const unsigned char* b1 = lds + cur * TB + kh * (TB / KH) + laneA1;
    auto rdA = [&](int ks) {
      const int grp = ks >> 1;
      return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(((ks & 1) ? b1 : b0) + ((grp >> 2) << 13) +
                                                                          ((grp & 3) << 9)));
    };
    f32x16_t s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    bf16x8_t an[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) an[q] = rdA(q);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8_t c = an[ks & 3];
      if (ks + 4 < KS) an[ks & 3] = rdA(ks + 4);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(c, __builtin_bit_cast(bf16x8_t, uf[ks]), s, 0, 0, 0);
      if ((ks & 1) == 1 && (ks >> 1) < PW) issue_pieces(soff_dma, s_dma, ks >> 1, (ks >> 1) + 1, ks == 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (KS / 2 < PW) issue_pieces(soff_dma, s_dma, KS / 2, PW, false);
    if constexpr (KH == 2) {
      // half 1's partial sums go to the pair's even wave: s = half 0 + half 1, every element added once in
      // that order. The even wave has read the previous tile's exchange before the barrier above.
      if (kh == 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) xchg[64 * q] = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
      }
      barrier();
      if (kh == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 p = xchg[64 * q];
          s[4 * q] += p.x;
          s[4 * q + 1] += p.y;
          s[4 * q + 2] += p.z;
          s[4 * q + 3] += p.w;
        }
      }
    }
    if (t * 32 + 32 > a.N) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (tk_item(t, r, h) >= a.N) s[r] = -INFINITY;
    }
    if (kh == 0) sel.consume(a, s, t, j);
  }
  tk_wait_vmcnt<0>();  // the LDS-DMA lands before the block's LDS is released
  if (sel_live) a.cand_cnt[user * a.nseg + split * 2 + h] = sel.cnt;
}

// (score desc, item desc): a before b
__device__ __forceinline__ bool tk_before(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && ia > ib);
}

struct TkSelArgs {
  const float* U;
  int64_t ldu;
  const float* E32;
  int64_t R, N, D;
  const int64_t* ex_row_ptr;
  const int32_t* ex_col;
  const int32_t* ex_rows;
  const int64_t* ex_rows_offset;
  int K;
  const int32_t* cand;
  const int32_t* cand_cnt;
  int nseg;
  int32_t* idx;  // [R, K]
  float* val;    // [R, K] (nullable)
  int32_t* flag; // [R]
};

template <int NK>  // D / 64
__global__ void __launch_bounds__(256) k_topk_select(TkSelArgs a) {
  __shared__ float ss[kTkMaxCand];
  __shared__ int si[kTkMaxCand];
  __shared__ int seen[kTkMaxSeen];
  __shared__ int s_off[1025];
  __shared__ int s_bad;
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int nseen = 0;
  int64_t m = 0;
  if (a.ex_row_ptr) {
    m = batch_row(a.ex_rows, a.ex_rows_offset, r);
    nseen = (int)(a.ex_row_ptr[m + 1] - a.ex_row_ptr[m]);
  }
  // candidate offsets per segment (nseg <= 1024)
  if (tid == 0) {
    int tot = 0, bad = 0;
    for (int sgi = 0; sgi < a.nseg; ++sgi) {
      const int c = a.cand_cnt[r * a.nseg + sgi];
      bad |= c > kTkSegCap;
      s_off[sgi] = tot;
      tot += min(c, kTkSegCap);
    }
    s_off[a.nseg] = tot;
    bad |= tot > kTkMaxCand || nseen > kTkMaxSeen || a.K + nseen > kTkHeap || tot < a.K;
    s_bad = bad;
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) a.flag[r] = 1;
    return;
  }
  const int C = s_off[a.nseg];
  // seen items, sorted ascending (bitonic over the next power of two)
  int P2s = 1;
  while (P2s < nseen) P2s <<= 1;
  for (int i = tid; i < P2s; i += 256) seen[i] = i < nseen ? a.ex_col[a.ex_row_ptr[m] + i] : INT_MAX;
  __syncthreads();
  tk_bitonic(P2s, tid, [&](int i, int p, bool up) {
    const int x = seen[i], y = seen[p];
    if ((x > y) == up) { seen[i] = y; seen[p] = x; }
  });
  // gather the candidates
  for (int sgi = 0; sgi < a.nseg; ++sgi) {
    const int o = s_off[sgi], n = s_off[sgi + 1] - o;
    for (int i = tid; i < n; i += 256) si[o + i] = a.cand[(r * a.nseg + sgi) * kTkSegCap + i];
  }
  __syncthreads();
  // exact fp32 rescore: 16 lanes per candidate, 4 candidates per wave pass; lane g of a group owns float4
  // columns g + 16 k (k < NK) of u (in registers) and of the candidate's E row, all NK loads in flight; the sum
  // is over k in order, then a fixed xor tree over the group (deterministic)
  const float* u = a.U + r * a.ldu;
  const int g = lane & 15, slot = lane >> 4;
  float4 u4[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) u4[k] = *reinterpret_cast<const float4*>(u + 4 * (g + 16 * k));
  for (int c0 = w * 4; c0 < C; c0 += 16) {
    const int c = c0 + slot;
    const int it = c < C ? si[c] : 0;
    const float4* e = reinterpret_cast<const float4*>(a.E32 + (int64_t)it * (16 * 4 * NK));
    float4 e4[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) e4[k] = e[g + 16 * k];
    float sdot = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      sdot += (u4[k].x * e4[k].x + u4[k].y * e4[k].y) + (u4[k].z * e4[k].z + u4[k].w * e4[k].w);
    sdot += __shfl_xor(sdot, 8, 64);
    sdot += __shfl_xor(sdot, 4, 64);
    sdot += __shfl_xor(sdot, 2, 64);
    sdot += __shfl_xor(sdot, 1, 64);
    if (g == 0 && c < C) {
      int lo = 0, hi = nseen;  // binary search in the sorted seen list
      while (lo < hi) {
        const int md = (lo + hi) >> 1;
        if (seen[md] < it) lo = md + 1;
        else hi = md;
      }
      const bool is_seen = lo < nseen && seen[lo] == it;
      ss[c] = (is_seen || sdot != sdot) ? -INFINITY : sdot;
    }
  }
  __syncthreads();
  int P2 = 1;
  while (P2 < C) P2 <<= 1;
  for (int i = C + tid; i < P2; i += 256) { ss[i] = -INFINITY; si[i] = -1; }
  __syncthreads();
  // bitonic sort, "before" first
  tk_bitonic(P2, tid, [&](int i, int p, bool up) {
    const float x = ss[i], y = ss[p];
    const int xi = si[i], yi = si[p];
    if (tk_before(y, yi, x, xi) == up) { ss[i] = y; si[i] = yi; ss[p] = x; si[p] = xi; }
  });
  // fewer than K finite candidates (seen items ate the shortlist): the exact path decides
  if (tid == 0) a.flag[r] = !(ss[a.K - 1] > -INFINITY);
  for (int i = tid; i < a.K; i += 256) {
    a.idx[r * a.K + i] = si[i];
    if (a.val) a.val[r * a.K + i] = ss[i];
  }
}

// ---- host: one plan per call ----

// A/B overrides of the plan, in the environment of builds with -DHVAE_AB=1 only (read at every plan); the default is
// the product's, and the product build has no other
struct TkAb {
  int lds_scan = 1;    // HVAE_TOPK_LDS=0: the global-load scan where D % 128 == 0 too
  int wave_users = 1;  // HVAE_TOPK_WAVE_USERS=0: the global-load scan's tile-split mapping
  int tau_period = 8;  // HVAE_TK_TAU_PERIOD: tiles between reads of the other waves' bounds (a power of two, else 8)
};
static TkAb tk_ab() {
  TkAb ab;
#if HVAE_AB
  auto env = [](const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
  };
  ab.lds_scan = env("HVAE_TOPK_LDS", ab.lds_scan) != 0;
  ab.wave_users = env("HVAE_TOPK_WAVE_USERS", ab.wave_users) != 0;
  ab.tau_period = env("HVAE_TK_TAU_PERIOD", ab.tau_period);
#endif
  return ab;
}

// The served widths: tk_serves and tk_dispatch both go by this list, and D / 64 (k_topk_select), the seed's k
// ranges and the scan's form follow from D in hvae_topk_fused's dispatched launch.
constexpr int kTkWidths[] = {64, 128, 256, 384, 512, 768, 1024};
constexpr int kTkNumWidths = sizeof(kTkWidths) / sizeof(kTkWidths[0]);
constexpr bool tk_serves(int64_t D, int64_t K) {
  for (int w : kTkWidths)
    if (D == w) return K <= kTkHeap;
  return false;
}
// f(std::integral_constant<int, D>) for the served D
template <int I = 0, typename F>
static int tk_dispatch(int64_t D, F&& f) {
  if constexpr (I == kTkNumWidths) {
    HVAE_FAIL(HVAE_ERR_UNSUPPORTED, "hvae_topk_fused: no kernel for D = %lld", (long long)D);
  } else {
    return D == kTkWidths[I] ? f(std::integral_constant<int, kTkWidths[I]>{}) : tk_dispatch<I + 1>(D, f);
  }
}

// a split's bf16 slice of E must stay below 2^31 bytes (the LDS scan's buffer resource extent is 32-bit): with
// cdiv(bytes, 2^30) splits a slice is at most 2^30 bytes + one tile (64 KiB at d = 1024's 2048 B per row)
constexpr int64_t kTkSplitBytes = (int64_t)1 << 30;

struct TkRefusal {
  int code;         // HVAE_OK: the plan stands
  const char* why;
};

// Everything a call needs, decided once. Every field is filled in whatever the verdict (an unserved width is sized
// as the scan its D would get: hvae_topk_fused_workspace answers for those too); the verdict says whether
// hvae_topk_fused runs it.
static TkRefusal tk_plan(int64_t R, int64_t N, int64_t D, int64_t K, const TkAb& ab, hvae_topk_plan* p) {
  bool lds = D % 128 == 0;
  int wu = 1;
  if constexpr (HVAE_AB != 0) {  // the product plans the LDS scan wherever it exists, and one mapping
    lds = lds && ab.lds_scan != 0;
    if (!lds) wu = ab.wave_users != 0;
  }
  p->scan = !lds ? HVAE_TOPK_SCAN_GLOBAL : tkl_kh(D) == 2 ? HVAE_TOPK_SCAN_LDS_KH2 : HVAE_TOPK_SCAN_LDS;
  p->wave_users = wu;
  p->block_users = lds ? tkl_block_users(D) : wu ? 128 : 32;
  const int64_t groups = std::max<int64_t>(1, cdiv(R, p->block_users));  // R = 0: a workspace query
  const int64_t tiles = cdiv(N, 32);
  int64_t s = std::max<int64_t>(1, cdiv(256, groups));  // ~256 blocks (one per CU: 128 KiB of heaps each)
  s = std::min<int64_t>(s, std::max<int64_t>(1, tiles / (wu ? 4 : 16)));  // >= 4 tiles per wave
  s = std::max<int64_t>(s, cdiv(tiles * 32 * D * 2, kTkSplitBytes));  // large E: enough splits for the extent
  s = std::min<int64_t>(s, wu ? 512 : 128);  // nseg <= 1024
  p->splits = (int)s;
  p->tiles_per_split = cdiv(tiles, s);
  p->full_splits = (int)(tiles - s * (p->tiles_per_split - 1));  // the other splits take one tile fewer
  p->nseg = p->splits * (wu ? 2 : 8);
  p->blocks = cdiv(R, p->block_users) * s;
  p->seed_blocks = cdiv(R, 32);  // the seed pass: one block per 32 users
  p->nsample = (int)std::min<int64_t>(tiles, kTkSeedTiles);
  p->stride = std::max<int64_t>(1, tiles / std::max(1, p->nsample));
  p->tau_period = (ab.tau_period >= 1 && (ab.tau_period & (ab.tau_period - 1)) == 0) ? ab.tau_period : 8;
  p->lds_bytes = lds ? (size_t)tkl_lds_bytes(D) : (size_t)4 * 32 * (kTkHeap + kTkHeapPad) * 4;
  // workspace: 256 B | tau [R] | eps [R] | cnt [R][nseg] | cand [R][nseg][kTkSegCap] | seed [R][kTkSeed]
  p->off_tau = 256;
  p->off_eps = p->off_tau + (size_t)R * 4;
  p->off_cnt = p->off_eps + (size_t)R * 4;
  p->off_cand = p->off_cnt + (size_t)R * p->nseg * 4;
  p->off_seed = p->off_cand + (size_t)R * p->nseg * kTkSegCap * 4;
  p->workspace = p->off_seed + (size_t)R * kTkSeed * 4;

  if (!tk_serves(D, K)) return {HVAE_ERR_UNSUPPORTED, "D must be 64, 128, 256, 384, 512, 768 or 1024, K <= 256"};
  if (R < 0 || N <= 0 || K <= 0) return {HVAE_ERR_ARG, "bad args"};
  // d = 1024 has the D-split LDS scan only: the global-load scan (A/B: HVAE_TOPK_LDS=0) would keep all of u in
  // registers and spill, so it is not instantiated
  if (!lds && tkl_kh(D) == 2) return {HVAE_ERR_UNSUPPORTED, "D = 1024 has no global-load scan"};
  if (K > N || N >= INT32_MAX) return {HVAE_ERR_ARG, "bad args"};
  if (lds && p->tiles_per_split * 32 * D * 2 >= ((int64_t)1 << 31))
    return {HVAE_ERR_ARG, "a split of E exceeds 2^31 bytes"};
  return {HVAE_OK, nullptr};
}

}  // namespace hvae

using namespace hvae;

extern "C" size_t hvae_topk_fused_workspace(int64_t R, int64_t N, int64_t D, int64_t K) {
  hvae_topk_plan p;
  tk_plan(R, N, D, K, tk_ab(), &p);
  return p.workspace;
}

extern "C" int hvae_topk_fused_plan(int64_t R, int64_t N, int64_t D, int64_t K, hvae_topk_plan* out) {
  HVAE_REQUIRE(out, "hvae_topk_fused_plan: null out");
  const TkRefusal no = tk_plan(R, N, D, K, tk_ab(), out);
  if (no.code != HVAE_OK) HVAE_FAIL(no.code, "hvae_topk_fused_plan: %s", no.why);
  return HVAE_OK;
}

extern "C" int hvae_topk_fused(const float* U, int64_t ldu, const void* E_bf16, const float* E32,
                               const float* e32_maxnorm, int64_t N, int64_t D, const hvae_csr_batch* exclude,
                               int64_t R, int64_t K, int32_t* idx, float* val, int32_t* flag, void* ws,
                               size_t ws_bytes, void* stream) {
  hvae_topk_plan pl;
  const TkRefusal no = tk_plan(R, N, D, K, tk_ab(), &pl);
  if (no.code != HVAE_OK) HVAE_FAIL(no.code, "hvae_topk_fused: %s", no.why);
  HVAE_REQUIRE(ldu >= D, "hvae_topk_fused: bad args");
  if (R == 0) return HVAE_OK;  // an empty batch: its (empty) output tensors may have null data pointers
  HVAE_REQUIRE(U && E_bf16 && E32 && e32_maxnorm && idx && flag, "hvae_topk_fused: null pointer");
  HVAE_REQUIRE(ws && ws_bytes >= pl.workspace, "hvae_topk_fused: workspace too small");
  if (exclude)
    HVAE_REQUIRE(exclude->row_ptr && exclude->col_idx && exclude->nb == R, "hvae_topk_fused: bad exclude");
  hipStream_t st = as_stream(stream);
  unsigned char* w = static_cast<unsigned char*>(ws);
  int32_t* cnt = reinterpret_cast<int32_t*>(w + pl.off_cnt);
  int32_t* cand = reinterpret_cast<int32_t*>(w + pl.off_cand);
  HVAE_HIP(hipMemsetAsync(cnt, 0, pl.off_cand - pl.off_cnt, st));
  HVAE_HIP(hipMemsetAsync(flag, 0, (size_t)R * 4, st));
  const TkScanArgs sa{U, ldu, static_cast<const bf16_t*>(E_bf16), e32_maxnorm, R, N,
                      exclude ? exclude->row_ptr : nullptr, exclude ? exclude->rows : nullptr,
                      exclude ? exclude->rows_offset : nullptr, (int)K, pl.splits, pl.tiles_per_split,
                      pl.full_splits,
                      reinterpret_cast<int*>(w + pl.off_tau), reinterpret_cast<float*>(w + pl.off_eps),
                      reinterpret_cast<float*>(w + pl.off_seed), cand, cnt, pl.nseg, pl.wave_users,
                      pl.tau_period - 1};
  const TkSelArgs la{U, ldu, E32, R, N, D, exclude ? exclude->row_ptr : nullptr,
                     exclude ? exclude->col_idx : nullptr, exclude ? exclude->rows : nullptr,
                     exclude ? exclude->rows_offset : nullptr, (int)K, cand, cnt, pl.nseg, idx, val, flag};
  return tk_dispatch(D, [&](auto width) -> int {
    constexpr int DD = decltype(width)::value;
    const dim3 seed_grid((unsigned)pl.seed_blocks);
    if constexpr (tkl_kh(DD) == 2) k_topk_seed_split<DD><<<seed_grid, 256, 0, st>>>(sa, pl.stride, pl.nsample);
    else k_topk_seed<DD><<<seed_grid, 256, 0, st>>>(sa, pl.stride, pl.nsample);
    HVAE_LAUNCH_CHECK("k_topk_seed");
    k_topk_seed_select<<<(unsigned)R, 256, 0, st>>>(sa, pl.nsample);
    HVAE_LAUNCH_CHECK("k_topk_seed_select");
    // the global-load scan where the LDS scan exists is an A/B arm: the product neither plans nor holds it
    constexpr bool has_global = DD % 128 != 0 || (HVAE_AB != 0 && tkl_kh(DD) == 1);
    if (pl.scan != HVAE_TOPK_SCAN_GLOBAL) {
      if constexpr (DD % 128 == 0) {
        HVAE_HIP(hipFuncSetAttribute((const void*)k_topk_scan_lds<DD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)pl.lds_bytes));
        k_topk_scan_lds<DD><<<(unsigned)pl.blocks, 256, pl.lds_bytes, st>>>(sa);
      }
    } else if constexpr (has_global) {
      HVAE_HIP(hipFuncSetAttribute((const void*)k_topk_scan<DD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)pl.lds_bytes));
      k_topk_scan<DD><<<(unsigned)pl.blocks, 256, pl.lds_bytes, st>>>(sa);
    } else {
      HVAE_FAIL(HVAE_ERR_UNSUPPORTED, "hvae_topk_fused: this build has no global-load scan at D = %d", DD);
    }
    HVAE_LAUNCH_CHECK("k_topk_scan");
    k_topk_select<DD / 64><<<(unsigned)R, 256, 0, st>>>(la);
    HVAE_LAUNCH_CHECK("k_topk_select");
    return HVAE_OK;
  });
}
