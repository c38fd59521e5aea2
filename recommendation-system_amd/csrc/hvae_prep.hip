// hvae_prep.hip -- (K23) the index work of `make preprocess` on the device: label encoding of string ids, the
// k-core filter, the leave-one-out split and the interaction matrix (src/preprocessing/cleaning.py:86-117 and
// src/preprocessing/dataset.py:37-91 of the reference), over integer columns only. pandas keeps the text.
//
// Every result is an integer, or an fp32 sum of a few 0 / 1 ratings taken in input order, so every output is exact
// and two runs give the same bits. The only atomics are integer adds (histograms, removal counts, row lengths).
// Sorting is rocprim::radix_sort_pairs (stable) and the scans are rocprim's, as in hvae_rgsort.hip; the rest is
// plain grid-stride kernels over at most 2^31 - 1 records with 64-bit index arithmetic. The caller owns every
// buffer, the workspace (the *_workspace queries) and the stream; nothing here allocates or waits, and the k-core
// rounds are all enqueued at once: a round after convergence finds the previous round's removal count at zero and
// returns at once.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "hvae_common.h"

namespace hvae {
namespace {

constexpr int64_t kPrepMaxN = ((int64_t)1 << 31) - 1;
constexpr unsigned long long kSignBit = 0x8000000000000000ull;

int bits_for(int64_t n_values) {  // key bits that hold 0 .. n_values - 1
  int b = 1;
  while (b < 32 && ((int64_t)1 << b) < n_values) ++b;
  return b;
}
unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256), 4096)); }
size_t al256(size_t bytes) { return (bytes + 255) / 256 * 256; }

size_t sort64_temp(int64_t n) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                  (const unsigned*)nullptr, (unsigned*)nullptr, (unsigned)n, 0, 64);
  return b;
}
size_t sort32_temp(int64_t n) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr,
                                  (unsigned*)nullptr, (unsigned)n, 0, 32);
  return b;
}
size_t scan32_temp(int64_t n) {
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (const unsigned*)nullptr, (unsigned*)nullptr, (unsigned)n,
                                rocprim::plus<unsigned>());
  return b;
}
size_t scan64_temp(int64_t n) {
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                (unsigned)n, rocprim::plus<unsigned long long>());
  return b;
}

// A carved workspace: regions in 256-byte steps, the same walk for the query and the call.
struct Carve {
  char* base;
  size_t off = 0;
  explicit Carve(void* p) : base(static_cast<char*>(p)) {}
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += al256(count * sizeof(T));
    return p;
  }
};

#define PREP_LOOP(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256) k_prep_iota(uint32_t* __restrict__ perm, int64_t n) {
  PREP_LOOP(i, n) perm[i] = (uint32_t)i;
}

// ------------------------------------------------------------------ encode --
// word w of the records in the current order
__global__ void __launch_bounds__(256) k_prep_gather_word(const unsigned long long* __restrict__ keys, int W, int w,
                                                          const uint32_t* __restrict__ perm, int64_t n,
                                                          unsigned long long* __restrict__ out) {
  PREP_LOOP(i, n) out[i] = keys[(int64_t)perm[i] * W + w];
}

// head[i] = 1 where sorted record i differs from its predecessor in any of the W words
__global__ void __launch_bounds__(256) k_prep_key_heads(const unsigned long long* __restrict__ keys, int W,
                                                        const uint32_t* __restrict__ perm, int64_t n,
                                                        uint32_t* __restrict__ head) {
  PREP_LOOP(i, n) {
    uint32_t h = 1;
    if (i > 0) {
      const unsigned long long* a = keys + (int64_t)perm[i] * W;
      const unsigned long long* b = keys + (int64_t)perm[i - 1] * W;
      h = 0;
      for (int w = 0; w < W; ++w) h |= (a[w] != b[w]) ? 1u : 0u;
    }
    head[i] = h;
  }
}

// seg = inclusive scan of head: the class of sorted record i is seg[i] - 1. The sort is stable, so the head of a
// class is its smallest record index.
__global__ void __launch_bounds__(256) k_prep_encode_emit(const uint32_t* __restrict__ perm,
                                                          const uint32_t* __restrict__ head,
                                                          const uint32_t* __restrict__ seg, int64_t n,
                                                          int32_t* __restrict__ codes, int32_t* __restrict__ first,
                                                          int32_t* __restrict__ n_classes) {
  PREP_LOOP(i, n) {
    const int32_t c = (int32_t)seg[i] - 1;
    const uint32_t p = perm[i];
    codes[p] = c;
    if (head[i]) first[c] = (int32_t)p;
    if (i == n - 1) *n_classes = c + 1;
  }
}

struct EncodeWs {
  unsigned long long *kbuf, *kbuf_s;
  uint32_t *perm, *perm_s, *head, *seg;
  void* temp;
  size_t temp_bytes, total;
};
EncodeWs encode_ws(void* ws, int64_t n) {
  Carve c(ws);
  EncodeWs L{};
  L.kbuf = c.take<unsigned long long>(n);
  L.kbuf_s = c.take<unsigned long long>(n);
  L.perm = c.take<uint32_t>(n);
  L.perm_s = c.take<uint32_t>(n);
  L.head = c.take<uint32_t>(n);
  L.seg = c.take<uint32_t>(n);
  L.temp_bytes = std::max(sort64_temp(n), scan32_temp(n));
  L.temp = c.take<char>(L.temp_bytes);
  L.total = c.off;
  return L;
}

// ------------------------------------------------------------------- kcore --
// state words (uint32): [0] records with a code out of range (dead from the start), [1 + r] records round r removed
__global__ void __launch_bounds__(256) k_prep_kcore_init(const int32_t* __restrict__ ucode,
                                                         const int32_t* __restrict__ icode, int64_t n, int64_t n_users,
                                                         int64_t n_items, uint8_t* __restrict__ alive,
                                                         uint32_t* __restrict__ state) {
  PREP_LOOP(i, n) {
    const int32_t u = ucode[i], t = icode[i];
    const bool ok = u >= 0 && u < n_users && t >= 0 && t < n_items;
    alive[i] = ok ? 1 : 0;
    if (!ok) atomicAdd(&state[0], 1u);
  }
}

// a round runs while the one before it removed something (round 0 always runs)
__device__ __forceinline__ bool round_runs(const uint32_t* state, int r) { return r == 0 || state[r] != 0; }

__global__ void __launch_bounds__(256) k_prep_kcore_zero(int32_t* __restrict__ cnt, int64_t m,
                                                         const uint32_t* __restrict__ state, int r) {
  if (!round_runs(state, r)) return;
  PREP_LOOP(i, m) cnt[i] = 0;
}

__global__ void __launch_bounds__(256) k_prep_kcore_hist(const int32_t* __restrict__ code,
                                                         const uint8_t* __restrict__ alive, int64_t n,
                                                         int32_t* __restrict__ cnt, const uint32_t* __restrict__ state,
                                                         int r) {
  if (!round_runs(state, r)) return;
  PREP_LOOP(i, n) {
    if (alive[i]) atomicAdd(&cnt[code[i]], 1);  // alive records have codes in range (k_prep_kcore_init)
  }
}

__global__ void __launch_bounds__(256) k_prep_kcore_kill(const int32_t* __restrict__ code, uint8_t* __restrict__ alive,
                                                         int64_t n, const int32_t* __restrict__ cnt, int32_t min_count,
                                                         uint32_t* __restrict__ state, int r) {
  if (!round_runs(state, r)) return;
  uint32_t killed = 0;
  PREP_LOOP(i, n) {
    if (alive[i] && cnt[code[i]] < min_count) {
      alive[i] = 0;
      ++killed;
    }
  }
  for (int o = 32; o > 0; o >>= 1) killed += __shfl_xor(killed, o, 64);
  if ((threadIdx.x & 63) == 0 && killed) atomicAdd(&state[1 + r], killed);
}

__global__ void k_prep_kcore_finish(const uint32_t* __restrict__ state, int max_iterations, int64_t n,
                                    int64_t* __restrict__ n_alive, int32_t* __restrict__ rounds) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t live = n - (int64_t)state[0];
  int32_t worked = 0;
  for (int r = 0; r < max_iterations; ++r) {
    live -= (int64_t)state[1 + r];
    worked += state[1 + r] != 0 ? 1 : 0;
  }
  *n_alive = live;
  *rounds = worked;
}

struct KcoreWs {
  int32_t *ucnt, *icnt;
  uint32_t* state;
  size_t state_words, total;
};
KcoreWs kcore_ws(void* ws, int64_t n_users, int64_t n_items, int max_iterations) {
  Carve c(ws);
  KcoreWs L{};
  L.ucnt = c.take<int32_t>(n_users);
  L.icnt = c.take<int32_t>(n_items);
  L.state_words = (size_t)max_iterations + 2;  // state[1 + max_iterations] is read by no round and stays zero
  L.state = c.take<uint32_t>(L.state_words);
  L.total = c.off;
  return L;
}

// ------------------------------------------------------------------- split --
__global__ void __launch_bounds__(256) k_prep_ts_keys(const int64_t* __restrict__ ts, int64_t n,
                                                      unsigned long long* __restrict__ key,
                                                      uint32_t* __restrict__ perm) {
  PREP_LOOP(i, n) {
    key[i] = (unsigned long long)ts[i] ^ kSignBit;  // signed order as unsigned order
    perm[i] = (uint32_t)i;
  }
}

__global__ void __launch_bounds__(256) k_prep_gather_code(const int32_t* __restrict__ code,
                                                          const uint32_t* __restrict__ perm, int64_t n,
                                                          uint32_t* __restrict__ out) {
  PREP_LOOP(i, n) out[i] = (uint32_t)code[perm[i]];
}

// Membership of sorted record i. With rank = its place from the end of its user's run (1 = last) and count = the
// run's length: test is rank 1 and count >= 2, val is rank 2 and count >= 3, train is the rest. Both conditions
// need rank and count only up to 3, which the record's three neighbours settle: rank from the two after it, and
// count >= rank + 1 from the one before it (the run holds rank records from i on).
// flag = val in the low word, test in the high word, so one 64-bit scan carries both running counts (each < 2^31).
__global__ void __launch_bounds__(256) k_prep_split_flags(const uint32_t* __restrict__ ukey, int64_t n,
                                                          unsigned long long* __restrict__ flag) {
  PREP_LOOP(i, n) {
    const uint32_t u = ukey[i];
    const bool next1 = i + 1 < n && ukey[i + 1] == u;
    const bool next2 = i + 2 < n && ukey[i + 2] == u;
    const bool prev = i > 0 && ukey[i - 1] == u;
    const int rank = !next1 ? 1 : (!next2 ? 2 : 3);  // 3 stands for 3 or more
    const bool test = rank == 1 && prev;             // count >= 2
    const bool val = rank == 2 && prev;              // count >= 3
    flag[i] = (val ? 1ull : 0ull) | (test ? (1ull << 32) : 0ull);
  }
}

__global__ void __launch_bounds__(256) k_prep_split_emit(const uint32_t* __restrict__ perm,
                                                         const unsigned long long* __restrict__ flag,
                                                         const unsigned long long* __restrict__ incl, int64_t n,
                                                         int32_t* __restrict__ perm_out, int32_t* __restrict__ train,
                                                         int32_t* __restrict__ val, int32_t* __restrict__ test,
                                                         int64_t* __restrict__ lens) {
  PREP_LOOP(i, n) {
    const unsigned long long f = flag[i], s = incl[i];
    const int64_t nv = (int64_t)(s & 0xffffffffull), nt = (int64_t)(s >> 32);  // inclusive counts
    const int32_t p = (int32_t)perm[i];
    perm_out[i] = p;
    if (f & 0xffffffffull)
      val[nv - 1] = p;
    else if (f >> 32)
      test[nt - 1] = p;
    else
      train[i - nv - nt] = p;
    if (i == n - 1) {
      lens[0] = n - nv - nt;
      lens[1] = nv;
      lens[2] = nt;
    }
  }
}

struct SplitWs {
  unsigned long long *key, *key_s, *flag, *incl;
  uint32_t *perm, *perm_s, *ukey, *ukey_s;
  void* temp;
  size_t temp_bytes, total;
};
SplitWs split_ws(void* ws, int64_t n) {
  Carve c(ws);
  SplitWs L{};
  L.key = c.take<unsigned long long>(n);
  L.key_s = c.take<unsigned long long>(n);
  L.flag = L.key;  // the timestamp keys are dead once the second sort has run
  L.incl = L.key_s;
  L.perm = c.take<uint32_t>(n);
  L.perm_s = c.take<uint32_t>(n);
  L.ukey = c.take<uint32_t>(n);
  L.ukey_s = c.take<uint32_t>(n);
  L.temp_bytes = std::max(std::max(sort64_temp(n), sort32_temp(n)), scan64_temp(n));
  L.temp = c.take<char>(L.temp_bytes);
  L.total = c.off;
  return L;
}

// --------------------------------------------------------------------- csr --
// key = user in the high word, item in the low word; a code out of range takes the all-ones key, which sorts last
__global__ void __launch_bounds__(256) k_prep_pair_keys(const int32_t* __restrict__ ucode,
                                                        const int32_t* __restrict__ icode, int64_t n, int64_t n_users,
                                                        int64_t n_items, unsigned long long* __restrict__ key,
                                                        uint32_t* __restrict__ perm) {
  PREP_LOOP(i, n) {
    const int32_t u = ucode[i], t = icode[i];
    const bool ok = u >= 0 && u < n_users && t >= 0 && t < n_items;
    key[i] = ok ? ((unsigned long long)(uint32_t)u << 32) | (uint32_t)t : ~0ull;
    perm[i] = (uint32_t)i;
  }
}

__global__ void __launch_bounds__(256) k_prep_pair_heads(const unsigned long long* __restrict__ key_s, int64_t n,
                                                         uint32_t* __restrict__ head) {
  PREP_LOOP(i, n) head[i] = (key_s[i] != ~0ull && (i == 0 || key_s[i] != key_s[i - 1])) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_prep_zero64(unsigned long long* __restrict__ p, int64_t m) {
  PREP_LOOP(i, m) p[i] = 0;
}

// The head of a run of equal pairs writes the stored entry: its column and the sum of the run's values in input
// order (the sort is stable, so the run lists its records by ascending index), and counts one entry for its row.
__global__ void __launch_bounds__(256) k_prep_csr_emit(const unsigned long long* __restrict__ key_s,
                                                       const uint32_t* __restrict__ perm_s,
                                                       const uint32_t* __restrict__ head,
                                                       const uint32_t* __restrict__ seg,
                                                       const float* __restrict__ vals, int64_t n,
                                                       int32_t* __restrict__ col_idx, float* __restrict__ out_vals,
                                                       unsigned long long* __restrict__ row_len,
                                                       int64_t* __restrict__ nnz) {
  PREP_LOOP(i, n) {
    if (head[i]) {
      const unsigned long long k = key_s[i];
      float s = vals[perm_s[i]];
      for (int64_t j = i + 1; j < n && key_s[j] == k; ++j) s += vals[perm_s[j]];
      const int64_t e = (int64_t)seg[i] - 1;
      col_idx[e] = (int32_t)(uint32_t)(k & 0xffffffffull);
      out_vals[e] = s;
      atomicAdd(&row_len[k >> 32], 1ull);
    }
    if (i == n - 1) *nnz = (int64_t)seg[i];
  }
}

__global__ void k_prep_rowptr0(int64_t* __restrict__ row_ptr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) row_ptr[0] = 0;
}

struct CsrWs {
  unsigned long long *key, *key_s, *row_len;
  uint32_t *perm, *perm_s, *head, *seg;
  void* temp;
  size_t temp_bytes, total;
};
CsrWs csr_ws(void* ws, int64_t n, int64_t n_users) {
  Carve c(ws);
  CsrWs L{};
  L.key = c.take<unsigned long long>(n);
  L.key_s = c.take<unsigned long long>(n);
  L.row_len = c.take<unsigned long long>(n_users);
  L.perm = c.take<uint32_t>(n);
  L.perm_s = c.take<uint32_t>(n);
  L.head = c.take<uint32_t>(n);
  L.seg = c.take<uint32_t>(n);
  L.temp_bytes = std::max(std::max(sort64_temp(n), scan32_temp(n)), scan64_temp(n_users));
  L.temp = c.take<char>(L.temp_bytes);
  L.total = c.off;
  return L;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace
}  // namespace hvae

using namespace hvae;

extern "C" size_t hvae_prep_encode_workspace(int64_t n, int W) {
  if (n < 1 || n > kPrepMaxN || W < 1 || W > 4) return 0;
  return encode_ws(nullptr, n).total;
}

extern "C" int hvae_prep_encode(const uint64_t* keys, int64_t n, int W, int32_t* codes, int32_t* n_classes,
                                int32_t* first, void* ws, size_t ws_bytes, void* stream) {
  HVAE_REQUIRE(keys && codes && n_classes && first && ws, "hvae_prep_encode: null pointer");
  HVAE_REQUIRE(n >= 1 && n <= kPrepMaxN && W >= 1 && W <= 4, "hvae_prep_encode: 1 <= n <= 2^31 - 1 and 1 <= W <= 4");
  HVAE_REQUIRE(aligned8(keys) && (reinterpret_cast<uintptr_t>(ws) & 255) == 0,
               "hvae_prep_encode: keys must be 8-byte and the workspace 256-byte aligned");
  const EncodeWs L = encode_ws(ws, n);
  if (ws_bytes < L.total)
    HVAE_FAIL(HVAE_ERR_WORKSPACE, "hvae_prep_encode: workspace %zu < %zu bytes", ws_bytes, L.total);
  hipStream_t st = as_stream(stream);
  const unsigned g = grid_for(n);
  const unsigned long long* k64 = reinterpret_cast<const unsigned long long*>(keys);
  uint32_t *perm = L.perm, *perm_s = L.perm_s;
  k_prep_iota<<<g, 256, 0, st>>>(perm, n);
  HVAE_LAUNCH_CHECK("k_prep_iota");
  for (int w = W - 1; w >= 0; --w) {  // least significant word first; each pass is stable
    k_prep_gather_word<<<g, 256, 0, st>>>(k64, W, w, perm, n, L.kbuf);
    HVAE_LAUNCH_CHECK("k_prep_gather_word");
    size_t tb = L.temp_bytes;
    if (rocprim::radix_sort_pairs(L.temp, tb, L.kbuf, L.kbuf_s, perm, perm_s, (unsigned)n, 0, 64, st) != hipSuccess)
      HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_encode: radix sort failed");
    std::swap(perm, perm_s);
  }
  k_prep_key_heads<<<g, 256, 0, st>>>(k64, W, perm, n, L.head);
  HVAE_LAUNCH_CHECK("k_prep_key_heads");
  size_t tb = L.temp_bytes;
  if (rocprim::inclusive_scan(L.temp, tb, L.head, L.seg, (unsigned)n, rocprim::plus<unsigned>(), st) != hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_encode: scan failed");
  k_prep_encode_emit<<<g, 256, 0, st>>>(perm, L.head, L.seg, n, codes, first, n_classes);
  HVAE_LAUNCH_CHECK("k_prep_encode_emit");
  return HVAE_OK;
}

extern "C" size_t hvae_prep_kcore_workspace(int64_t n_users, int64_t n_items, int32_t max_iterations) {
  if (n_users < 1 || n_items < 1 || n_users > kPrepMaxN || n_items > kPrepMaxN || max_iterations < 0 ||
      max_iterations > 1 << 20)
    return 0;
  return kcore_ws(nullptr, n_users, n_items, max_iterations).total;
}

extern "C" int hvae_prep_kcore(const int32_t* ucode, const int32_t* icode, int64_t n, int64_t n_users, int64_t n_items,
                               int32_t min_user, int32_t min_item, int32_t max_iterations, uint8_t* alive,
                               int64_t* n_alive, int32_t* rounds, void* ws, size_t ws_bytes, void* stream) {
  HVAE_REQUIRE(ucode && icode && alive && n_alive && rounds && ws, "hvae_prep_kcore: null pointer");
  HVAE_REQUIRE(n >= 1 && n <= kPrepMaxN && n_users >= 1 && n_users <= kPrepMaxN && n_items >= 1 &&
                   n_items <= kPrepMaxN && max_iterations >= 0 && max_iterations <= 1 << 20,
               "hvae_prep_kcore: bad sizes (1 <= n, n_users, n_items <= 2^31 - 1; 0 <= max_iterations <= 2^20)");
  HVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && aligned8(n_alive),
               "hvae_prep_kcore: the workspace must be 256-byte and n_alive 8-byte aligned");
  const KcoreWs L = kcore_ws(ws, n_users, n_items, max_iterations);
  if (ws_bytes < L.total)
    HVAE_FAIL(HVAE_ERR_WORKSPACE, "hvae_prep_kcore: workspace %zu < %zu bytes", ws_bytes, L.total);
  hipStream_t st = as_stream(stream);
  const unsigned g = grid_for(n);
  HVAE_HIP(hipMemsetAsync(L.state, 0, L.state_words * sizeof(uint32_t), st));
  k_prep_kcore_init<<<g, 256, 0, st>>>(ucode, icode, n, n_users, n_items, alive, L.state);
  HVAE_LAUNCH_CHECK("k_prep_kcore_init");
  for (int r = 0; r < max_iterations; ++r) {
    k_prep_kcore_zero<<<grid_for(n_users), 256, 0, st>>>(L.ucnt, n_users, L.state, r);
    k_prep_kcore_hist<<<g, 256, 0, st>>>(ucode, alive, n, L.ucnt, L.state, r);
    k_prep_kcore_kill<<<g, 256, 0, st>>>(ucode, alive, n, L.ucnt, min_user, L.state, r);
    k_prep_kcore_zero<<<grid_for(n_items), 256, 0, st>>>(L.icnt, n_items, L.state, r);
    k_prep_kcore_hist<<<g, 256, 0, st>>>(icode, alive, n, L.icnt, L.state, r);
    k_prep_kcore_kill<<<g, 256, 0, st>>>(icode, alive, n, L.icnt, min_item, L.state, r);
    HVAE_LAUNCH_CHECK("k_prep_kcore round");
  }
  k_prep_kcore_finish<<<1, 64, 0, st>>>(L.state, max_iterations, n, n_alive, rounds);
  HVAE_LAUNCH_CHECK("k_prep_kcore_finish");
  return HVAE_OK;
}

extern "C" size_t hvae_prep_split_workspace(int64_t n) {
  if (n < 1 || n > kPrepMaxN) return 0;
  return split_ws(nullptr, n).total;
}

extern "C" int hvae_prep_split(const int32_t* ucode, const int64_t* ts, int64_t n, int64_t n_users, int32_t* perm,
                               int32_t* train_idx, int32_t* val_idx, int32_t* test_idx, int64_t* lens, void* ws,
                               size_t ws_bytes, void* stream) {
  HVAE_REQUIRE(ucode && ts && perm && train_idx && val_idx && test_idx && lens && ws, "hvae_prep_split: null pointer");
  HVAE_REQUIRE(n >= 1 && n <= kPrepMaxN && n_users >= 1 && n_users <= kPrepMaxN,
               "hvae_prep_split: 1 <= n, n_users <= 2^31 - 1");
  HVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && aligned8(ts) && aligned8(lens),
               "hvae_prep_split: the workspace must be 256-byte, ts and lens 8-byte aligned");
  const SplitWs L = split_ws(ws, n);
  if (ws_bytes < L.total)
    HVAE_FAIL(HVAE_ERR_WORKSPACE, "hvae_prep_split: workspace %zu < %zu bytes", ws_bytes, L.total);
  hipStream_t st = as_stream(stream);
  const unsigned g = grid_for(n);
  // stable sort by timestamp, then by user: (user, timestamp) order with ties in input order. A user code out of
  // range is only ever a sort key here (all 32 bits are sorted), never an index.
  k_prep_ts_keys<<<g, 256, 0, st>>>(ts, n, L.key, L.perm);
  HVAE_LAUNCH_CHECK("k_prep_ts_keys");
  size_t tb = L.temp_bytes;
  if (rocprim::radix_sort_pairs(L.temp, tb, L.key, L.key_s, L.perm, L.perm_s, (unsigned)n, 0, 64, st) != hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_split: timestamp sort failed");
  k_prep_gather_code<<<g, 256, 0, st>>>(ucode, L.perm_s, n, L.ukey);
  HVAE_LAUNCH_CHECK("k_prep_gather_code");
  tb = L.temp_bytes;
  if (rocprim::radix_sort_pairs(L.temp, tb, L.ukey, L.ukey_s, L.perm_s, L.perm, (unsigned)n, 0, 32, st) != hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_split: user sort failed");
  k_prep_split_flags<<<g, 256, 0, st>>>(L.ukey_s, n, L.flag);
  HVAE_LAUNCH_CHECK("k_prep_split_flags");
  tb = L.temp_bytes;
  if (rocprim::inclusive_scan(L.temp, tb, L.flag, L.incl, (unsigned)n, rocprim::plus<unsigned long long>(), st) !=
      hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_split: scan failed");
  k_prep_split_emit<<<g, 256, 0, st>>>(L.perm, L.flag, L.incl, n, perm, train_idx, val_idx, test_idx, lens);
  HVAE_LAUNCH_CHECK("k_prep_split_emit");
  return HVAE_OK;
}

extern "C" size_t hvae_prep_csr_workspace(int64_t n, int64_t n_users) {
  if (n < 1 || n > kPrepMaxN || n_users < 1 || n_users > kPrepMaxN) return 0;
  return csr_ws(nullptr, n, n_users).total;
}

extern "C" int hvae_prep_csr(const int32_t* ucode, const int32_t* icode, const float* vals, int64_t n, int64_t n_users,
                             int64_t n_items, int64_t* row_ptr, int32_t* col_idx, float* out_vals, int64_t* nnz,
                             void* ws, size_t ws_bytes, void* stream) {
  HVAE_REQUIRE(ucode && icode && vals && row_ptr && col_idx && out_vals && nnz && ws, "hvae_prep_csr: null pointer");
  HVAE_REQUIRE(n >= 1 && n <= kPrepMaxN && n_users >= 1 && n_users <= kPrepMaxN && n_items >= 1 && n_items <= kPrepMaxN,
               "hvae_prep_csr: 1 <= n, n_users, n_items <= 2^31 - 1");
  HVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && aligned8(row_ptr) && aligned8(nnz),
               "hvae_prep_csr: the workspace must be 256-byte, row_ptr and nnz 8-byte aligned");
  const CsrWs L = csr_ws(ws, n, n_users);
  if (ws_bytes < L.total)
    HVAE_FAIL(HVAE_ERR_WORKSPACE, "hvae_prep_csr: workspace %zu < %zu bytes", ws_bytes, L.total);
  hipStream_t st = as_stream(stream);
  const unsigned g = grid_for(n);
  k_prep_pair_keys<<<g, 256, 0, st>>>(ucode, icode, n, n_users, n_items, L.key, L.perm);
  HVAE_LAUNCH_CHECK("k_prep_pair_keys");
  size_t tb = L.temp_bytes;
  // all 64 bits: the key of a record with a code out of range is all ones
  if (rocprim::radix_sort_pairs(L.temp, tb, L.key, L.key_s, L.perm, L.perm_s, (unsigned)n, 0, 64, st) != hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_csr: radix sort failed");
  k_prep_pair_heads<<<g, 256, 0, st>>>(L.key_s, n, L.head);
  HVAE_LAUNCH_CHECK("k_prep_pair_heads");
  tb = L.temp_bytes;
  if (rocprim::inclusive_scan(L.temp, tb, L.head, L.seg, (unsigned)n, rocprim::plus<unsigned>(), st) != hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_csr: scan failed");
  k_prep_zero64<<<grid_for(n_users), 256, 0, st>>>(L.row_len, n_users);
  HVAE_LAUNCH_CHECK("k_prep_zero64");
  k_prep_csr_emit<<<g, 256, 0, st>>>(L.key_s, L.perm_s, L.head, L.seg, vals, n, col_idx, out_vals, L.row_len, nnz);
  HVAE_LAUNCH_CHECK("k_prep_csr_emit");
  k_prep_rowptr0<<<1, 64, 0, st>>>(row_ptr);
  HVAE_LAUNCH_CHECK("k_prep_rowptr0");
  tb = L.temp_bytes;
  if (rocprim::inclusive_scan(L.temp, tb, L.row_len, reinterpret_cast<unsigned long long*>(row_ptr + 1),
                              (unsigned)n_users, rocprim::plus<unsigned long long>(), st) != hipSuccess)
    HVAE_FAIL(HVAE_ERR_HIP, "hvae_prep_csr: row scan failed");
  return HVAE_OK;
}
