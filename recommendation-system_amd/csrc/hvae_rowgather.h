// hvae_rowgather.h -- a sparse row's weighted sum of gathered dense rows, out[r] = f(sum_p w_p x[j_p]), in one fixed
// order. k_svd_spmm (hvae_svd.hip, double, one column per lane) and k_lgcn_propagate (hvae_lgcn.hip, float, V columns
// per lane) are instantiations; "two runs are bitwise equal" in both files rests on the paragraph below.
//
// Summation order of a gathered row. A wave owns the row, lane l owns columns [l V, l V + V), so a gathered row of x is
// one coalesced read. The entries are walked in storage order in chunks of 64 (lane l fetches index and weight of
// entry l, then they are broadcast); within a chunk entry k goes to accumulator k mod 4 while four entries are left and
// to accumulator 0 after that, one fma each; the row sum is (a0 + a1) + (a2 + a3). A row longer than kGatherSplit is
// cut into four contiguous quarters, one per wave of the block, each summed as above, and merged
// ((q0 + q1) + q2) + q3 through LDS.
//
// A kernel calls gather_rows with live, whether the lane's columns exist (a lane that is not live loads nothing and
// its sum is 0), and three functions:
//   row(r, p0, p1)  sets the extent [p0, p1) of row r's entries and returns its entry reader, entry(p) -> GatherEntry:
//                   the index of the dense row and the weight, or, for an index out of range (a broken matrix), a
//                   row that is safe to read with a NaN weight;
//   load(j)         the lane's part of dense row j;
//   finish(r, s)    what becomes of row r's sum (called by one wave, every lane).
#pragma once
#include "hvae_common.h"

namespace hvae {

constexpr int kGatherRows = 4;       // rows per 256-thread block: one wave each
constexpr int kGatherSplit = 256;    // entries above which the block's four waves share one row

// A lane's V consecutive columns of a row of 64 V.
template <typename T, int V>
struct RowVec {
  static_assert(V == 1 || (V == 2 && sizeof(T) == 4), "one element or one 8-byte pair per lane");
  T v[V];
};
template <typename T, int V>
__device__ __forceinline__ RowVec<T, V> ld_row(const T* __restrict__ t, int64_t row, int lane) {
  RowVec<T, V> r;
  const T* p = t + row * (64 * V) + lane * V;
  if constexpr (V == 2) {
    const float2 x = *reinterpret_cast<const float2*>(p);
    r.v[0] = x.x;
    r.v[1] = x.y;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <typename T, int V>
__device__ __forceinline__ void st_row(T* __restrict__ t, int64_t row, int lane, const RowVec<T, V>& r) {
  T* p = t + row * (64 * V) + lane * V;
  if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  else *p = r.v[0];
}
template <typename T, int V>
__device__ __forceinline__ void fma_row(RowVec<T, V>& acc, T w, const RowVec<T, V>& x) {
#pragma unroll
  for (int v = 0; v < V; ++v) acc.v[v] = fma(w, x.v[v], acc.v[v]);
}

// lane k's value in every lane (k wave-uniform)
__device__ __forceinline__ float bcast(float x, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k));
}
__device__ __forceinline__ double bcast(double x, int k) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), k);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <typename T>
struct GatherEntry {
  int j;
  T w;
};

// sum_{p in [p0, p1)} entry(p).w * load(entry(p).j) for one wave, in the order above.
template <typename T, int V, typename Entry, typename Load>
__device__ __forceinline__ RowVec<T, V> gather_span(int64_t p0, int64_t p1, int lane, bool live, Entry entry,
                                                    Load load) {
  const RowVec<T, V> zero = {};
  RowVec<T, V> a[4] = {};
  for (int64_t base = p0; base < p1; base += 64) {
    const int cnt = (int)(p1 - base < 64 ? p1 - base : 64);
    GatherEntry<T> e = {0, (T)0};  // lanes from cnt up are never broadcast
    if (lane < cnt) e = entry(base + lane);
    int k = 0;
    for (; k + 4 <= cnt; k += 4) {
      const int j0 = __builtin_amdgcn_readlane(e.j, k), j1 = __builtin_amdgcn_readlane(e.j, k + 1);
      const int j2 = __builtin_amdgcn_readlane(e.j, k + 2), j3 = __builtin_amdgcn_readlane(e.j, k + 3);
      const RowVec<T, V> x0 = live ? load(j0) : zero, x1 = live ? load(j1) : zero;
      const RowVec<T, V> x2 = live ? load(j2) : zero, x3 = live ? load(j3) : zero;
      fma_row<T, V>(a[0], bcast(e.w, k), x0);
      fma_row<T, V>(a[1], bcast(e.w, k + 1), x1);
      fma_row<T, V>(a[2], bcast(e.w, k + 2), x2);
      fma_row<T, V>(a[3], bcast(e.w, k + 3), x3);
    }
    for (; k < cnt; ++k) {
      const int j = __builtin_amdgcn_readlane(e.j, k);
      fma_row<T, V>(a[0], bcast(e.w, k), live ? load(j) : zero);
    }
  }
  RowVec<T, V> s;
#pragma unroll
  for (int v = 0; v < V; ++v) s.v[v] = live ? (a[0].v[v] + a[1].v[v]) + (a[2].v[v] + a[3].v[v]) : (T)0;
  return s;
}

// The body of a 256-thread block over rows [blockIdx.x kGatherRows, ...) of n_rows; grid = cdiv(n_rows, kGatherRows).
template <typename T, int V, typename Row, typename Load, typename Finish>
__device__ __forceinline__ void gather_rows(int64_t n_rows, bool live, Row row, Load load, Finish finish) {
  __shared__ T part[kGatherRows][64 * V];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t r0 = (int64_t)blockIdx.x * kGatherRows;
  for (int q = 0; q < kGatherRows; ++q) {  // every wave looks at the block's rows: a long one is shared
    const int64_t r = r0 + q;
    if (r >= n_rows) break;
    int64_t p0, p1;
    const auto entry = row(r, p0, p1);
    const int64_t deg = p1 - p0;
    const bool split = deg > kGatherSplit;  // the same in every wave of the block
    if (!split && q != wave) continue;
    int64_t a = p0, b = p1;
    if (split) {
      const int64_t per = (deg + kGatherRows - 1) / kGatherRows;
      a = p0 + wave * per;
      if (a > p1) a = p1;
      b = a + per < p1 ? a + per : p1;
    }
    RowVec<T, V> s = gather_span<T, V>(a, b, lane, live, entry, load);
    if (split) {
#pragma unroll
      for (int v = 0; v < V; ++v) part[wave][lane * V + v] = s.v[v];
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const int c = lane * V + v;
          s.v[v] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
        }
      }
      __syncthreads();
      if (wave != 0) continue;
    }
    finish(r, s);
  }
}

}  // namespace hvae
