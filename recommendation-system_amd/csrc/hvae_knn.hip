// hvae_knn.hip -- scoring of the training-free baselines: Popularity and Item-KNN (K17).
//
// Reference: PopularityRecommender / ItemKNNRecommender (src/ml/baseline.py:57-99). Popularity scores are the
// column sums of the train+val matrix M. Item-KNN scores one user at a time: above 10,000 items it calls
// cosine_similarity(item_matrix, item_matrix[interacted]).sum(axis=1) over the whole catalogue per test row
// (:97-99), below it sums columns of a dense N x N similarity with a zeroed diagonal (:84-95).
//
// Here, with c_j the columns of M, I_u the nonzero structure of row u and Nn = M diag(1 / ||c||):
//   score[u, j] = inv_norm[j] * sum_{v in col j} M[v, j] * T[u, v],   T[u, v] = sum_{i in I_u} M[v, i] * inv_norm[i]
// so a batch of users costs one sparse scatter (stage 1, T = Nn b) and one sparse gather per scored item
// (stage 2), instead of a dense N x |I_u| product per row. Every sum is in double, in a fixed order (items and
// users ascending), rounded to fp32 once; there are no atomics, so two runs are bitwise equal and the candidate
// kernel and the all-items kernel give the same bits for the same (user, item).
//
// T is user-major with the batch contiguous (T[v * nb + b]): stage 2 reads, per entry of a column, the nb
// doubles of one user -- 512 contiguous bytes per wave.
#include "hvae_common.h"

namespace hvae {

// One thread per item column: the popularity score (fp32 sum, exact for counts) and 1 / ||c_j|| in double
// (0 for an empty column, as sklearn's normalize leaves a zero vector).
__global__ void __launch_bounds__(256) k_csc_col_stats(const int64_t* __restrict__ col_ptr,
                                                       const float* __restrict__ vals, int64_t N,
                                                       float* __restrict__ col_sum, double* __restrict__ inv_norm) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  float s = 0.f;
  double q = 0.0;
  for (int64_t p = col_ptr[j]; p < col_ptr[j + 1]; ++p) {
    const float x = vals[p];
    s += x;
    q += (double)x * (double)x;
  }
  if (col_sum) col_sum[j] = s;
  if (inv_norm) inv_norm[j] = q > 0.0 ? 1.0 / sqrt(q) : 0.0;
}

// Stage 1. One workgroup per batch row; the row's items in ascending order, the lanes over the entries of the
// item's column. The users of one column are distinct, so the lanes of one item never meet; the barrier orders
// the items, which fixes the order of every T[b, v] sum.
__global__ void __launch_bounds__(256) k_knn_user_weights(const int64_t* __restrict__ row_ptr,
                                                          const int32_t* __restrict__ col_idx,
                                                          const float* __restrict__ row_vals,
                                                          const int32_t* __restrict__ rows,
                                                          const int64_t* __restrict__ rows_offset, int64_t nb,
                                                          int64_t n_users, int64_t n_items,
                                                          const int64_t* __restrict__ col_ptr,
                                                          const int32_t* __restrict__ row_idx,
                                                          const float* __restrict__ vals,
                                                          const double* __restrict__ inv_norm, double* T) {
  const int64_t b = blockIdx.x;
  const int64_t u = batch_row(rows, rows_offset, b);
  if (u < 0 || u >= n_users) return;  // uniform per block
  for (int64_t e = row_ptr[u]; e < row_ptr[u + 1]; ++e) {
    const int64_t i = col_idx[e];
    if (row_vals[e] == 0.f || i < 0 || i >= n_items) continue;  // structure only: nonzero()
    const double w = inv_norm[i];
    if (w != 0.0) {
      for (int64_t p = col_ptr[i] + threadIdx.x; p < col_ptr[i + 1]; p += 256) {
        const int64_t v = row_idx[p];
        if (v >= 0 && v < n_users) T[v * nb + b] += (double)vals[p] * w;
      }
    }
    __syncthreads();
  }
}

// 1 when item j is in the nonzero structure of CSR row u (col_idx ascending within a row).
__device__ __forceinline__ bool row_has(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx,
                                        const float* __restrict__ row_vals, int64_t u, int64_t j) {
  int64_t lo = row_ptr[u], hi = row_ptr[u + 1];
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col_idx[mid] < j) lo = mid + 1; else hi = mid;
  }
  return lo < row_ptr[u + 1] && col_idx[lo] == j && row_vals[lo] != 0.f;
}

// The stage-2 sum of one (batch row, item): users ascending, double.
__device__ __forceinline__ double knn_dot(const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row_idx,
                                          const float* __restrict__ vals, const double* __restrict__ T,
                                          int64_t nb, int64_t b, int64_t j) {
  double acc = 0.0;
  for (int64_t p = col_ptr[j]; p < col_ptr[j + 1]; ++p) acc += (double)vals[p] * T[(int64_t)row_idx[p] * nb + b];
  return acc;
}

// Stage 2a. One thread per (batch row, candidate).
__global__ void __launch_bounds__(256) k_knn_score_candidates(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx, const float* __restrict__ row_vals,
    const int32_t* __restrict__ rows, const int64_t* __restrict__ rows_offset, int64_t nb, int64_t n_users,
    int64_t n_items, const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row_idx,
    const float* __restrict__ vals, const double* __restrict__ inv_norm, const double* __restrict__ T,
    const int32_t* __restrict__ cand, int64_t C, int zero_diag, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nb * C) return;
  const int64_t b = t / C;
  const int64_t j = cand[t];
  const int64_t u = batch_row(rows, rows_offset, b);
  if (j < 0 || j >= n_items || u < 0 || u >= n_users) { out[t] = NAN; return; }  // a caller's bug, made visible
  double s = inv_norm[j] * knn_dot(col_ptr, row_idx, vals, T, nb, b, j);
  if (zero_diag && inv_norm[j] != 0.0 && row_has(row_ptr, col_idx, row_vals, u, j)) s -= 1.0;
  out[t] = (float)s;
}

// Stage 2b. A workgroup takes kJT items x 256 batch rows: a thread owns one batch row, walks each of the
// items' columns once (the column's entries are the same address for every lane, the T reads are 512
// contiguous bytes per wave) and the tile goes through LDS so that the [B, ld] output is written kJT
// contiguous floats at a time.
constexpr int kJT = 16;
__global__ void __launch_bounds__(256) k_knn_scores(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx, const float* __restrict__ row_vals,
    const int32_t* __restrict__ rows, const int64_t* __restrict__ rows_offset, int64_t nb, int64_t n_users,
    int64_t n_items, const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ row_idx,
    const float* __restrict__ vals, const double* __restrict__ inv_norm, const double* __restrict__ T,
    int zero_diag, float* __restrict__ out, int64_t ld) {
  __shared__ float tile[kJT][257];
  const int64_t j0 = (int64_t)blockIdx.x * kJT;
  const int64_t b0 = (int64_t)blockIdx.y * 256;
  const int64_t b = b0 + threadIdx.x;
  const int nj = (int)(n_items - j0 < kJT ? n_items - j0 : kJT);
  if (b < nb) {
    const int64_t u = batch_row(rows, rows_offset, b);
    const bool ok = u >= 0 && u < n_users;
    for (int jj = 0; jj < nj; ++jj) {
      const int64_t j = j0 + jj;
      const double w = inv_norm[j];
      double s = w * knn_dot(col_ptr, row_idx, vals, T, nb, b, j);
      if (zero_diag && w != 0.0 && ok && row_has(row_ptr, col_idx, row_vals, u, j)) s -= 1.0;
      tile[jj][threadIdx.x] = ok ? (float)s : NAN;
    }
  }
  __syncthreads();
  const int64_t nbt = nb - b0 < 256 ? nb - b0 : 256;
  for (int64_t k = threadIdx.x; k < nbt * nj; k += 256) {
    const int64_t bb = k / nj, jj = k - bb * nj;
    out[(b0 + bb) * ld + j0 + jj] = tile[jj][bb];
  }
}

}  // namespace hvae

using namespace hvae;

extern "C" int hvae_csc_col_stats(const int64_t* col_ptr, const int32_t* row_idx, const float* vals,
                                  int64_t n_items, float* col_sum, double* inv_norm, void* stream) {
  (void)row_idx;
  HVAE_REQUIRE(n_items >= 0, "hvae_csc_col_stats: bad args");
  if (n_items == 0) return HVAE_OK;
  HVAE_REQUIRE(col_ptr && vals && (col_sum || inv_norm), "hvae_csc_col_stats: null pointer");
  k_csc_col_stats<<<(unsigned)cdiv(n_items, 256), 256, 0, as_stream(stream)>>>(col_ptr, vals, n_items, col_sum,
                                                                               inv_norm);
  HVAE_LAUNCH_CHECK("k_csc_col_stats");
  return HVAE_OK;
}

extern "C" size_t hvae_knn_workspace(int64_t nb, int64_t n_users) {
  if (nb <= 0 || n_users <= 0) return 0;
  return (size_t)nb * (size_t)n_users * sizeof(double);
}

static int knn_check(const char* who, const hvae_csr_batch* x, const int64_t* col_ptr, const int32_t* row_idx,
                     const float* vals, const double* inv_norm, int64_t n_users, const double* T, size_t t_bytes) {
  HVAE_REQUIRE(x && x->nb >= 0 && x->n_items > 0 && n_users > 0 && x->nb < INT32_MAX && x->n_items < INT32_MAX,
               "%s: bad args", who);
  if (x->nb == 0) return HVAE_OK;
  HVAE_REQUIRE(x->row_ptr && x->col_idx && x->vals && col_ptr && row_idx && vals && inv_norm && T,
               "%s: null pointer", who);
  HVAE_REQUIRE(t_bytes >= hvae_knn_workspace(x->nb, n_users), "%s: T holds %zu bytes, needs %zu", who, t_bytes,
               hvae_knn_workspace(x->nb, n_users));
  return HVAE_OK;
}

extern "C" int hvae_knn_user_weights(const hvae_csr_batch* x, const int64_t* col_ptr, const int32_t* row_idx,
                                     const float* vals, const double* inv_norm, int64_t n_users, double* T,
                                     size_t t_bytes, void* stream) {
  const int rc = knn_check("hvae_knn_user_weights", x, col_ptr, row_idx, vals, inv_norm, n_users, T, t_bytes);
  if (rc != HVAE_OK || x->nb == 0) return rc;
  hipStream_t st = as_stream(stream);
  HVAE_HIP(hipMemsetAsync(T, 0, hvae_knn_workspace(x->nb, n_users), st));
  k_knn_user_weights<<<(unsigned)x->nb, 256, 0, st>>>(x->row_ptr, x->col_idx, x->vals, x->rows, x->rows_offset,
                                                      x->nb, n_users, x->n_items, col_ptr, row_idx, vals,
                                                      inv_norm, T);
  HVAE_LAUNCH_CHECK("k_knn_user_weights");
  return HVAE_OK;
}

extern "C" int hvae_knn_score_candidates(const hvae_csr_batch* x, const int64_t* col_ptr, const int32_t* row_idx,
                                         const float* vals, const double* inv_norm, int64_t n_users,
                                         const double* T, size_t t_bytes, const int32_t* cand, int64_t C,
                                         int zero_diag, float* out, void* stream) {
  const int rc = knn_check("hvae_knn_score_candidates", x, col_ptr, row_idx, vals, inv_norm, n_users, T, t_bytes);
  if (rc != HVAE_OK || x->nb == 0) return rc;
  HVAE_REQUIRE(C > 0 && cdiv(x->nb * C, 256) < INT32_MAX, "hvae_knn_score_candidates: bad C");
  HVAE_REQUIRE(cand && out, "hvae_knn_score_candidates: null pointer");
  k_knn_score_candidates<<<(unsigned)cdiv(x->nb * C, 256), 256, 0, as_stream(stream)>>>(
      x->row_ptr, x->col_idx, x->vals, x->rows, x->rows_offset, x->nb, n_users, x->n_items, col_ptr, row_idx, vals,
      inv_norm, T, cand, C, zero_diag, out);
  HVAE_LAUNCH_CHECK("k_knn_score_candidates");
  return HVAE_OK;
}

extern "C" int hvae_knn_scores(const hvae_csr_batch* x, const int64_t* col_ptr, const int32_t* row_idx,
                               const float* vals, const double* inv_norm, int64_t n_users, const double* T,
                               size_t t_bytes, int zero_diag, float* out, int64_t ld, void* stream) {
  const int rc = knn_check("hvae_knn_scores", x, col_ptr, row_idx, vals, inv_norm, n_users, T, t_bytes);
  if (rc != HVAE_OK || x->nb == 0) return rc;
  HVAE_REQUIRE(out && ld >= x->n_items, "hvae_knn_scores: bad out / ld");
  HVAE_REQUIRE(cdiv(x->nb, 256) <= 65535, "hvae_knn_scores: nb %lld exceeds 65535 * 256", (long long)x->nb);
  const dim3 grid((unsigned)cdiv(x->n_items, kJT), (unsigned)cdiv(x->nb, 256));
  k_knn_scores<<<grid, 256, 0, as_stream(stream)>>>(x->row_ptr, x->col_idx, x->vals, x->rows, x->rows_offset, x->nb,
                                                    n_users, x->n_items, col_ptr, row_idx, vals, inv_norm, T,
                                                    zero_diag, out, ld);
  HVAE_LAUNCH_CHECK("k_knn_scores");
  return HVAE_OK;
}
