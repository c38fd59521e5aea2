// hvae_svd.hip -- the SVD baseline's tall-skinny fp64 linear algebra (K19).
//
// Reference: SVDRecommender (src/ml/baseline.py:102-118), scikit-learn's randomized TruncatedSVD: a subspace
// iteration Q <- orth(M Q), Q <- orth(M^T Q) over the sparse interaction matrix M and a sketch of W = k + 10 columns.
// Here a tall matrix is [n, HVAE_SVD_LD] doubles row-major with W live columns; the columns from W up are written as
// zeros and never read as data. The four kernels are the product with the sparse matrix (k_svd_spmm, from the CSR for
// M X and from the CSC for M^T X), the Gram matrix Y^T Y (k_svd_gram and its reduction), the Cholesky factor's
// inverse (k_svd_chol_inv) and the product with a small matrix (k_svd_apply): CholeskyQR2 is gram -> chol_inv ->
// apply, twice.
//
// Everything is fp64 in plain FMAs (the products here are a few hundred MFLOP in all, bounded by launches and the
// gathered reads, not by the FMA rate) with no atomics; every sum has one fixed order that depends on the shapes
// only, so two runs are bitwise equal.
//
// An spmm row is a gathered row sum of hvae_rowgather.h, whose first comment states its summation order: lane l owns
// column l, so a gathered row of X is one coalesced 512-byte read.
#include "hvae_rowgather.h"

namespace hvae {

constexpr int kSvdLd = HVAE_SVD_LD;
constexpr int kApplyRows = 4;       // apply rows per 256-thread block: one wave each
constexpr int kGramRows = 32;       // rows of Y staged per step of a gram block
constexpr int kGramMaxBlocks = 256; // partial Gram matrices at the most
static_assert(kSvdLd == 64, "one lane per column");

// out[r, lane] = sum_p double(vals[p]) x[idx[p], lane] over row r's entries; an index outside [0, n_cols) (a broken
// matrix) reads row 0 with a NaN weight instead of reading out of bounds. Lanes from W up read nothing and write 0.
__global__ void __launch_bounds__(256) k_svd_spmm(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                  const float* __restrict__ vals, int64_t n_rows, int64_t n_cols,
                                                  const double* __restrict__ x,
                                                  double* __restrict__ out, int W) {
  using Row = RowVec<double, 1>;
  const int lane = threadIdx.x & 63;
  gather_rows<double, 1>(
      n_rows, lane < W,
      [&](int64_t r, int64_t& p0, int64_t& p1) {
        p0 = ptr[r];
        p1 = ptr[r + 1];
        return [&](int64_t p) {
          const int64_t j = idx[p];
          return j >= 0 && j < n_cols ? GatherEntry<double>{(int)j, (double)vals[p]} : GatherEntry<double>{0, NAN};
        };
      },
      [&](int j) { return ld_row<double, 1>(x, j, lane); },
      [&](int64_t r, const Row& s) { out[r * kSvdLd + lane] = s.v[0]; });
}

// ---- Gram ------------------------------------------------------------------------------------------------
// Block b sums y_r^T y_r over the row chunks b, b + gridDim.x, ... (kGramRows rows each, ascending) into its own
// [64, 64] partial; thread (ti, tj) of the 16 x 16 block owns the 4 x 4 tile at (4 ti, 4 tj) and adds the rows in
// order with one fma per entry. Entry (i, j) and entry (j, i) are the same chain of fma(y_i, y_j, .) in the same
// order, so every partial, and the sum of the partials in block order, is exactly symmetric.
__global__ void __launch_bounds__(256) k_svd_gram(const double* __restrict__ Y, int64_t n, int W,
                                                  double* __restrict__ part) {
  __shared__ double tile[kGramRows][kSvdLd];
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[4][4] = {};
  const int64_t n_chunks = (n + kGramRows - 1) / kGramRows;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * kGramRows;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < kGramRows / 4; ++rr) {
      const int row = rr * 4 + wave;
      const int64_t r = base + row;
      tile[row][lane] = (r < n && lane < W) ? Y[r * kSvdLd + lane] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int row = 0; row < kGramRows; ++row) {
      double yi[4], yj[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        yi[v] = tile[row][4 * ti + v];
        yj[v] = tile[row][4 * tj + v];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(yi[u], yj[v], acc[u][v]);
    }
  }
  double* p = part + (int64_t)blockIdx.x * kSvdLd * kSvdLd;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) p[(4 * ti + u) * kSvdLd + 4 * tj + v] = acc[u][v];
}

__global__ void __launch_bounds__(256) k_svd_gram_sum(const double* __restrict__ part, int n_part,
                                                      double* __restrict__ G) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // 16 blocks: the 4096 entries
  double s = 0.0;
  for (int b = 0; b < n_part; ++b) s += part[(int64_t)b * kSvdLd * kSvdLd + e];
  G[e] = s;
}

// ---- Cholesky and the factor's inverse ---------------------------------------------------------------------
// One 256-thread block. G = L L^T (R = L^T) by the right-looking algorithm in LDS: per column k the pivot's square
// root, the column's division, then the trailing update a[i][j] -= a[i][k] a[j][k] over the lower triangle. A pivot
// that is NaN or not above kSvdLd 2^-53 times its own diagonal entry of G (the size of the rounding error it carries:
// such a pivot cannot be told from zero) sets *flag; the arithmetic goes on and leaves NaN or noise. Then column j of
// L^-1 by forward substitution, one thread per column: entry (i, j), i > j, is kept at a[j][i], in the upper triangle
// that L leaves free, and the diagonal 1 / L[j][j] in invd, so that R^-1 = (L^-1)^T is the upper triangle as it
// stands.
__global__ void __launch_bounds__(256) k_svd_chol_inv(const double* __restrict__ G, int W, double* __restrict__ Rinv,
                                                      int32_t* __restrict__ flag) {
  __shared__ double a[kSvdLd][kSvdLd + 1];
  __shared__ double invd[kSvdLd];
  __shared__ int bad;
  const int t = threadIdx.x;
  if (t == 0) bad = 0;
  for (int e = t; e < kSvdLd * kSvdLd; e += 256) {
    const int i = e >> 6, j = e & 63;
    a[i][j] = (i < W && j < W) ? G[e] : 0.0;
  }
  __syncthreads();
  for (int k = 0; k < W; ++k) {
    if (t == 0) {
      const double piv = a[k][k];
      if (!(piv > (double)kSvdLd * 0x1p-53 * G[k * kSvdLd + k])) bad = 1;
      a[k][k] = sqrt(piv);
    }
    __syncthreads();
    const double d = a[k][k];
    if (t > k && t < W) a[t][k] = a[t][k] / d;
    __syncthreads();
    const int m = W - 1 - k;  // the trailing block is m x m; its lower triangle is updated
    for (int e = t; e < m * m; e += 256) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) a[i][j] = fma(-a[i][k], a[j][k], a[i][j]);
    }
    __syncthreads();
  }
  if (t < W) {
    const int j = t;
    const double dj = 1.0 / a[j][j];
    invd[j] = dj;
    for (int i = j + 1; i < W; ++i) {
      double s = a[i][j] * dj;
      for (int u = j + 1; u < i; ++u) s = fma(a[i][u], a[j][u], s);
      a[j][i] = -s / a[i][i];
    }
  }
  __syncthreads();
  for (int e = t; e < kSvdLd * kSvdLd; e += 256) {
    const int i = e >> 6, j = e & 63;
    Rinv[e] = (j < W && i <= j) ? (i == j ? invd[i] : a[i][j]) : 0.0;
  }
  if (t == 0 && bad) *flag = 1;
}

// ---- apply -------------------------------------------------------------------------------------------------
// out[r, c] = sum_{t < W} Y[r, t] T[t, c] for c < W_out, t ascending, one fma each; 0 for c >= W_out. A wave owns a
// row and reads all of it before it writes, so out may be Y.
__global__ void __launch_bounds__(256) k_svd_apply(const double* Y, int64_t n, int W, const double* __restrict__ T,
                                                   int W_out, double* out) {
  __shared__ double tm[kSvdLd][kSvdLd];
  __shared__ double yrow[kApplyRows][kSvdLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < kSvdLd * kSvdLd; e += 256) {
    const int i = e >> 6, j = e & 63;
    tm[i][j] = (i < W && j < W_out) ? T[e] : 0.0;
  }
  const int64_t n_groups = (n + kApplyRows - 1) / kApplyRows;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {  // the same trip count in every wave of the block
    const int64_t r = g * kApplyRows + wave;
    __syncthreads();
    yrow[wave][lane] = (r < n && lane < W) ? Y[r * kSvdLd + lane] : 0.0;
    __syncthreads();
    double s = 0.0;
    for (int t = 0; t < W; ++t) s = fma(yrow[wave][t], tm[t][lane], s);
    if (r < n) out[r * kSvdLd + lane] = s;
  }
}

static int gram_blocks(int64_t n) {
  const int64_t chunks = cdiv(n, kGramRows);
  return (int)(chunks < kGramMaxBlocks ? chunks : kGramMaxBlocks);
}

}  // namespace hvae

using namespace hvae;

static bool svd_w_ok(int64_t W) { return W >= 1 && W <= HVAE_SVD_LD; }

extern "C" int hvae_svd_spmm(const int64_t* ptr, const int32_t* idx, const float* vals, int64_t n_rows,
                             int64_t n_cols, const double* X, double* out, int64_t W, void* stream) {
  HVAE_REQUIRE(n_rows > 0 && n_cols > 0 && n_rows < INT32_MAX && n_cols < INT32_MAX, "hvae_svd_spmm: bad args");
  HVAE_REQUIRE(svd_w_ok(W), "hvae_svd_spmm: W = %lld is not served (1 to %d)", (long long)W, HVAE_SVD_LD);
  HVAE_REQUIRE(ptr && idx && vals && X && out, "hvae_svd_spmm: null pointer");
  HVAE_REQUIRE(X != out, "hvae_svd_spmm: out may not alias X");
  k_svd_spmm<<<(unsigned)cdiv(n_rows, kGatherRows), 256, 0, as_stream(stream)>>>(ptr, idx, vals, n_rows, n_cols, X,
                                                                                 out, (int)W);
  HVAE_LAUNCH_CHECK("k_svd_spmm");
  return HVAE_OK;
}

extern "C" size_t hvae_svd_gram_workspace(int64_t n) {
  if (n <= 0) return 0;
  return (size_t)gram_blocks(n) * HVAE_SVD_LD * HVAE_SVD_LD * sizeof(double);
}

extern "C" int hvae_svd_gram(const double* Y, int64_t n, int64_t W, double* G, void* ws, size_t ws_bytes,
                             void* stream) {
  HVAE_REQUIRE(n > 0, "hvae_svd_gram: bad args");
  HVAE_REQUIRE(svd_w_ok(W), "hvae_svd_gram: W = %lld is not served (1 to %d)", (long long)W, HVAE_SVD_LD);
  HVAE_REQUIRE(Y && G && ws, "hvae_svd_gram: null pointer");
  HVAE_REQUIRE(ws_bytes >= hvae_svd_gram_workspace(n), "hvae_svd_gram: ws holds %zu bytes, needs %zu", ws_bytes,
               hvae_svd_gram_workspace(n));
  HVAE_REQUIRE(((uintptr_t)ws & 7) == 0, "hvae_svd_gram: ws must be 8-byte aligned");
  const int nb = gram_blocks(n);
  hipStream_t st = as_stream(stream);
  k_svd_gram<<<nb, 256, 0, st>>>(Y, n, (int)W, (double*)ws);
  HVAE_LAUNCH_CHECK("k_svd_gram");
  k_svd_gram_sum<<<kSvdLd * kSvdLd / 256, 256, 0, st>>>((const double*)ws, nb, G);
  HVAE_LAUNCH_CHECK("k_svd_gram_sum");
  return HVAE_OK;
}

extern "C" int hvae_svd_chol_inv(const double* G, int64_t W, double* Rinv, int32_t* flag, void* stream) {
  HVAE_REQUIRE(svd_w_ok(W), "hvae_svd_chol_inv: W = %lld is not served (1 to %d)", (long long)W, HVAE_SVD_LD);
  HVAE_REQUIRE(G && Rinv && flag, "hvae_svd_chol_inv: null pointer");
  HVAE_REQUIRE(G != Rinv, "hvae_svd_chol_inv: Rinv may not alias G");
  k_svd_chol_inv<<<1, 256, 0, as_stream(stream)>>>(G, (int)W, Rinv, flag);
  HVAE_LAUNCH_CHECK("k_svd_chol_inv");
  return HVAE_OK;
}

extern "C" int hvae_svd_apply(const double* Y, int64_t n, int64_t W, const double* T, int64_t W_out, double* out,
                              void* stream) {
  HVAE_REQUIRE(n > 0, "hvae_svd_apply: bad args");
  HVAE_REQUIRE(svd_w_ok(W) && svd_w_ok(W_out), "hvae_svd_apply: W = %lld, W_out = %lld are not served (1 to %d)",
               (long long)W, (long long)W_out, HVAE_SVD_LD);
  HVAE_REQUIRE(Y && T && out, "hvae_svd_apply: null pointer");
  HVAE_REQUIRE(T != Y && T != out, "hvae_svd_apply: T may not alias Y or out");
  const int64_t groups = cdiv(n, kApplyRows);
  const unsigned grid = (unsigned)(groups < 1024 ? groups : 1024);
  k_svd_apply<<<grid, 256, 0, as_stream(stream)>>>(Y, n, (int)W, T, (int)W_out, out);
  HVAE_LAUNCH_CHECK("k_svd_apply");
  return HVAE_OK;
}
