// hvae_tsne.hip -- exact t-SNE of a few thousand latent vectors in fp64 (K21).
//
// Reference: plot_latent_space (src/ml/visualize.py:163-289) runs scikit-learn's TSNE(n_components=2, perplexity=30,
// max_iter=1000, random_state=42): Barnes-Hut in fp32 on host threads. Here the same algorithm (the k nearest
// neighbours, the per-row binary search for the perplexity, the gradient descent with gains and momentum) runs with
// the exact O(n^2) repulsion -- the angle = 0 limit of the tree -- and with every quantity in fp64. n is at most
// HVAE_TSNE_MAX_N, so a force evaluation is at most 2.7e8 pair terms.
//
// No atomics; every sum has one fixed order that depends on the shapes only (stated beside each kernel), so two fits
// of the same input are bitwise equal. The symmetrisation of P between hvae_tsne_perplexity and hvae_tsne_forces is
// the fit's one host step (src/ml/visualize.py).
//
// wave_sum_d is the xor butterfly over offsets 32, 16, 8, 4, 2, 1: lanes a and a ^ o add the same two numbers, so
// after every level both hold the same bits and the final sum is one value in all 64 lanes.
#include "hvae_common.h"

#include <float.h>

namespace hvae {

constexpr int kKnnMaxBlocks = 1024;  // rows of the distance workspace: one per block
constexpr int kForcePts = 16;        // points per forces block
constexpr int kForceSeg = 16;        // interleaved segments a point's sums are cut into: one thread each
static_assert(kForcePts * kForceSeg == 256, "one thread per (point, segment)");

// ---- neighbours --------------------------------------------------------------------------------------------
// A block owns row i (rows i, i + gridDim.x, ...). Distances: wave w takes j = w, w + 4, ...; lane l sums
// (double(x_il') - double(x_jl'))^2 over l' = l, l + 64, ... ascending with one fma per term, then wave_sum_d; the
// n distances go to the block's own row of the workspace. Selection: k rounds, each the smallest (distance, index)
// pair, in that lexicographic order, above the pair the round before selected; j = i is left out. A minimum under a
// total order does not depend on the order it is taken in. A row with fewer than k selectable entries (NaN input:
// every comparison with NaN is false) writes index -1, which the host refuses.
__global__ void __launch_bounds__(256) k_tsne_knn(const float* __restrict__ X, int n, int L, int64_t ldx, int k,
                                                  int32_t* __restrict__ idx, double* __restrict__ d2,
                                                  double* __restrict__ ws) {
  __shared__ double xi[HVAE_TSNE_MAX_L];
  __shared__ double rd[4];
  __shared__ int rj[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* dist = ws + (int64_t)blockIdx.x * n;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {  // the same trip count in every thread of the block
    __syncthreads();
    for (int l = t; l < L; l += 256) xi[l] = (double)X[(int64_t)i * ldx + l];
    __syncthreads();
    for (int j = wave; j < n; j += 4) {
      const float* xj = X + (int64_t)j * ldx;
      double acc = 0.0;
      for (int l = lane; l < L; l += 64) {
        const double diff = xi[l] - (double)xj[l];
        acc = fma(diff, diff, acc);
      }
      acc = wave_sum_d(acc);
      if (lane == 0) dist[j] = acc;
    }
    __syncthreads();
    double last_d = -1.0;
    int last_j = -1;
    for (int r = 0; r < k; ++r) {
      double bd = INFINITY;
      int bj = INT32_MAX;
      for (int j = t; j < n; j += 256) {
        if (j == i) continue;
        const double v = dist[j];
        const bool after = v > last_d || (v == last_d && j > last_j);
        const bool less = v < bd || (v == bd && j < bj);
        if (after && less) {
          bd = v;
          bj = j;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (od < bd || (od == bd && oj < bj)) {
          bd = od;
          bj = oj;
        }
      }
      if (lane == 0) {
        rd[wave] = bd;
        rj[wave] = bj;
      }
      __syncthreads();
      bd = rd[0];
      bj = rj[0];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (rd[w] < bd || (rd[w] == bd && rj[w] < bj)) {
          bd = rd[w];
          bj = rj[w];
        }
      if (t == 0) {
        idx[(int64_t)i * k + r] = bj == INT32_MAX ? -1 : bj;
        d2[(int64_t)i * k + r] = bd;
      }
      last_d = bd;
      last_j = bj;
      __syncthreads();
    }
  }
}

// ---- perplexity --------------------------------------------------------------------------------------------
// scikit-learn's _binary_search_perplexity, one row per wave: lane l holds the entries l, l + 64, l + 128, l + 192 of
// the row (k <= 255). Each of the two sums of a step (sum P, sum d P) is the lane's entries ascending, then
// wave_sum_d; every lane holds the same sums, so the loop's branches are uniform.
__global__ void __launch_bounds__(256) k_tsne_perplexity(const double* __restrict__ d2, int n, int k, double log_perp,
                                                         double* __restrict__ P) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  double d[4], p[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = lane + 64 * q;
    d[q] = e < k ? d2[(int64_t)row * k + e] : 0.0;
    p[q] = 0.0;
  }
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      p[q] = lane + 64 * q < k ? exp(-d[q] * beta) : 0.0;
      s += p[q];
    }
    s = wave_sum_d(s);
    if (s == 0.0) s = 1e-8;
    double sd = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      p[q] = p[q] / s;
      sd += d[q] * p[q];
    }
    sd = wave_sum_d(sd);
    const double diff = log(s) + beta * sd - log_perp;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = lane + 64 * q;
    if (e < k) P[(int64_t)row * k + e] = p[q];
  }
}

// ---- forces ------------------------------------------------------------------------------------------------
// A block owns kForcePts points; thread (point p = t & 15, segment s = t >> 4). The repulsion and the row's share of
// Z: y goes through LDS in tiles of 256 points as pairs of doubles; segment s adds the tile entries s, s + 16, ...,
// tiles ascending, so it holds the terms j = s (mod 16) in ascending j. The attraction: segment s adds the entries
// ptr[i] + s, + 16, ... of the point's CSR row in storage order. Each of the five sums is then the sixteen segments
// added in order s = 0, 1, ..., 15. j = i adds nothing; a coincident j != i has q = 1 and a zero difference.
__global__ void __launch_bounds__(256) k_tsne_forces(const double2* __restrict__ Y, int n,
                                                     const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                     const double* __restrict__ pval, double2* __restrict__ attr,
                                                     double2* __restrict__ rep, double* __restrict__ z) {
  __shared__ double2 ty[256];
  __shared__ double part[5][kForceSeg][kForcePts];
  const int t = threadIdx.x, p = t & (kForcePts - 1), s = t / kForcePts;
  const int i = blockIdx.x * kForcePts + p;
  const bool live = i < n;
  const double2 yi = live ? Y[i] : make_double2(0.0, 0.0);
  double rx = 0.0, ry = 0.0, zs = 0.0;
  for (int base = 0; base < n; base += 256) {
    __syncthreads();
    ty[t] = base + t < n ? Y[base + t] : make_double2(0.0, 0.0);
    __syncthreads();
    const int cnt = n - base < 256 ? n - base : 256;
    for (int jj = s; jj < cnt; jj += kForceSeg) {
      const double dx = yi.x - ty[jj].x, dy = yi.y - ty[jj].y;
      const double q = 1.0 / (1.0 + (dx * dx + dy * dy));
      if (base + jj != i) {
        const double q2 = q * q;
        zs += q;
        rx = fma(q2, dx, rx);
        ry = fma(q2, dy, ry);
      }
    }
  }
  double ax = 0.0, ay = 0.0;
  if (live) {
    const int64_t e1 = ptr[i + 1];
    for (int64_t e = ptr[i] + s; e < e1; e += kForceSeg) {
      const int j = col[e];
      const bool ok = j >= 0 && j < n;  // a broken matrix gives NaN, not a read out of bounds
      const double2 yj = Y[ok ? j : 0];
      const double dx = yi.x - yj.x, dy = yi.y - yj.y;
      const double pq = (ok ? pval[e] : (double)NAN) / (1.0 + (dx * dx + dy * dy));
      ax = fma(pq, dx, ax);
      ay = fma(pq, dy, ay);
    }
  }
  part[0][s][p] = ax;
  part[1][s][p] = ay;
  part[2][s][p] = rx;
  part[3][s][p] = ry;
  part[4][s][p] = zs;
  __syncthreads();
  if (s == 0 && live) {
    double v[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      v[c] = part[c][0][p];
      for (int u = 1; u < kForceSeg; ++u) v[c] += part[c][u][p];
    }
    attr[i] = make_double2(v[0], v[1]);
    rep[i] = make_double2(v[2], v[3]);
    z[i] = v[4];
  }
}

// ---- update ------------------------------------------------------------------------------------------------
// Sum of 256 threads' values in one order: wave_sum_d, then the four waves as ((w0 + w1) + w2) + w3.
__device__ __forceinline__ double tsne_block_sum(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Every block sums Z itself, the same way: thread t adds z[t], z[t + 256], ... ascending, then tsne_block_sum. Then one
// thread per point: the gradient, scikit-learn's _gradient_descent step on its two coordinates, y_out = y_in + update.
// With stats, the point's KL terms over its CSR row in storage order at y_in (y_out is another buffer, so no block
// reads what another writes) and its squared gradient after the gains; each of the two is summed over the block by
// tsne_block_sum into the block's pair of partials, which k_tsne_stats adds in block order.
__global__ void __launch_bounds__(256) k_tsne_update(const double2* __restrict__ attr, const double2* __restrict__ rep,
                                                     const double* __restrict__ z, int n, double exag, double momentum,
                                                     double lr, double2* __restrict__ gains, double2* __restrict__ upd,
                                                     const double2* __restrict__ y_in, double2* __restrict__ y_out,
                                                     const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                     const double* __restrict__ pval, int want_stats,
                                                     double* __restrict__ partials, double2* __restrict__ grad_out,
                                                     double* __restrict__ z_out) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double zs = 0.0;
  for (int j = t; j < n; j += 256) zs += z[j];
  double Z = tsne_block_sum(zs, red);
  Z = Z > DBL_EPSILON ? Z : DBL_EPSILON;
  if (z_out && blockIdx.x == 0 && t == 0) *z_out = Z;
  const int i = blockIdx.x * 256 + t;
  double gn2 = 0.0, err = 0.0;
  if (i < n) {
    const double2 a = attr[i], r = rep[i], g0 = gains[i], u0 = upd[i], y = y_in[i];
    double g[2] = {4.0 * (exag * a.x - r.x / Z), 4.0 * (exag * a.y - r.y / Z)};
    if (grad_out) grad_out[i] = make_double2(g[0], g[1]);
    double gain[2] = {g0.x, g0.y}, u[2] = {u0.x, u0.y};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      gain[c] = u[c] * g[c] < 0.0 ? gain[c] + 0.2 : gain[c] * 0.8;
      gain[c] = gain[c] > 0.01 ? gain[c] : 0.01;
      g[c] *= gain[c];
      u[c] = momentum * u[c] - lr * g[c];
      gn2 += g[c] * g[c];
    }
    gains[i] = make_double2(gain[0], gain[1]);
    upd[i] = make_double2(u[0], u[1]);
    y_out[i] = make_double2(y.x + u[0], y.y + u[1]);
    if (want_stats) {
      const int64_t e1 = ptr[i + 1];
      for (int64_t e = ptr[i]; e < e1; ++e) {
        const int j = col[e];
        const bool ok = j >= 0 && j < n;
        const double2 yj = y_in[ok ? j : 0];
        const double dx = y.x - yj.x, dy = y.y - yj.y;
        const double q = 1.0 / (1.0 + (dx * dx + dy * dy));
        const double pe = ok ? exag * pval[e] : (double)NAN;
        err += pe * log(fmax(pe, (double)FLT_MIN) / fmax(q / Z, (double)FLT_MIN));
      }
    }
  }
  if (want_stats) {
    const double e_sum = tsne_block_sum(err, red);
    const double g_sum = tsne_block_sum(gn2, red);
    if (t == 0) {
      partials[2 * blockIdx.x] = e_sum;
      partials[2 * blockIdx.x + 1] = g_sum;
    }
  }
}

// stats[0] = the KL error, stats[1] = the gradient's 2-norm: the blocks' partials added in block order by one thread.
__global__ void k_tsne_stats(const double* __restrict__ partials, int nb, double* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double e = 0.0, g = 0.0;
  for (int b = 0; b < nb; ++b) {
    e += partials[2 * b];
    g += partials[2 * b + 1];
  }
  stats[0] = e;
  stats[1] = sqrt(g);
}

static int knn_blocks(int64_t n) { return (int)(n < kKnnMaxBlocks ? n : kKnnMaxBlocks); }

}  // namespace hvae

using namespace hvae;

static bool tsne_n_ok(int64_t n) { return n >= HVAE_TSNE_MIN_N && n <= HVAE_TSNE_MAX_N; }
#define TSNE_REQUIRE_N(what)                                                                                   \
  HVAE_REQUIRE(tsne_n_ok(n), what ": n = %lld is not served (%d to %d points)", (long long)n, HVAE_TSNE_MIN_N, \
               HVAE_TSNE_MAX_N)

extern "C" size_t hvae_tsne_knn_workspace(int64_t n) {
  if (!tsne_n_ok(n)) return 0;
  return (size_t)knn_blocks(n) * (size_t)n * sizeof(double);
}

extern "C" int hvae_tsne_knn(const float* X, int64_t n, int64_t L, int64_t ldx, int64_t k, int32_t* idx, double* d2,
                             void* ws, size_t ws_bytes, void* stream) {
  TSNE_REQUIRE_N("hvae_tsne_knn");
  HVAE_REQUIRE(L >= HVAE_TSNE_MIN_L && L <= HVAE_TSNE_MAX_L && ldx >= L,
               "hvae_tsne_knn: L = %lld (row stride %lld) is not served (%d to %d columns, stride >= L)",
               (long long)L, (long long)ldx, HVAE_TSNE_MIN_L, HVAE_TSNE_MAX_L);
  HVAE_REQUIRE(k >= 1 && k <= HVAE_TSNE_MAX_K && k < n, "hvae_tsne_knn: k = %lld is not served (1 to min(n - 1, %d))",
               (long long)k, HVAE_TSNE_MAX_K);
  HVAE_REQUIRE(X && idx && d2 && ws, "hvae_tsne_knn: null pointer");
  HVAE_REQUIRE(ws_bytes >= hvae_tsne_knn_workspace(n), "hvae_tsne_knn: ws holds %zu bytes, needs %zu", ws_bytes,
               hvae_tsne_knn_workspace(n));
  HVAE_REQUIRE(((uintptr_t)ws & 7) == 0, "hvae_tsne_knn: ws must be 8-byte aligned");
  k_tsne_knn<<<knn_blocks(n), 256, 0, as_stream(stream)>>>(X, (int)n, (int)L, ldx, (int)k, idx, d2, (double*)ws);
  HVAE_LAUNCH_CHECK("k_tsne_knn");
  return HVAE_OK;
}

extern "C" int hvae_tsne_perplexity(const double* d2, int64_t n, int64_t k, double perplexity, double* P,
                                    void* stream) {
  TSNE_REQUIRE_N("hvae_tsne_perplexity");
  HVAE_REQUIRE(k >= 1 && k <= HVAE_TSNE_MAX_K && k < n,
               "hvae_tsne_perplexity: k = %lld is not served (1 to min(n - 1, %d))", (long long)k, HVAE_TSNE_MAX_K);
  HVAE_REQUIRE(perplexity > 0.0 && perplexity < (double)n,
               "hvae_tsne_perplexity: perplexity = %g is not served (0 < perplexity < n)", perplexity);
  HVAE_REQUIRE(d2 && P && d2 != P, "hvae_tsne_perplexity: null or aliased pointer");
  k_tsne_perplexity<<<(unsigned)cdiv(n, 4), 256, 0, as_stream(stream)>>>(d2, (int)n, (int)k, log(perplexity), P);
  HVAE_LAUNCH_CHECK("k_tsne_perplexity");
  return HVAE_OK;
}

extern "C" int hvae_tsne_forces(const double* Y, int64_t n, const int64_t* ptr, const int32_t* col, const double* pval,
                                double* attr, double* rep, double* z, void* stream) {
  TSNE_REQUIRE_N("hvae_tsne_forces");
  HVAE_REQUIRE(Y && ptr && col && pval && attr && rep && z, "hvae_tsne_forces: null pointer");
  HVAE_REQUIRE((((uintptr_t)Y | (uintptr_t)attr | (uintptr_t)rep) & 15) == 0,
               "hvae_tsne_forces: Y, attr and rep must be 16-byte aligned");
  k_tsne_forces<<<(unsigned)cdiv(n, kForcePts), 256, 0, as_stream(stream)>>>(
      (const double2*)Y, (int)n, ptr, col, pval, (double2*)attr, (double2*)rep, z);
  HVAE_LAUNCH_CHECK("k_tsne_forces");
  return HVAE_OK;
}

extern "C" size_t hvae_tsne_update_workspace(int64_t n) {
  if (!tsne_n_ok(n)) return 0;
  return (size_t)cdiv(n, 256) * 2 * sizeof(double);
}

extern "C" int hvae_tsne_update(const double* attr, const double* rep, const double* z, int64_t n, double exaggeration,
                                double momentum, double lr, double* gains, double* upd, const double* y_in,
                                double* y_out, const int64_t* ptr, const int32_t* col, const double* pval,
                                int want_stats, double* stats, double* grad_out, double* z_out, void* ws,
                                size_t ws_bytes, void* stream) {
  TSNE_REQUIRE_N("hvae_tsne_update");
  HVAE_REQUIRE(attr && rep && z && gains && upd && y_in && y_out, "hvae_tsne_update: null pointer");
  HVAE_REQUIRE(y_in != y_out, "hvae_tsne_update: y_out may not alias y_in");
  HVAE_REQUIRE((((uintptr_t)attr | (uintptr_t)rep | (uintptr_t)gains | (uintptr_t)upd | (uintptr_t)y_in |
                 (uintptr_t)y_out | (uintptr_t)grad_out) & 15) == 0,
               "hvae_tsne_update: the [n, 2] arrays must be 16-byte aligned");
  if (want_stats) {
    HVAE_REQUIRE(ptr && col && pval && stats && ws, "hvae_tsne_update: the statistics need P, stats and ws");
    HVAE_REQUIRE(ws_bytes >= hvae_tsne_update_workspace(n), "hvae_tsne_update: ws holds %zu bytes, needs %zu",
                 ws_bytes, hvae_tsne_update_workspace(n));
    HVAE_REQUIRE(((uintptr_t)ws & 7) == 0, "hvae_tsne_update: ws must be 8-byte aligned");
  }
  const int nb = (int)cdiv(n, 256);
  hipStream_t st = as_stream(stream);
  k_tsne_update<<<nb, 256, 0, st>>>((const double2*)attr, (const double2*)rep, z, (int)n, exaggeration, momentum, lr,
                                    (double2*)gains, (double2*)upd, (const double2*)y_in, (double2*)y_out, ptr, col,
                                    pval, want_stats ? 1 : 0, (double*)ws, (double2*)grad_out, z_out);
  HVAE_LAUNCH_CHECK("k_tsne_update");
  if (want_stats) {
    k_tsne_stats<<<1, 64, 0, st>>>((const double*)ws, nb, stats);
    HVAE_LAUNCH_CHECK("k_tsne_stats");
  }
  return HVAE_OK;
}
