// hvae_lgcn.hip -- the LightGCN baseline's train step: graph propagation and the BPR loss (K18).
//
// Reference: LightGCNModel / LightGCNRecommender (src/ml/baseline.py:239-385). There every batch of 1024
// interactions runs torch.sparse.mm three times forward and three times backward over a COO adjacency with one
// stored fp32 weight per edge, then indexes the layer mean and lets autograd scatter the gradient back.
//
// Here the nodes are one table [n_users + n_items, d] (users first, as torch.cat([user_emb, item_emb])), the
// adjacency is never stored: a user row reads its neighbours through the CSR of the interaction matrix, an item
// row through the CSC, and the weight of edge (u, i) is (float)(s_u * s_i) with s = deg^-1/2 in double, formed
// on the fly (the reference's FloatTensor(d_inv_sqrt[rows] * d_inv_sqrt[cols])). The weights are symmetric, so
// the layer mean and its backward are the same chain of launches (Horner form, n_layers = 3):
//   F  = 1/4 (E + A(E + A(E + A E)))        dE = 1/4 (g + A(g + A(g + A g)))
// each link one k_lgcn_propagate: out[r] = alpha * (add[r] + sum_{j in N(r)} w_rj x[j]).
//
// Everything is fp32 with no floating-point atomics; every sum has one fixed order that depends on the graph
// (or the batch plan) only, so two runs are bitwise equal.
//
// A propagated row is a gathered row sum of hvae_rowgather.h, whose first comment states its summation order: lane
// l owns columns [l V, l V + V) (V = d / 64), so a neighbour row is one coalesced 256-byte (d = 64) or 512-byte
// (d = 128) read.
#include "hvae_rowgather.h"

namespace hvae {

__global__ void __launch_bounds__(256) k_lgcn_norm(const int64_t* __restrict__ row_ptr, int64_t n_users,
                                                   const int64_t* __restrict__ col_ptr, int64_t n_items,
                                                   double* __restrict__ scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_users + n_items) return;
  const int64_t deg = i < n_users ? row_ptr[i + 1] - row_ptr[i] : col_ptr[i - n_users + 1] - col_ptr[i - n_users];
  scale[i] = deg > 0 ? 1.0 / sqrt((double)deg) : 0.0;
}

// out[r] = alpha * (add[r] + sum_{j in N(r)} w_rj x[j]) with w_rj = (float)(s_r * s_j); a user row's neighbours are
// col_idx + n_users, an item row's row_idx. A neighbour outside the other side's node range (a broken graph) reads
// that range's first row with a NaN weight instead of reading out of bounds.
template <int V>
__global__ void __launch_bounds__(256) k_lgcn_propagate(const int64_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ col_idx,
                                                        const int64_t* __restrict__ col_ptr,
                                                        const int32_t* __restrict__ row_idx,
                                                        const double* __restrict__ scale, int64_t n_users,
                                                        int64_t n_items, const float* __restrict__ x,
                                                        const float* add, float* out, float alpha) {
  using Row = RowVec<float, V>;
  const int lane = threadIdx.x & 63;
  const int64_t n = n_users + n_items;
  gather_rows<float, V>(
      n, true,
      [&](int64_t r, int64_t& p0, int64_t& p1) {
        const bool is_user = r < n_users;
        const int64_t* ptr = is_user ? row_ptr + r : col_ptr + (r - n_users);
        const int32_t* idx = is_user ? col_idx : row_idx;
        p0 = ptr[0];
        p1 = ptr[1];
        const int64_t off = is_user ? n_users : 0, lo = is_user ? n_users : 0, hi = is_user ? n : n_users;
        const double s_r = scale[r];
        return [=](int64_t p) {
          const int64_t j = (int64_t)idx[p] + off;
          return j >= lo && j < hi ? GatherEntry<float>{(int)j, (float)(s_r * scale[j])}
                                   : GatherEntry<float>{(int)lo, NAN};
        };
      },
      [&](int j) { return ld_row<float, V>(x, j, lane); },
      [&](int64_t r, Row s) {
        if (add) {
          const Row e = ld_row<float, V>(add, r, lane);
#pragma unroll
          for (int v = 0; v < V; ++v) s.v[v] = e.v[v] + s.v[v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) s.v[v] = alpha * s.v[v];
        st_row<float, V>(out, r, lane, s);
      });
}

// ---- BPR -------------------------------------------------------------------------------------------------
// Per triple b = (u, p, n) of the batch, from the rows of F (fp32 dots, butterfly wave sums):
//   x = F_u . F_p - F_u . F_n,  loss_b = softplus(-x),  coef_b = -sigmoid(-x) / nb        (scalars in double)
// so that dL/dF_u += coef_b (F_p - F_n), dL/dF_p += coef_b F_u, dL/dF_n -= coef_b F_u, and the regulariser
// reg (|U|^2 + |P|^2 + |N|^2) / nb over the gathered [nb, d] matrices adds (2 reg / nb) times its own row to a
// node once per occurrence.
template <int V>
__global__ void __launch_bounds__(256) k_lgcn_bpr_rows(const float* __restrict__ F, int64_t n_users, int64_t n_items,
                                                       const int32_t* __restrict__ users,
                                                       const int32_t* __restrict__ pos,
                                                       const int32_t* __restrict__ neg, int64_t nb,
                                                       float* __restrict__ coef, double* __restrict__ sp,
                                                       double* __restrict__ sq) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  const int64_t u = users[b], p = pos[b], q = neg[b];
  if (u < 0 || u >= n_users || p < 0 || p >= n_items || q < 0 || q >= n_items) {  // a caller's bug, made visible
    if (lane == 0) { coef[b] = NAN; sp[b] = NAN; sq[b] = NAN; }
    return;
  }
  const RowVec<float, V> fu = ld_row<float, V>(F, u, lane), fp = ld_row<float, V>(F, n_users + p, lane),
                         fn = ld_row<float, V>(F, n_users + q, lane);
  float dp = 0.f, dn = 0.f, nn = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    dp = fmaf(fu.v[v], fp.v[v], dp);
    dn = fmaf(fu.v[v], fn.v[v], dn);
    nn = fmaf(fu.v[v], fu.v[v], nn);
    nn = fmaf(fp.v[v], fp.v[v], nn);
    nn = fmaf(fn.v[v], fn.v[v], nn);
  }
  dp = wave_sum(dp);
  dn = wave_sum(dn);
  nn = wave_sum(nn);
  if (lane == 0) {
    const double x = (double)(dp - dn);
    sp[b] = fmax(-x, 0.0) + log1p(exp(-fabs(x)));
    coef[b] = (float)(-1.0 / (1.0 + exp(x)) / (double)nb);
    sq[b] = (double)nn;
  }
}

// One wave per node of the batch (a segment of the plan: its occurrences as slots role * nb + b, ascending; role
// 0 = user, 1 = positive, 2 = negative), lanes over the columns. Per occurrence, in slot order:
//   role 0: acc = fma(coef_b, F_p, acc); acc = fma(-coef_b, F_n, acc)
//   role 1: acc = fma(coef_b, F_u, acc)        role 2: acc = fma(-coef_b, F_u, acc)
//   then    acc = fma(2 reg / nb, F_node, acc)
// The last block sums the batch's loss terms (thread-strided, then a butterfly, then ((w0 + w1) + w2) + w3, in
// double) into loss = mean softplus + reg * sum sq / nb, rounded to fp32.
template <int V>
__global__ void __launch_bounds__(256) k_lgcn_bpr_grad(const float* __restrict__ F, int64_t n_users, int64_t n_items,
                                                       const int32_t* __restrict__ users,
                                                       const int32_t* __restrict__ pos,
                                                       const int32_t* __restrict__ neg, int64_t nb,
                                                       const int32_t* __restrict__ slots,
                                                       const int32_t* __restrict__ seg_off, int64_t n_seg,
                                                       const float* __restrict__ coef, const double* __restrict__ sp,
                                                       const double* __restrict__ sq, float r2, double reg,
                                                       float* __restrict__ g, float* __restrict__ loss_out,
                                                       double* __restrict__ loss_accum) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double lred[2][4];
    double a = 0.0, c = 0.0;
    for (int64_t i = threadIdx.x; i < nb; i += 256) {
      a += sp[i];
      c += sq[i];
    }
    a = wave_sum_d(a);
    c = wave_sum_d(c);
    if (lane == 0) { lred[0][threadIdx.x >> 6] = a; lred[1][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double ssp = ((lred[0][0] + lred[0][1]) + lred[0][2]) + lred[0][3];
      const double ssq = ((lred[1][0] + lred[1][1]) + lred[1][2]) + lred[1][3];
      const float loss = (float)(ssp / (double)nb + reg * ssq / (double)nb);
      if (loss_out) *loss_out = loss;
      if (loss_accum) *loss_accum += (double)loss;
    }
    return;
  }
  const int64_t s = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (s >= n_seg) return;
  const int64_t e0 = seg_off[s], e1 = seg_off[s + 1];
  const int64_t n = n_users + n_items;
  if (e0 < 0 || e1 <= e0 || e1 > 3 * nb) return;  // a broken plan writes nothing
  int64_t node = -1;
  RowVec<float, V> acc = {}, self = {};
  bool bad = false;
  for (int64_t base = e0; base < e1; base += 64) {
    const int cnt = (int)(e1 - base < 64 ? e1 - base : 64);
    int me = -1, ia = 0, ib = -1;
    float ca = 0.f;
    if (lane < cnt) {
      const int64_t t = slots[base + lane];
      if (t >= 0 && t < 3 * nb) {
        const int role = (int)(t / nb);
        const int64_t b = t - role * nb;
        const int64_t u = users[b], p = pos[b], q = neg[b];
        if (u >= 0 && u < n_users && p >= 0 && p < n_items && q >= 0 && q < n_items) {
          const float c = coef[b];
          // selects, not an if / else chain over role: hipcc's code for the chain lost the negation of role 2
          const int iu = (int)u, ip = (int)(n_users + p), iq = (int)(n_users + q);
          me = role == 0 ? iu : (role == 1 ? ip : iq);
          ia = role == 0 ? ip : iu;
          ib = role == 0 ? iq : -1;
          ca = role == 2 ? -c : c;
        }
      }
    }
    for (int k = 0; k < cnt; ++k) {
      const int m = __builtin_amdgcn_readlane(me, k);
      if (m < 0 || (node >= 0 && m != node)) { bad = true; continue; }
      if (node < 0) {
        node = m;
        self = ld_row<float, V>(F, node, lane);
      }
      const float c = bcast(ca, k);
      fma_row<float, V>(acc, c, ld_row<float, V>(F, __builtin_amdgcn_readlane(ia, k), lane));
      const int j = __builtin_amdgcn_readlane(ib, k);
      if (j >= 0) fma_row<float, V>(acc, -c, ld_row<float, V>(F, j, lane));
      fma_row<float, V>(acc, r2, self);
    }
  }
  if (node < 0 || node >= n) return;
  if (bad) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc.v[v] = NAN;
  }
  st_row<float, V>(g, node, lane, acc);
}

}  // namespace hvae

using namespace hvae;

static bool lgcn_dim_ok(int64_t d) { return d == 64 || d == 128; }

extern "C" int hvae_lgcn_norm(const int64_t* row_ptr, int64_t n_users, const int64_t* col_ptr, int64_t n_items,
                              double* scale, void* stream) {
  HVAE_REQUIRE(n_users > 0 && n_items > 0 && n_users + n_items < INT32_MAX, "hvae_lgcn_norm: bad args");
  HVAE_REQUIRE(row_ptr && col_ptr && scale, "hvae_lgcn_norm: null pointer");
  k_lgcn_norm<<<(unsigned)cdiv(n_users + n_items, 256), 256, 0, as_stream(stream)>>>(row_ptr, n_users, col_ptr,
                                                                                     n_items, scale);
  HVAE_LAUNCH_CHECK("k_lgcn_norm");
  return HVAE_OK;
}

extern "C" int hvae_lgcn_propagate(const hvae_lgcn_graph* gr, int64_t d, const float* x, const float* add,
                                   float* out, float alpha, void* stream) {
  HVAE_REQUIRE(gr && gr->n_users > 0 && gr->n_items > 0 && gr->n_users + gr->n_items < INT32_MAX,
               "hvae_lgcn_propagate: bad args");
  HVAE_REQUIRE(lgcn_dim_ok(d), "hvae_lgcn_propagate: d = %lld is not served (64 or 128)", (long long)d);
  HVAE_REQUIRE(gr->row_ptr && gr->col_idx && gr->col_ptr && gr->row_idx && gr->scale && x && out,
               "hvae_lgcn_propagate: null pointer");
  HVAE_REQUIRE(x != out, "hvae_lgcn_propagate: out may not alias x");
  const unsigned grid = (unsigned)cdiv(gr->n_users + gr->n_items, kGatherRows);
  hipStream_t st = as_stream(stream);
  if (d == 64)
    k_lgcn_propagate<1><<<grid, 256, 0, st>>>(gr->row_ptr, gr->col_idx, gr->col_ptr, gr->row_idx, gr->scale,
                                              gr->n_users, gr->n_items, x, add, out, alpha);
  else
    k_lgcn_propagate<2><<<grid, 256, 0, st>>>(gr->row_ptr, gr->col_idx, gr->col_ptr, gr->row_idx, gr->scale,
                                              gr->n_users, gr->n_items, x, add, out, alpha);
  HVAE_LAUNCH_CHECK("k_lgcn_propagate");
  return HVAE_OK;
}

extern "C" size_t hvae_lgcn_bpr_workspace(int64_t nb) {
  if (nb <= 0) return 0;
  return (size_t)nb * (2 * sizeof(double) + sizeof(float));
}

extern "C" int hvae_lgcn_bpr(const float* F, int64_t n_users, int64_t n_items, int64_t d, const int32_t* users,
                             const int32_t* pos, const int32_t* neg, int64_t nb, const int32_t* slots,
                             const int32_t* seg_off, int64_t n_seg, double reg, float* g, float* loss_out,
                             double* loss_accum, void* ws, size_t ws_bytes, void* stream) {
  HVAE_REQUIRE(n_users > 0 && n_items > 0 && n_users + n_items < INT32_MAX, "hvae_lgcn_bpr: bad args");
  HVAE_REQUIRE(lgcn_dim_ok(d), "hvae_lgcn_bpr: d = %lld is not served (64 or 128)", (long long)d);
  HVAE_REQUIRE(nb >= 1 && nb <= HVAE_LGCN_MAX_BATCH, "hvae_lgcn_bpr: nb = %lld outside [1, %d]", (long long)nb,
               HVAE_LGCN_MAX_BATCH);
  HVAE_REQUIRE(n_seg >= 1 && n_seg <= 3 * nb, "hvae_lgcn_bpr: n_seg = %lld outside [1, 3 nb]", (long long)n_seg);
  HVAE_REQUIRE(F && users && pos && neg && slots && seg_off && g && ws, "hvae_lgcn_bpr: null pointer");
  HVAE_REQUIRE(ws_bytes >= hvae_lgcn_bpr_workspace(nb), "hvae_lgcn_bpr: ws holds %zu bytes, needs %zu", ws_bytes,
               hvae_lgcn_bpr_workspace(nb));
  HVAE_REQUIRE(((uintptr_t)ws & 7) == 0, "hvae_lgcn_bpr: ws must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  double* sp = (double*)ws;
  double* sq = sp + nb;
  float* coef = (float*)(sq + nb);
  const float r2 = (float)(2.0 * reg / (double)nb);
  HVAE_HIP(hipMemsetAsync(g, 0, (size_t)(n_users + n_items) * (size_t)d * sizeof(float), st));
  const unsigned g1 = (unsigned)cdiv(nb, 4), g2 = (unsigned)cdiv(n_seg, 4) + 1;
  if (d == 64) {
    k_lgcn_bpr_rows<1><<<g1, 256, 0, st>>>(F, n_users, n_items, users, pos, neg, nb, coef, sp, sq);
    HVAE_LAUNCH_CHECK("k_lgcn_bpr_rows");
    k_lgcn_bpr_grad<1><<<g2, 256, 0, st>>>(F, n_users, n_items, users, pos, neg, nb, slots, seg_off, n_seg, coef, sp,
                                           sq, r2, reg, g, loss_out, loss_accum);
  } else {
    k_lgcn_bpr_rows<2><<<g1, 256, 0, st>>>(F, n_users, n_items, users, pos, neg, nb, coef, sp, sq);
    HVAE_LAUNCH_CHECK("k_lgcn_bpr_rows");
    k_lgcn_bpr_grad<2><<<g2, 256, 0, st>>>(F, n_users, n_items, users, pos, neg, nb, slots, seg_off, n_seg, coef, sp,
                                           sq, r2, reg, g, loss_out, loss_accum);
  }
  HVAE_LAUNCH_CHECK("k_lgcn_bpr_grad");
  return HVAE_OK;
}
