// hvae_mvae.hip -- the Mult-VAE baseline's own kernels (K20): the first layer over sparse rows with its L2
// normalisation, input dropout, tanh and hidden dropout; the elementwise tanh + dropout of the dense layers and
// its backward; and the multinomial loss with its gradient against a sparse target, in place over stored logits.
// Every dense product, the row-sparse W1 gradient, Adam, the reparameterisation and the loss means are the
// library's existing entry points (src/ml/multvae.py strings them together).
//
// Reference: src/ml/baseline.py:126-231 (MultVAE, MultVAERecommender.fit).
//
// All fp32, wave64, no floating-point atomics, tanhf / expf / logf / sqrtf of the device library (the build has no
// fast-math). Every sum has one fixed order, stated at its kernel: two runs give the same bits.
#include "hvae_common.h"

namespace hvae {

enum : uint32_t {
  kTagMvaeIn = 0x400u,    // input mask, element index b * N + j (independent of the CSR layout)
  kTagMvaeHid1 = 0x401u,  // first hidden mask, element index b * H + h
  kTagMvaeHid2 = 0x402u,  // second hidden mask (hvae_mvae_tanh_drop_*'s caller passes the tag)
};

constexpr float kNormEps = 1e-12f;  // F.normalize's eps

// One wave per batch row, four rows per 256-thread block. Lane l holds the float4 chunks l, l + 64, ... of the
// row's H columns (NV chunks, chunk c valid iff 4 c < H).
//   ss    = sum of x_e^2: lane l adds its entries l, l + 64, ... in storage order, then the xor butterfly
//           (wave_sum) over the 64 lanes;
//   den   = max(sqrtf(ss), 1e-12f);  xs_e = (x_e / den) * in_mult_e
//   a[c]  = b1[c], then a[c] = fmaf(xs_e, w1t[j_e][c], a[c]) for the row's entries e in storage order
//   t = tanhf(a);  h = t * mult
// A column index outside [0, N) contributes NaN and is never used as an address.
template <int NV>
__global__ void __launch_bounds__(256) k_mvae_encoder_fwd(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx, const float* __restrict__ vals,
    const int32_t* __restrict__ rows, const int64_t* __restrict__ rows_offset, int64_t nb, int64_t N,
    const float* __restrict__ w1t, const float* __restrict__ b1, int64_t H, float p_in, float scale_in,
    float p_drop, float scale, const float* __restrict__ in_mult, const float* __restrict__ drop_mult,
    uint64_t seed, const int64_t* __restrict__ step_dev, int train, float* __restrict__ xs_out,
    float* __restrict__ t_out, float* __restrict__ h_out) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;  // whole waves leave; no block-wide barrier below
  const int64_t step = load_step(step_dev);
  const int64_t r = batch_row(rows, rows_offset, b);
  const int64_t beg = row_ptr[r], end = row_ptr[r + 1];

  float ss = 0.f;
  for (int64_t e = beg + lane; e < end; e += 64) {
    const float v = vals[e];
    ss = fmaf(v, v, ss);
  }
  const float den = fmaxf(sqrtf(wave_sum(ss)), kNormEps);

  float4 acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int64_t c = 4 * (int64_t)(lane + 64 * k);
    acc[k] = (c < H) ? *reinterpret_cast<const float4*>(b1 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // The entries are fetched 64 at a time (one per lane) and broadcast with v_readlane; four item rows are in
  // flight per step. The fma chain of a column runs in entry order either way.
  for (int64_t base = beg; base < end; base += 64) {
    const int n = (int)min((int64_t)64, end - base);
    int my_j = 0;
    float my_x = 0.f;
    if (lane < n) {
      my_j = col_idx[base + lane];
      float m = 1.f;
      if (train) {
        const uint64_t idx = in_mult ? (uint64_t)(base + lane) : (uint64_t)(b * N + (int64_t)my_j);
        m = dropout_mult(p_in, scale_in, in_mult, idx, seed, step, kTagMvaeIn);
      }
      my_x = (vals[base + lane] / den) * m;
      if (xs_out) xs_out[base + lane] = my_x;
      if ((uint32_t)my_j >= (uint64_t)N) { my_j = 0; my_x = NAN; }  // row 0 is read, the product is NaN
    }
    int t = 0;
    for (; t + 4 <= n; t += 4) {
      int j[4];
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        j[u] = __builtin_amdgcn_readlane(my_j, t + u);
        x[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_x), t + u));
      }
      float4 w[NV][4];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int64_t c = 4 * (int64_t)(lane + 64 * k);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          w[k][u] = c < H ? *reinterpret_cast<const float4*>(w1t + (int64_t)j[u] * H + c)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[k].x = fmaf(x[u], w[k][u].x, acc[k].x); acc[k].y = fmaf(x[u], w[k][u].y, acc[k].y);
          acc[k].z = fmaf(x[u], w[k][u].z, acc[k].z); acc[k].w = fmaf(x[u], w[k][u].w, acc[k].w);
        }
    }
    for (; t < n; ++t) {
      const int j = __builtin_amdgcn_readlane(my_j, t);
      const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_x), t));
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int64_t c = 4 * (int64_t)(lane + 64 * k);
        if (c >= H) continue;
        const float4 w = *reinterpret_cast<const float4*>(w1t + (int64_t)j * H + c);
        acc[k].x = fmaf(x, w.x, acc[k].x); acc[k].y = fmaf(x, w.y, acc[k].y);
        acc[k].z = fmaf(x, w.z, acc[k].z); acc[k].w = fmaf(x, w.w, acc[k].w);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int64_t c = 4 * (int64_t)(lane + 64 * k);
    if (c >= H) continue;  // the tail chunk of a width that is no multiple of 256 (H = 600: lanes 22.. of k = 2)
    const float tv[4] = {tanhf(acc[k].x), tanhf(acc[k].y), tanhf(acc[k].z), tanhf(acc[k].w)};
    float hv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      hv[i] = train ? tv[i] * dropout_mult(p_drop, scale, drop_mult, (uint64_t)(b * H + c + i), seed, step,
                                           kTagMvaeHid1)
                    : tv[i];
    if (t_out) *reinterpret_cast<float4*>(t_out + b * H + c) = make_float4(tv[0], tv[1], tv[2], tv[3]);
    *reinterpret_cast<float4*>(h_out + b * H + c) = make_float4(hv[0], hv[1], hv[2], hv[3]);
  }
}

// Elementwise, one float4 per thread: t = tanhf(a), h = t * mult. t may be a; h may be t when there is no mask.
__global__ void __launch_bounds__(256) k_mvae_tanh_drop_fwd(
    const float* a, int64_t lda, int64_t nb, int64_t W, float p, float scale, const float* __restrict__ drop_mult,
    uint64_t seed, const int64_t* __restrict__ step_dev, uint32_t tag, int masked, float* t_out, float* h_out,
    int64_t ldo) {
  const int64_t W4 = W >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nb * W4) return;
  const int64_t b = i / W4, c = 4 * (i - b * W4);
  const float4 av = *reinterpret_cast<const float4*>(a + b * lda + c);
  const float tv[4] = {tanhf(av.x), tanhf(av.y), tanhf(av.z), tanhf(av.w)};
  float hv[4];
  const int64_t step = masked ? load_step(step_dev) : 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    hv[k] = masked ? tv[k] * dropout_mult(p, scale, drop_mult, (uint64_t)(b * W + c + k), seed, step, tag) : tv[k];
  if (t_out) *reinterpret_cast<float4*>(t_out + b * ldo + c) = make_float4(tv[0], tv[1], tv[2], tv[3]);
  if (h_out != t_out || masked)
    *reinterpret_cast<float4*>(h_out + b * ldo + c) = make_float4(hv[0], hv[1], hv[2], hv[3]);
}

// da = dh * mult * (1 - t^2), the same multipliers as the forward's. da may be dh.
__global__ void __launch_bounds__(256) k_mvae_tanh_drop_bwd(
    const float* dh, int64_t ldd, const float* __restrict__ t, int64_t ldt, int64_t nb, int64_t W, float p,
    float scale, const float* __restrict__ drop_mult, uint64_t seed, const int64_t* __restrict__ step_dev,
    uint32_t tag, int masked, float* da, int64_t lda) {
  const int64_t W4 = W >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nb * W4) return;
  const int64_t b = i / W4, c = 4 * (i - b * W4);
  const float4 g = *reinterpret_cast<const float4*>(dh + b * ldd + c);
  const float4 tv = *reinterpret_cast<const float4*>(t + b * ldt + c);
  const float gv[4] = {g.x, g.y, g.z, g.w}, tt[4] = {tv.x, tv.y, tv.z, tv.w};
  float o[4];
  const int64_t step = masked ? load_step(step_dev) : 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float m = masked ? dropout_mult(p, scale, drop_mult, (uint64_t)(b * W + c + k), seed, step, tag) : 1.f;
    o[k] = (gv[k] * m) * fmaf(-tt[k], tt[k], 1.f);
  }
  *reinterpret_cast<float4*>(da + b * lda + c) = make_float4(o[0], o[1], o[2], o[3]);
}

// Block-wide max for 256 threads; result valid in every thread.
__device__ __forceinline__ float block_max_256(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// One 256-thread block per batch row, over the row's stored logits s = S[b, 0:N]:
//   mx   = max_j s[j]
//   se   = sum_j expf(s[j] - mx): thread t adds its columns t, t + 256, ... in ascending order, then the xor
//          butterfly over each wave's lanes, then the four waves' sums in wave order (block_sum);
//   lse  = mx + logf(se)
//   dot  = sum_e x_e (s[j_e] - lse), n = sum_e x_e: thread t adds its entries t, t + 256, ... in storage order,
//          then the same butterfly and wave order;  recon = -dot
//   (barrier: every entry logit has been read)
//   s[j] = (gs n) expf(s[j] - lse) for every j < N
//   (barrier: every column of the row has been written)
//   s[j_e] = s[j_e] - gs x_e for every entry, i.e. gs (n softmax(s)_j - x_j) with the subtraction rounded last.
// Each entry is one thread's read-modify-write: a column that occurs twice in a row would race (precondition: no
// duplicate column in a row). Columns N .. lds - 1 are neither read nor written. A column index outside [0, N)
// makes the row's recon NaN and is never used as an address.
__global__ void __launch_bounds__(256) k_mvae_nll(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx, const float* __restrict__ vals,
    const int32_t* __restrict__ rows, const int64_t* __restrict__ rows_offset, int64_t N, float* __restrict__ S,
    int64_t lds, float gs, float* __restrict__ lse_out, float* __restrict__ recon_rows) {
  __shared__ float red[4];
  const int64_t b = blockIdx.x;
  float* s = S + b * lds;
  const int64_t r = batch_row(rows, rows_offset, b);
  const int64_t beg = row_ptr[r], end = row_ptr[r + 1];

  float mx = -INFINITY;
#pragma unroll 4
  for (int64_t j = threadIdx.x; j < N; j += 256) mx = fmaxf(mx, s[j]);
  mx = block_max_256(mx, red);
  float se = 0.f;
#pragma unroll 4
  for (int64_t j = threadIdx.x; j < N; j += 256) se += expf(s[j] - mx);
  se = block_sum<256>(se, red);
  const float lse = mx + logf(se);

  float dot = 0.f, n = 0.f;
  for (int64_t e = beg + threadIdx.x; e < end; e += 256) {
    const int32_t j = col_idx[e];
    const float x = vals[e];
    const float v = (uint32_t)j < (uint64_t)N ? s[j] : NAN;
    dot = fmaf(x, v - lse, dot);
    n += x;
  }
  dot = block_sum<256>(dot, red);
  n = block_sum<256>(n, red);
  if (threadIdx.x == 0) {
    lse_out[b] = lse;
    recon_rows[b] = 0.f - dot;
  }
  __syncthreads();  // every entry logit has been read before the row is overwritten
  const float gn = gs * n;
#pragma unroll 4
  for (int64_t j = threadIdx.x; j < N; j += 256) s[j] = gn * expf(s[j] - lse);
  __syncthreads();  // the dense pass has written every column (a block's own global writes are visible after it)
  for (int64_t e = beg + threadIdx.x; e < end; e += 256) {
    const int32_t j = col_idx[e];
    if ((uint32_t)j < (uint64_t)N) s[j] = s[j] - gs * vals[e];
  }
}

static int check_width(const char* what, const char* name, int64_t H, int64_t hi) {
  if (H < 4 || H > hi || (H & 3))
    HVAE_FAIL(HVAE_ERR_UNSUPPORTED, "%s: %s = %lld is not served (a multiple of 4 in 4 .. %lld)", what, name,
              (long long)H, (long long)hi);
  return HVAE_OK;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace hvae

using namespace hvae;

extern "C" int hvae_mvae_encoder_fwd(const hvae_csr_batch* x, const float* w1t, const float* b1, int64_t H,
                                     float p_in, float p_drop, const float* in_mult, const float* drop_mult,
                                     uint64_t seed, const int64_t* step_dev, int train, float* xs_out,
                                     float* t_out, float* h_out, void* stream) {
  HVAE_REQUIRE(x && x->row_ptr && w1t && b1 && h_out, "hvae_mvae_encoder_fwd: null arg");
  if (int rc = check_width("hvae_mvae_encoder_fwd", "H", H, 2048)) return rc;
  HVAE_REQUIRE(x->nb >= 0 && x->n_items > 0 && x->n_items < ((int64_t)1 << 31),
               "hvae_mvae_encoder_fwd: nb >= 0 and 0 < n_items < 2^31 required");
  HVAE_REQUIRE(p_in >= 0.f && p_in < 1.f && p_drop >= 0.f && p_drop < 1.f,
               "hvae_mvae_encoder_fwd: dropout probabilities must lie in [0, 1)");
  HVAE_REQUIRE(aligned16(w1t) && aligned16(b1) && aligned16(h_out) && aligned16(t_out) && aligned16(drop_mult),
               "hvae_mvae_encoder_fwd: w1t, b1, t_out, h_out must be 16-B aligned");
  if (x->nb == 0) return HVAE_OK;
  HVAE_REQUIRE(x->col_idx && x->vals, "hvae_mvae_encoder_fwd: null CSR arrays");
  const float scale_in = 1.0f / (1.0f - p_in), scale = 1.0f / (1.0f - p_drop);
  const unsigned grid = (unsigned)cdiv(x->nb, 4);
  ProbeScope probe("mvae_encoder_fwd", as_stream(stream));
#define MVAE_ENC(NV_)                                                                                          \
  k_mvae_encoder_fwd<NV_><<<grid, 256, 0, as_stream(stream)>>>(                                                \
      x->row_ptr, x->col_idx, x->vals, x->rows, x->rows_offset, x->nb, x->n_items, w1t, b1, H, p_in, scale_in, \
      p_drop, scale, in_mult, drop_mult, seed, step_dev, train, xs_out, t_out, h_out)
  const int nv = (int)cdiv(H, 256);  // float4 chunks per lane
  switch (nv) {
    case 1: MVAE_ENC(1); break;
    case 2: MVAE_ENC(2); break;
    case 3: MVAE_ENC(3); break;
    case 4: MVAE_ENC(4); break;
    case 5: case 6: MVAE_ENC(6); break;
    default: MVAE_ENC(8); break;
  }
#undef MVAE_ENC
  HVAE_LAUNCH_CHECK("k_mvae_encoder_fwd");
  return HVAE_OK;
}

extern "C" int hvae_mvae_tanh_drop_fwd(const float* a, int64_t lda, int64_t nb, int64_t W, float p_drop,
                                       const float* drop_mult, uint64_t seed, const int64_t* step_dev,
                                       uint32_t tag, int train, float* t_out, float* h_out, int64_t ldo,
                                       void* stream) {
  HVAE_REQUIRE(a && h_out && nb >= 0, "hvae_mvae_tanh_drop_fwd: null arg");
  if (int rc = check_width("hvae_mvae_tanh_drop_fwd", "W", W, (int64_t)1 << 24)) return rc;
  HVAE_REQUIRE(lda >= W && ldo >= W && !(lda & 3) && !(ldo & 3) && aligned16(a) && aligned16(t_out) &&
                   aligned16(h_out) && aligned16(drop_mult),
               "hvae_mvae_tanh_drop_fwd: leading dimensions must be multiples of 4 and >= W, pointers 16-B aligned");
  HVAE_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "hvae_mvae_tanh_drop_fwd: p_drop must lie in [0, 1)");
  const int masked = train && (drop_mult || p_drop > 0.f);
  HVAE_REQUIRE(!masked || (t_out != h_out && a != h_out),
               "hvae_mvae_tanh_drop_fwd: h may alias t (or a) only without a mask");
  if (nb == 0) return HVAE_OK;
  ProbeScope probe("mvae_tanh_drop_fwd", as_stream(stream));
  k_mvae_tanh_drop_fwd<<<(unsigned)cdiv(nb * (W >> 2), 256), 256, 0, as_stream(stream)>>>(
      a, lda, nb, W, p_drop, 1.0f / (1.0f - p_drop), drop_mult, seed, step_dev, tag, masked, t_out, h_out, ldo);
  HVAE_LAUNCH_CHECK("k_mvae_tanh_drop_fwd");
  return HVAE_OK;
}

extern "C" int hvae_mvae_tanh_drop_bwd(const float* dh, int64_t ldd, const float* t, int64_t ldt, int64_t nb,
                                       int64_t W, float p_drop, const float* drop_mult, uint64_t seed,
                                       const int64_t* step_dev, uint32_t tag, int train, float* da, int64_t lda,
                                       void* stream) {
  HVAE_REQUIRE(dh && t && da && nb >= 0, "hvae_mvae_tanh_drop_bwd: null arg");
  if (int rc = check_width("hvae_mvae_tanh_drop_bwd", "W", W, (int64_t)1 << 24)) return rc;
  HVAE_REQUIRE(ldd >= W && ldt >= W && lda >= W && !(ldd & 3) && !(ldt & 3) && !(lda & 3) && aligned16(dh) &&
                   aligned16(t) && aligned16(da) && aligned16(drop_mult),
               "hvae_mvae_tanh_drop_bwd: leading dimensions must be multiples of 4 and >= W, pointers 16-B aligned");
  HVAE_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "hvae_mvae_tanh_drop_bwd: p_drop must lie in [0, 1)");
  HVAE_REQUIRE(da != t, "hvae_mvae_tanh_drop_bwd: da may alias dh, not t");
  if (nb == 0) return HVAE_OK;
  const int masked = train && (drop_mult || p_drop > 0.f);
  ProbeScope probe("mvae_tanh_drop_bwd", as_stream(stream));
  k_mvae_tanh_drop_bwd<<<(unsigned)cdiv(nb * (W >> 2), 256), 256, 0, as_stream(stream)>>>(
      dh, ldd, t, ldt, nb, W, p_drop, 1.0f / (1.0f - p_drop), drop_mult, seed, step_dev, tag, masked, da, lda);
  HVAE_LAUNCH_CHECK("k_mvae_tanh_drop_bwd");
  return HVAE_OK;
}

extern "C" int hvae_mvae_nll(const hvae_csr_batch* x, float* S, int64_t lds, float grad_scale, float* lse,
                             float* recon_rows, void* stream) {
  HVAE_REQUIRE(x && x->row_ptr && S && lse && recon_rows, "hvae_mvae_nll: null arg");
  HVAE_REQUIRE(x->nb >= 0 && x->n_items > 0 && x->n_items < ((int64_t)1 << 31) && lds >= x->n_items,
               "hvae_mvae_nll: nb >= 0, 0 < n_items < 2^31 and lds >= n_items required");
  if (x->nb == 0) return HVAE_OK;
  HVAE_REQUIRE(x->col_idx && x->vals, "hvae_mvae_nll: null CSR arrays");
  HVAE_REQUIRE(x->nb < ((int64_t)1 << 31), "hvae_mvae_nll: nb < 2^31 required (one block per row)");
  ProbeScope probe("mvae_nll", as_stream(stream));
  k_mvae_nll<<<(unsigned)x->nb, 256, 0, as_stream(stream)>>>(x->row_ptr, x->col_idx, x->vals, x->rows,
                                                             x->rows_offset, x->n_items, S, lds, grad_scale, lse,
                                                             recon_rows);
  HVAE_LAUNCH_CHECK("k_mvae_nll");
  return HVAE_OK;
}
