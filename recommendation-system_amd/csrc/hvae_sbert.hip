// hvae_sbert.hip -- the item-text encoder: a post-LayerNorm BERT body over packed sequences, in fp32 (K22).
//
// Reference: ItemEmbeddingGenerator (src/preprocessing/embeddings.py:27-131) runs SentenceTransformer.encode with
// normalize_embeddings=True: BertModel -> mean pooling -> L2 normalisation, one padded batch at a time. Here the
// sequences of a pass are packed without padding: cu[S + 1] (int32) holds the token offsets, row t of sequence s has
// position t - cu[s], and there is no attention mask anywhere. The linear layers are hvae_gemm_f32; this file holds
// what lies between them.
//
// No atomics; every sum has one fixed order that depends on the shapes only (stated beside each kernel), so two runs
// of the same input are bitwise equal. Nothing here allocates or waits; every launch goes to the caller's stream.
// Every index read from device memory (ids, cu, the work list) is checked before it addresses anything: a bad one
// gives NaN rows or an untouched output, never an access out of bounds.
#include "hvae_common.h"

namespace hvae {

typedef float sb_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4c(const float* p) { return *reinterpret_cast<const float4*>(p); }

constexpr int kSbMaxH = 1024;       // widest hidden size: 4 float4 per lane of a row's wave
constexpr int kSbMaxLen = 512;      // longest sequence the attention serves
constexpr int kSbRowF4 = kSbMaxH / 4 / 64;
constexpr int kSbTK = 16;           // keys per K / V tile
constexpr int kSbQW = 16;           // queries per wave
constexpr int kSbQB = 64;           // queries per block: one work item
constexpr int kSbRelN = kSbMaxLen + kSbQB;  // a chunk's relative-bias window: at most 575 deltas, rounded up

// ---- LayerNorm over one row held by one wave -----------------------------------------------------------------
// Lane l holds the float4 columns l, l + 64, ... (at most kSbRowF4). mean = sum / H and var = sum (x - mean)^2 / H
// (two passes over the registers, as torch's LayerNorm is two-moment exact); each sum is the lane's own columns in
// ascending order, then wave_sum's xor butterfly (the same bits in all 64 lanes).
__device__ __forceinline__ void row_ln_store(float4 (&v)[kSbRowF4], int H4, int lane, const float* __restrict__ ln_w,
                                             const float* __restrict__ ln_b, float eps, float* __restrict__ out) {
  const float invH = 1.0f / (float)(4 * H4);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i)
    if (lane + 64 * i < H4) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = wave_sum(s) * invH;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i)
    if (lane + 64 * i < H4) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) * invH + eps);
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) {
    const int c = lane + 64 * i;
    if (c < H4) {
      const float4 w = ld4c(ln_w + 4 * c), b = ld4c(ln_b + 4 * c);
      *reinterpret_cast<float4*>(out + 4 * c) =
          make_float4(v[i].x * rstd * w.x + b.x, v[i].y * rstd * w.y + b.y, v[i].z * rstd * w.z + b.z,
                      v[i].w * rstd * w.w + b.w);
    }
  }
}

__device__ __forceinline__ void row_nan_store(int H4, int lane, float* __restrict__ out) {
  const float n = __int_as_float(0x7fc00000);
  for (int c = lane; c < H4; c += 64) *reinterpret_cast<float4*>(out + 4 * c) = make_float4(n, n, n, n);
}

// One wave per token row, four rows per block. The row's sequence is found by bisection over cu (wave-uniform).
// An id outside [0, vocab), a position outside [0, max_pos) or a cu that does not bracket the row writes a NaN row.
__global__ void __launch_bounds__(256) k_sbert_embed_ln(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                        int S, int T, const float* __restrict__ word, int vocab,
                                                        const float* __restrict__ pos, int max_pos,
                                                        const float* __restrict__ type0,
                                                        const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                        float eps, int H4, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  int lo = 0, hi = S;  // the last s with cu[s] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= t) lo = mid; else hi = mid;
  }
  const int p = t - cu[lo];
  const int id = ids[t];
  float* orow = out + (int64_t)t * 4 * H4;
  if (id < 0 || id >= vocab || p < 0 || p >= max_pos || t >= cu[lo + 1]) {
    row_nan_store(H4, lane, orow);
    return;
  }
  const float* wr = word + (int64_t)id * 4 * H4;
  const float* pr = pos + (int64_t)p * 4 * H4;
  float4 v[kSbRowF4];
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) {
    const int c = lane + 64 * i;
    if (c < H4) {
      const float4 a = ld4c(wr + 4 * c), b = ld4c(pr + 4 * c), d = ld4c(type0 + 4 * c);
      v[i] = make_float4((a.x + b.x) + d.x, (a.y + b.y) + d.y, (a.z + b.z) + d.z, (a.w + b.w) + d.w);
    } else {
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  row_ln_store(v, H4, lane, ln_w, ln_b, eps, orow);
}

// out = LayerNorm(x + res), one wave per row. A lane reads exactly the elements it writes, so out may be x or res.
__global__ void __launch_bounds__(256) k_sbert_add_ln(const float* x, const float* res,
                                                      const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                      float eps, int T, int H4, float* out) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const float* xr = x + (int64_t)t * 4 * H4;
  const float* rr = res + (int64_t)t * 4 * H4;
  float4 v[kSbRowF4];
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) {
    const int c = lane + 64 * i;
    if (c < H4) {
      const float4 a = ld4c(xr + 4 * c), b = ld4c(rr + 4 * c);
      v[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    } else {
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  row_ln_store(v, H4, lane, ln_w, ln_b, eps, out + (int64_t)t * 4 * H4);
}

// ---- self-attention --------------------------------------------------------------------------------------------
// k_dec_f32's streaming softmax (hvae_decoder.hip) with separate K and V: a block is one (sequence, 64-query chunk)
// work item of one head, 4 waves x 16 queries; the sequence's keys pass through LDS in 16-key K and V tiles,
// double buffered, rows padded to DH + 4 floats (16-B aligned rows; both MFMA reads below are bank-conflict free:
// (DH + 4) c16 modulo 64 runs through 16 distinct multiples of 4 for DH = 32 and 64, so the K read's c16 (DH + 4) + q
// hits 64 banks; the V read's 4 q (DH + 4) + c16 is 16 q + c16 modulo 64).
//   S^T tile = K_tile Q^T  (A = K[key c16][4 ks + q], B = Q[query c16][4 ks + q]; two accumulator chains, even and
//                           odd ks, added at the end)  -> lane (q, c16) holds keys 4 q + r of query c16
//   O^T     += V_tile^T P^T (A = V[key 4 q + r][16 d + c16], B = p[r])
// Keys past the sequence's end score -inf (their V rows are staged as zeros). Query rows past the end load zeros
// and are never stored: in the packed layout they are the next sequence's tokens. The sums over keys run in tile
// order; inside a tile the MFMA's k order, then the xor butterfly over the four lane groups.
//
// BIAS (MPNet's relative-position bias): score (query i, key j) += rel[head][(j - i) + L - 1], rel [heads, 2 L - 1],
// after the scale. A chunk's queries c 64 .. c 64 + 63 against keys 0 .. 16 ntiles - 1 need the deltas
// -(c 64 + 63) .. 16 ntiles - 1 - c 64: that window of the head's row is staged once into relw, relw[x] = the bias
// of delta x - (c 64 + 63), before the first barrier. An entry outside the table is staged as 0: it belongs to a
// query or a key past the sequence's end (len <= L), whose score is never stored or is -inf. Lane (q, c16) of wave w
// reads relw[63 + 4 q - 16 w - c16 + 16 t + r], r = 0 .. 3: the 32 lanes of a ds_read_b32 group span 20 consecutive
// floats, so lanes either share an address (broadcast) or hit distinct banks. Without BIAS rel and L are not read
// and relw is not allocated.
template <int DH, bool BIAS>
__global__ void __launch_bounds__(256) k_sbert_attn(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                    int S, int T, int H, const int32_t* __restrict__ work,
                                                    float scale, float* __restrict__ ctx,
                                                    const float* __restrict__ rel, int L) {
  constexpr int KS = DH / 4;
  constexpr int DB = DH / 16;
  constexpr int LD = DH + 4;
  constexpr int TF = kSbTK * LD;        // floats per K or V tile
  constexpr int Q4 = DH / 4;            // float4 per row
  constexpr int LPT = 2 * kSbTK * Q4 / 256;
  static_assert(LPT * 256 == 2 * kSbTK * Q4, "the K and V tiles are a whole number of float4 per thread");
  __shared__ __attribute__((aligned(16))) float lds[2][2 * TF];
  __shared__ float relw[BIAS ? kSbRelN : 1];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c16 = lane & 15;
  const int seq = work[2 * blockIdx.x], chunk = work[2 * blockIdx.x + 1];
  if (seq < 0 || seq >= S) return;  // block-uniform: before any barrier
  const int base = cu[seq], len = cu[seq + 1] - base;
  if (base < 0 || len <= 0 || len > kSbMaxLen || base + len > T) return;
  if (chunk < 0 || chunk * kSbQB >= len) return;
  if (BIAS && len > L) return;  // the table does not cover the sequence: untouched rows
  const int head = blockIdx.y;
  const int ld3 = 3 * H;
  const float* qkv_s = qkv + (int64_t)base * ld3 + head * DH;

  const int q0 = chunk * kSbQB + w * kSbQW;
  const bool wave_active = q0 < len;
  const int qrow = q0 + c16;
  float uf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) uf[ks] = (qrow < len) ? qkv_s[(int64_t)qrow * ld3 + 4 * ks + q] : 0.f;

  sb_f32x4 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o[d] = sb_f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;

  float4 stage[LPT];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = tid + 256 * i;
      const int which = c / (kSbTK * Q4), rem = c % (kSbTK * Q4);
      const int row = t * kSbTK + rem / Q4, c4 = rem % Q4;
      stage[i] = (row < len) ? ld4c(qkv_s + (int64_t)row * ld3 + (1 + which) * H + 4 * c4)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto lstore = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = tid + 256 * i;
      const int which = c / (kSbTK * Q4), rem = c % (kSbTK * Q4);
      *reinterpret_cast<float4*>(buf + which * TF + (rem / Q4) * LD + 4 * (rem % Q4)) = stage[i];
    }
  };

  const int ntiles = (len + kSbTK - 1) / kSbTK;
  if constexpr (BIAS) {
    const float* relh = rel + (int64_t)head * (2 * L - 1);
    const int g0 = L - 1 - (chunk * kSbQB + kSbQB - 1);  // the table index of relw[0]
    for (int x = tid; x < ntiles * kSbTK + kSbQB; x += 256) {  // at most 512 + 64 = kSbRelN
      const int g = g0 + x;
      relw[x] = (g >= 0 && g <= 2 * L - 2) ? relh[g] : 0.f;
    }
  }
  const int rb = kSbQB - 1 + 4 * q - kSbQW * w - c16;  // 0 .. 75; + 16 t + r <= 574
  gload(0);
  lstore(lds[0]);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) gload(t + 1);
    const float* kb = lds[cur];
    const float* vb = lds[cur] + TF;
    if (wave_active) {
      sb_f32x4 s0 = sb_f32x4{0.f, 0.f, 0.f, 0.f}, s1 = sb_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ks += 2) {
        s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[c16 * LD + 4 * ks + q], uf[ks], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[c16 * LD + 4 * ks + 4 + q], uf[ks + 1], s1, 0, 0, 0);
      }
      const int kbase = t * kSbTK + 4 * q;
      float sc[4];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (BIAS)
          sc[r] = (kbase + r < len) ? (s0[r] + s1[r]) * scale + relw[rb + t * kSbTK + r] : -INFINITY;
        else
          sc[r] = (kbase + r < len) ? (s0[r] + s1[r]) * scale : -INFINITY;
        mx = fmaxf(mx, sc[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // tile 0 holds key 0 of a non-empty sequence, so mx is finite from the first tile on
      const float mn = fmaxf(m, mx);
      if (__any(mn > m)) {
        const float alpha = __expf(m - mn);  // exp(-inf) = 0 on the first tile
        lsum *= alpha;
#pragma unroll
        for (int d = 0; d < DB; ++d) o[d] *= alpha;
        m = mn;
      }
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = __expf(sc[r] - m);
        lsum += p[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int d = 0; d < DB; ++d)
          o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[(4 * q + r) * LD + 16 * d + c16], p[r], o[d], 0, 0, 0);
    }
    if (more) lstore(lds[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }

  if (!wave_active) return;  // wave-uniform
  float ltot = lsum + __shfl_xor(lsum, 16, 64);
  ltot += __shfl_xor(ltot, 32, 64);
  if (qrow >= len) return;
  const float inv = 1.0f / ltot;
  // O^T block d: lane holds columns 16 d + 4 q + r of query c16
  float* crow = ctx + (int64_t)(base + qrow) * H + head * DH;
#pragma unroll
  for (int d = 0; d < DB; ++d)
    *reinterpret_cast<float4*>(crow + 16 * d + 4 * q) =
        make_float4(o[d][0] * inv, o[d][1] * inv, o[d][2] * inv, o[d][3] * inv);
}

// ---- mean pooling and L2 normalisation -------------------------------------------------------------------------
// One block per sequence. Wave g sums rows g, g + 4, ... of the sequence in ascending order (lane l owns the float4
// columns l, l + 64, ...); the four partial rows meet in LDS and are added as ((g0 + g1) + g2) + g3. The mean divides
// by the row count; the squared norm is each thread's own columns ascending, then block_sum. A sequence whose cu
// entries do not lie in [0, T] or that is empty writes a NaN row.
__global__ void __launch_bounds__(256) k_sbert_pool_norm(const float* __restrict__ x, const int32_t* __restrict__ cu,
                                                         int T, int H4, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float part[4][kSbMaxH];
  __shared__ float red[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int base = cu[s], len = cu[s + 1] - base;
  float* orow = out + (int64_t)s * 4 * H4;
  if (base < 0 || len <= 0 || base + len > T) {  // block-uniform
    if (g == 0) row_nan_store(H4, lane, orow);
    return;
  }
  float4 acc[kSbRowF4];
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r = g; r < len; r += 4) {
    const float* xr = x + (int64_t)(base + r) * 4 * H4;
#pragma unroll
    for (int i = 0; i < kSbRowF4; ++i) {
      const int c = lane + 64 * i;
      if (c < H4) {
        const float4 a = ld4c(xr + 4 * c);
        acc[i].x += a.x; acc[i].y += a.y; acc[i].z += a.z; acc[i].w += a.w;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) {
    const int c = lane + 64 * i;
    if (c < H4) *reinterpret_cast<float4*>(&part[g][4 * c]) = acc[i];
  }
  __syncthreads();
  const float invn = 1.0f / (float)len;
  float mean[kSbRowF4];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) {
    const int c = tid + 256 * i;
    mean[i] = 0.f;
    if (c < 4 * H4) {
      mean[i] = (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) * invn;
      ss += mean[i] * mean[i];
    }
  }
  const float nrm = fmaxf(sqrtf(block_sum<256>(ss, red)), 1e-12f);
#pragma unroll
  for (int i = 0; i < kSbRowF4; ++i) {
    const int c = tid + 256 * i;
    if (c < 4 * H4) orow[c] = mean[i] / nrm;
  }
}

}  // namespace hvae

using namespace hvae;

static bool sbert_h_ok(int64_t H) { return H >= 4 && H <= kSbMaxH && H % 4 == 0; }
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int hvae_sbert_supported(int64_t H, int64_t heads, int64_t max_len) {
  if (!sbert_h_ok(H) || heads <= 0 || H % heads != 0) return 0;
  const int64_t dh = H / heads;
  return (dh == 32 || dh == 64) && max_len >= 1 && max_len <= kSbMaxLen;
}

extern "C" int hvae_sbert_embed_ln(const int32_t* ids, const int32_t* cu, int64_t S, int64_t T, const float* word,
                                   int64_t vocab, const float* pos, int64_t max_pos, const float* type0,
                                   const float* ln_w, const float* ln_b, float eps, int64_t H, float* out,
                                   void* stream) {
  HVAE_REQUIRE(sbert_h_ok(H), "hvae_sbert_embed_ln: H = %lld is not served (a multiple of 4 in 4 .. %d)",
               (long long)H, kSbMaxH);
  HVAE_REQUIRE(S >= 1 && T >= 1 && S <= T && T < (1LL << 31) / (3 * H), "hvae_sbert_embed_ln: S = %lld, T = %lld",
               (long long)S, (long long)T);
  HVAE_REQUIRE(vocab >= 1 && vocab < (1LL << 31) && max_pos >= 1 && max_pos < (1LL << 31),
               "hvae_sbert_embed_ln: vocab = %lld, max_pos = %lld", (long long)vocab, (long long)max_pos);
  HVAE_REQUIRE(ids && cu && word && pos && type0 && ln_w && ln_b && out, "hvae_sbert_embed_ln: null pointer");
  HVAE_REQUIRE(al16(word) && al16(pos) && al16(type0) && al16(ln_w) && al16(ln_b) && al16(out),
               "hvae_sbert_embed_ln: the float arrays must be 16-byte aligned");
  k_sbert_embed_ln<<<(unsigned)cdiv(T, 4), 256, 0, as_stream(stream)>>>(ids, cu, (int)S, (int)T, word, (int)vocab, pos,
                                                                      (int)max_pos, type0, ln_w, ln_b, eps,
                                                                      (int)(H / 4), out);
  HVAE_LAUNCH_CHECK("k_sbert_embed_ln");
  return HVAE_OK;
}

extern "C" int hvae_sbert_add_ln(const float* x, const float* res, const float* ln_w, const float* ln_b, float eps,
                                 int64_t T, int64_t H, float* out, void* stream) {
  HVAE_REQUIRE(sbert_h_ok(H), "hvae_sbert_add_ln: H = %lld is not served (a multiple of 4 in 4 .. %d)", (long long)H,
               kSbMaxH);
  HVAE_REQUIRE(T >= 1 && T < (1LL << 31) / (3 * H), "hvae_sbert_add_ln: T = %lld", (long long)T);
  HVAE_REQUIRE(x && res && ln_w && ln_b && out, "hvae_sbert_add_ln: null pointer");
  HVAE_REQUIRE(al16(x) && al16(res) && al16(ln_w) && al16(ln_b) && al16(out),
               "hvae_sbert_add_ln: the arrays must be 16-byte aligned");
  k_sbert_add_ln<<<(unsigned)cdiv(T, 4), 256, 0, as_stream(stream)>>>(x, res, ln_w, ln_b, eps, (int)T, (int)(H / 4),
                                                                    out);
  HVAE_LAUNCH_CHECK("k_sbert_add_ln");
  return HVAE_OK;
}

// The two attention entry points share their checks and launch; fn names the caller in the messages.
template <bool BIAS>
static int sbert_attention_launch(const char* fn, const float* qkv, const int32_t* cu, int64_t S, int64_t T, int64_t H,
                                  int64_t heads, const int32_t* work, int64_t n_work, const float* rel, int64_t L,
                                  float* ctx, void* stream) {
  HVAE_REQUIRE(hvae_sbert_supported(H, heads, 1),
               "%s: H = %lld with %lld heads is not served (head width 32 or 64, H <= %d)", fn, (long long)H,
               (long long)heads, kSbMaxH);
  HVAE_REQUIRE(S >= 1 && T >= 1 && S <= T && T < (1LL << 31) / (3 * H), "%s: S = %lld, T = %lld", fn, (long long)S,
               (long long)T);
  HVAE_REQUIRE(n_work >= 1 && n_work < (1LL << 31) && heads <= 65535, "%s: n_work = %lld", fn, (long long)n_work);
  HVAE_REQUIRE(!BIAS || (L >= 1 && L <= kSbMaxLen), "%s: L = %lld is not served (1 .. %d)", fn, (long long)L,
               kSbMaxLen);
  HVAE_REQUIRE(qkv && cu && work && ctx && qkv != ctx && (!BIAS || rel), "%s: null or aliased pointer", fn);
  HVAE_REQUIRE(al16(qkv) && al16(ctx), "%s: qkv and ctx must be 16-byte aligned", fn);
  const int64_t dh = H / heads;
  const float scale = (float)(1.0 / sqrt((double)dh));
  const dim3 grid((unsigned)n_work, (unsigned)heads);
  if (dh == 32)
    k_sbert_attn<32, BIAS><<<grid, 256, 0, as_stream(stream)>>>(qkv, cu, (int)S, (int)T, (int)H, work, scale, ctx,
                                                                rel, (int)L);
  else
    k_sbert_attn<64, BIAS><<<grid, 256, 0, as_stream(stream)>>>(qkv, cu, (int)S, (int)T, (int)H, work, scale, ctx,
                                                                rel, (int)L);
  HVAE_LAUNCH_CHECK("k_sbert_attn");
  return HVAE_OK;
}

extern "C" int hvae_sbert_attention(const float* qkv, const int32_t* cu, int64_t S, int64_t T, int64_t H,
                                    int64_t heads, const int32_t* work, int64_t n_work, float* ctx, void* stream) {
  return sbert_attention_launch<false>("hvae_sbert_attention", qkv, cu, S, T, H, heads, work, n_work, nullptr, 0, ctx,
                                       stream);
}

extern "C" int hvae_sbert_attention_relbias(const float* qkv, const int32_t* cu, int64_t S, int64_t T, int64_t H,
                                            int64_t heads, const int32_t* work, int64_t n_work, const float* rel,
                                            int64_t L, float* ctx, void* stream) {
  return sbert_attention_launch<true>("hvae_sbert_attention_relbias", qkv, cu, S, T, H, heads, work, n_work, rel, L,
                                      ctx, stream);
}

extern "C" int hvae_sbert_pool_norm(const float* x, const int32_t* cu, int64_t S, int64_t T, int64_t H, float* out,
                                    void* stream) {
  HVAE_REQUIRE(sbert_h_ok(H), "hvae_sbert_pool_norm: H = %lld is not served (a multiple of 4 in 4 .. %d)",
               (long long)H, kSbMaxH);
  HVAE_REQUIRE(S >= 1 && T >= 1 && S <= T && T < (1LL << 31) / (3 * H), "hvae_sbert_pool_norm: S = %lld, T = %lld",
               (long long)S, (long long)T);
  HVAE_REQUIRE(x && cu && out && x != out, "hvae_sbert_pool_norm: null or aliased pointer");
  HVAE_REQUIRE(al16(x) && al16(out), "hvae_sbert_pool_norm: x and out must be 16-byte aligned");
  k_sbert_pool_norm<<<(unsigned)S, 256, 0, as_stream(stream)>>>(x, cu, (int)T, (int)(H / 4), out);
  HVAE_LAUNCH_CHECK("k_sbert_pool_norm");
  return HVAE_OK;
}
