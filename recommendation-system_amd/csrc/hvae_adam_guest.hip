// hvae_adam_guest.hip -- the recorded W1t update (hvae_optim.hip's k_adam_pending) as a guest kernel beside the
// decoder sweep: hvae_adam_lazy_pending_guest, and the host query whether it fits there.
//
// The d = 768 sweep's block holds two waves of 240 allocated registers on every SIMD and nearly all of the CU's
// LDS, so a 256-thread block of k_adam_pending cannot share a CU with it; what the sweep leaves free is 32
// registers per lane and six wave slots on each SIMD, the scalar registers and most of HBM. k_adam_pending_guest
// is written to fit there: one 64-lane wave a block, no LDS, no barrier, at most 32 VGPRs
// (tests/test_adam_guest_fit_cpu.py reads the code object). This file is built with -fno-slp-vectorize (Makefile):
// packed two-float instructions keep every wave-uniform constant in a register pair and took the kernel from 26
// to 34 VGPRs.
#include <algorithm>

#include "hvae_common.h"
#include "hvae_adam.h"

namespace hvae {

// A block takes kGuestRows whole rows, one after the other; lane l takes float2 columns l, l + 64, ... What a row
// shares -- its index, stamp, replay range, the header's fields, the step table's entries -- is wave-uniform and
// lives in scalar registers (readfirstlane; tab[] and the header are read with scalar loads), so the vector
// registers hold p, m, v, g, the column's offset and the element update's temporaries. The wave reads last_step[j]
// before its first column and one lane writes it after the last store. Same rows, same claim test, same stamp and
// the same float operations (col_math_lazy) as k_adam_pending: p, m, v and last_step are bitwise its.
// Blocks are short and the grid is sized by the work, not persistent: a guest wave that stayed on a CU for
// milliseconds could keep a sweep block from starting there. The recorded rows are walked with k_adam_pending's
// grid stride (max_rows sizes the grid, hdr->n bounds the walk), so a grid sized for fewer rows than were recorded
// still takes every one of them; with max_rows right a block takes one group of kGuestRows rows.
// (Non-temporal loads and stores of p, m, v were tried and lost 0.04 ms a step: profiles/adam_guest_ab.jsonl.)
constexpr int kGuestRows = 4;
typedef float guest_f2 __attribute__((ext_vector_type(2)));
// The 8 bytes at byte offset `off` of a row, as the x, y of a float4 column whose z, w nobody reads: a wave-uniform
// row base and one 32-bit lane offset for p, m, v and g. With float4 columns the kernel took 44 to 54 VGPRs; a
// lane's float2 takes the same element updates, so no value changes.
__device__ __forceinline__ float4 guest_ld(const float* row, uint32_t off) {
  const float2 x = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(row) + off);
  return make_float4(x.x, x.y, 0.f, 0.f);
}
__device__ __forceinline__ void guest_st(float* row, uint32_t off, const float4& x) {
  *reinterpret_cast<float2*>(reinterpret_cast<char*>(row) + off) = make_float2(x.x, x.y);
}
__device__ __forceinline__ int guest_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// row j (wave-uniform) through col_math_lazy. STEP: replay to `to`, then the recorded step with coef * its gradient
// row grow; else through `to` with g = 0. One column at a time, its stores issued before the next column's loads.
template <bool STEP>
__device__ __forceinline__ void guest_row(const AdamArgs& a, const float2* __restrict__ tab, float* __restrict__ p,
                                          float* __restrict__ m, float* __restrict__ v, int64_t j, int H4,
                                          const float* grow, float coef, int from, int pst, int to, const AdamK& k) {
  float* pr = p + j * 4 * H4;
  float* mr = m + j * 4 * H4;
  float* vr = v + j * 4 * H4;
  const uint32_t end = 16u * (uint32_t)H4;
#pragma clang loop unroll(disable)
  for (uint32_t off = 8u * threadIdx.x; off < end; off += 8u * kWave) {
    ColState cs{guest_ld(pr, off), guest_ld(mr, off), guest_ld(vr, off)};
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (STEP) {
      // (the recorded pointer is to global memory: said so, the load takes a scalar base and the lane's offset)
      typedef const __attribute__((address_space(1))) guest_f2* gptr2;
      const guest_f2 x = *(gptr2)(reinterpret_cast<const char*>(grow) + off);
      g.x = x[0] * coef; g.y = x[1] * coef;
    }
    col_math_lazy(a, tab, cs, from, pst, to, STEP, k, g);
    // the stores' offset is the loads', handed over opaquely: the compiler then forms the three store addresses
    // here, from the scalar bases, instead of carrying three 64-bit lane addresses through the replay loop
    uint32_t soff = off;
    __asm__ volatile("" : "+v"(soff));
    guest_st(pr, soff, cs.p);
    guest_st(mr, soff, cs.m);
    guest_st(vr, soff, cs.v);
    __asm__ volatile("" ::: "memory");
  }
}

__global__ void __launch_bounds__(kWave) k_adam_pending_guest(AdamArgs a, const float2* __restrict__ tab,
                                                              float* __restrict__ p, float* __restrict__ m,
                                                              float* __restrict__ v, int32_t* __restrict__ last_step,
                                                              const int32_t* __restrict__ pend_slot,
                                                              const int32_t* __restrict__ pend_item,
                                                              const PendHdr* __restrict__ hdr, int64_t N, int H4,
                                                              int nb_rows, int period) {
  const int64_t t64 = hdr->t;
  if (t64 <= 0 || t64 != load_step(a.step_dev)) return;  // the record is live only at its own step
  const int t = (int)t64;
  const AdamK k = adam_consts_tab(a, tab[t]);
  if ((int)blockIdx.x < nb_rows) {
    const float* rows = hdr->rows;
    const int64_t ld = hdr->ld;
    const float coef = hdr->coef;
    const int nu = hdr->n;
    // groups of kGuestRows slots, strided by the row blocks: every recorded row is taken whatever max_rows was
#pragma clang loop unroll(disable)
    for (int64_t s0 = (int64_t)blockIdx.x * kGuestRows; s0 < nu; s0 += (int64_t)nb_rows * kGuestRows) {
#pragma clang loop unroll(disable)
      for (int r = 0; r < kGuestRows; ++r) {
        const int s = (int)s0 + r;
        if (s >= nu) break;
        const int j = pend_item[s];
        const int32_t ls = guest_uniform(last_step[j]);
        if (!(ls & kPendBit) || guest_uniform(pend_slot[j]) != s) continue;  // a catch-up claimed it
        guest_row<true>(a, tab, p, m, v, j, H4, rows + (int64_t)s * ld, coef, ls_mv(ls), ls_p(ls), t - 1, k);
        if (threadIdx.x == 0) last_step[j] = t;
      }
    }
  } else {
    const int64_t chunk = (N + period - 1) / period;
    const int64_t r0 = (int64_t)((t - 1) % period) * chunk, r1 = min(N, r0 + chunk);
#pragma clang loop unroll(disable)
    for (int r = 0; r < kGuestRows; ++r) {
      const int64_t j = r0 + (int64_t)((int)blockIdx.x - nb_rows) * kGuestRows + r;
      if (j >= r1) break;
      const int32_t ls = guest_uniform(last_step[j]);
      if ((ls & kPendBit) || ls_mv(ls) >= t) continue;
      // through step t with g = 0 (k_adam_pending's sweep range); steps p already has move m and v alone
      guest_row<false>(a, tab, p, m, v, j, H4, nullptr, 0.f, ls_mv(ls), ls_p(ls), t, k);
      if (threadIdx.x == 0) last_step[j] = t;
    }
  }
}

// The guest's head start for the sweep: one wave that sleeps a fixed time on the constant 100-MHz clock (a bounded
// loop, k_probe_hold's; not a spin on memory) in front of the guest on its stream, so that the sweep's blocks are
// resident when the guest's first blocks look for room. If the guest comes first all the same, the sweep's
// displaced blocks start once the short guest blocks drain.
__global__ void k_guest_hold(uint64_t ticks) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

}  // namespace hvae

using namespace hvae;

// The hold as a call of its own, so that hvae_adam_lazy_pending_guest carries no placement policy: the trainer
// launches it in front of the guest (hvae/executor.py GUEST_HOLD_US has the length and the trace it comes from).
extern "C" int hvae_adam_guest_hold(int64_t us, void* stream) {
  HVAE_REQUIRE(us >= 0 && us <= 1000, "hvae_adam_guest_hold: 0 <= us <= 1000");
  if (us == 0) return HVAE_OK;
  k_guest_hold<<<1, kWave, 0, as_stream(stream)>>>((uint64_t)us * 100);
  HVAE_LAUNCH_CHECK("k_guest_hold");
  return HVAE_OK;
}

extern "C" int hvae_adam_lazy_pending_guest(const hvae_adam* cfg, const float* tab, float* p, float* m, float* v,
                                            int32_t* last_step, int64_t N, int64_t H, int64_t max_rows,
                                            const hvae_adam_pend* pend, void* stream) {
  HVAE_REQUIRE(cfg && cfg->step_dev && tab && p && m && v && last_step, "hvae_adam_lazy_pending_guest: bad args");
  HVAE_REQUIRE(pend && pend->slot_of && pend->item_of && pend->hdr && H % 4 == 0 && N >= 0 && max_rows >= 0,
               "hvae_adam_lazy_pending_guest: bad args");
  HVAE_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0,
               "hvae_adam_lazy_pending_guest: 16-B alignment required");
  HVAE_REQUIRE(H / 4 <= (1 << 24) && N <= ((int64_t)1 << 31) - 1, "hvae_adam_lazy_pending_guest: H or N too large");
  if (N == 0) return HVAE_OK;
  // the grid follows the work: the rows max_rows expects (more are taken by the row blocks' stride) and the sweep
  // range, kGuestRows rows a block
  const int64_t b_rows = std::max<int64_t>(1, cdiv(std::min(max_rows, N), kGuestRows));
  const int period = hvae_adam_lazy_sweep_period(N);
  const int64_t b_sweep = std::max<int64_t>(1, cdiv(cdiv(N, period), kGuestRows));
  ProbeScope probe("adam_pending", as_stream(stream));
  k_adam_pending_guest<<<(unsigned)(b_rows + b_sweep), kWave, 0, as_stream(stream)>>>(
      to_args(cfg), (const float2*)tab, p, m, v, last_step, pend->slot_of, pend->item_of, (const PendHdr*)pend->hdr, N,
      (int)(H / 4), (int)b_rows, period);
  HVAE_LAUNCH_CHECK("k_adam_pending_guest");
  return HVAE_OK;
}

// Whether guest waves fit on a SIMD beside the sweep's, from the two kernels' footprints: registers are allocated
// in granules of 8 per lane out of 512 a SIMD, a CU has 160 KiB of LDS and 32 wave slots (8 a SIMD, four SIMDs).
// Returns how many guest waves fit on one SIMD beside the sweep's (0: none).
extern "C" int hvae_adam_guest_fit_calc(int sweep_waves_per_simd, int sweep_regs, int64_t sweep_lds_bytes,
                                        int guest_regs, int64_t guest_lds_bytes) {
  if (sweep_waves_per_simd < 0 || sweep_regs < 0 || guest_regs <= 0 || sweep_lds_bytes < 0 || guest_lds_bytes < 0)
    return 0;
  auto alloc = [](int r) { return (r + 7) / 8 * 8; };
  const int free_regs = 512 - sweep_waves_per_simd * alloc(sweep_regs);
  if (free_regs < alloc(guest_regs) || sweep_lds_bytes > 160 * 1024) return 0;
  int waves = free_regs / alloc(guest_regs);
  waves = std::min(waves, 32 / 4 - sweep_waves_per_simd);  // 32 waves a CU: the sweep's and the guest's together
  if (guest_lds_bytes > 0) {
    // a guest block is one wave, and each brings its block's LDS; four SIMDs share the CU's
    const int64_t free_lds = 160 * 1024 - sweep_lds_bytes;
    waves = (int)std::min<int64_t>(waves, free_lds / guest_lds_bytes / 4);
  }
  return std::max(waves, 0);
}

extern "C" int hvae_adam_pending_guest_fits(int dtype, int64_t B, int64_t N, int64_t D) {
  SweepFootprint f{};
  if (!dec_sweep_footprint(dtype, B, N, D, &f)) return 0;  // no sweep there whose code object this build reads
  hipFuncAttributes ga{};
  if (hipFuncGetAttributes(&ga, (const void*)k_adam_pending_guest) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  if (ga.localSizeBytes != 0) return 0;  // scratch: the guest must not spill
  return hvae_adam_guest_fit_calc(f.waves_per_simd, f.regs, (int64_t)f.lds_bytes, ga.numRegs,
                                  (int64_t)ga.sharedSizeBytes) > 0;
}
