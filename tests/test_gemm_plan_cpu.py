"""The fp32 GEMM's kernel choice, through the host plan query (no GPU needed).

hvae_gemm_f32_plan / hvae_gemm_f32_pair_plan answer from the same function the launchers run from
(csrc/hvae_gemm.hip plan_one / plan_pair), so what is asserted here is what a launch does.

The scan finds 63 single-launch keys and 102 pair keys on the grid. Instantiations of the dispatch macros that no
grid point reaches in the product build (also in DESIGN.md, under the train step's kernel table; none is removed
here):
  * k_gemm_f32<false, true, 32, 32, 1> and <false, true, 64, 64, 1>: nst_class keeps A B^T long k ranges on the ring
    (nst 4), so HVAE_GEMM_CALL's one-stage branch is dead for that transposition.
  * k_gemm_dma<true, false, 32, 32>: dma_tile refuses the 32-square tile for trans_a without trans_b (those weight
    gradients stay on the fast kernel) unless HVAE_GEMM_DMA_TILE forces it (A/B build). With it go
    k_gemm_dma_pair<32, 64> and <32, 32>, whose first half is that instance.
  * k_gemm_dma<true, false, 64, 32> and k_gemm_dma<true, true, 64, 32>: the 64 x 32 tile is never planned with trans_a.
  * k_gemm_f32_pair<64, 64, 4, 4>: a weight gradient in 64-square tiles over a short k range needs 512 tiles and a
    batch of at most 128 rows; its data gradient then has a long K = M, whose k ranges come down to 128 only with
    16 splits, and 64-square tiles at long K (24 or more of them) never get that many.
  * k_gemm_fast<true, false, 64, 64> is reached only without split-K (K = 1024, or no workspace): a whole-tile
    weight gradient with more than 256 32-square tiles and K > 1024 splits, and then dma_tile's 64-square tile
    count (times the splits) takes it first. The instantiation runs; its split-K path never does.
(k_gemm_fast<false, ...> exists only in the A/B build, behind HVAE_GEMM_FAST_SHORT.)
All 12 k_gemm_mixed_pair instantiations, the other 15 of k_gemm_f32_pair and k_gemm_dma_pair<64, 64> and <64, 32>
are reached.
"""
import ctypes as C

import pytest

import gemm_plan_cases as G


@pytest.fixture(scope="module")
def L():
    from hvae import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def single_scan(L):
    """key -> one grid point that plans to it, over the whole grid."""
    found = {}
    for ta, tb in G.TRANS:
        for M in G.GRID_MN:
            for N in G.GRID_MN:
                for K in G.GRID_K:
                    for addr in (G.ALIGNED, G.MISALIGNED):
                        for ws in (True, False):
                            p = G.single_plan(L, ta, tb, M, N, K, a=addr, b=addr, ws=ws)
                            found.setdefault(G.single_key(ta, tb, p), (ta, tb, M, N, K, addr == G.ALIGNED, ws))
    return found


@pytest.fixture(scope="module")
def pair_scan(L):
    found = {}
    for B in G.GRID_K:
        for M in G.GRID_MN:
            for N in G.GRID_MN:
                for Kx in dict.fromkeys((N,) + G.PAIR_KX):
                    for ws in ("own", "shared", "none"):
                        for addr in (G.ALIGNED, G.MISALIGNED):
                            w, x = G.pair_descs(L, B, M, N, Kx, ws=ws, a=addr)
                            kind, pw, px = G.pair_plan(L, w, x)
                            found.setdefault(G.pair_key(kind, pw, px), (B, M, N, Kx, ws, addr == G.ALIGNED))
    return found


def test_single_scan_is_covered(single_scan):
    """Every kernel instance a single launch can reach on the grid has a case in the GPU test's table."""
    have = {c[-1] for c in G.SINGLE_CASES}
    missing = {k: v for k, v in single_scan.items() if k not in have}
    assert not missing, f"plan keys without a case in gemm_plan_cases.SINGLE_CASES (key: a grid point): {missing}"


def test_single_cases_plan_as_recorded(L):
    for ta, tb, M, N, K, ws, aligned, key in G.SINGLE_CASES + G.EXTRA_SINGLE_CASES:
        addr = G.ALIGNED if aligned else G.MISALIGNED
        got = G.single_key(ta, tb, G.single_plan(L, ta, tb, M, N, K, a=addr, b=addr, ws=bool(ws)))
        assert got == key, f"{(ta, tb, M, N, K, ws, aligned)} now plans to {got}, the table records {key}"
    keys = [c[-1] for c in G.SINGLE_CASES]
    assert len(keys) == len(set(keys))


def test_pair_scan_is_covered(pair_scan):
    have = {c[-1] for c in G.PAIR_CASES}
    missing = {k: v for k, v in pair_scan.items() if k not in have}
    assert not missing, f"pair keys without a case in gemm_plan_cases.PAIR_CASES (key: a grid point): {missing}"
    assert {k[0] for k in pair_scan} == {0, 1, 2, 3}


def test_pair_cases_plan_as_recorded(L):
    for B, M, N, Kx, ws, aligned, key in G.PAIR_CASES:
        w, x = G.pair_descs(L, B, M, N, Kx, ws=ws, a=G.ALIGNED if aligned else G.MISALIGNED)
        got = G.pair_key(*G.pair_plan(L, w, x))
        assert got == key, f"{(B, M, N, Kx, ws, aligned)} now plans to {got}, the table records {key}"
    # both halves split-K into one shared workspace: two launches
    w, x = G.pair_descs(L, *G.PAIR_SHARED_SPLIT, ws="shared")
    kind, pw, px = G.pair_plan(L, w, x)
    assert kind == 0 and pw.splits > 1 and px.splits > 1


def test_pair_halves_are_the_single_plans_when_unfused(L):
    """launch_kind 0 reports what each half's own hvae_gemm_f32 call plans."""
    for B, M, N, Kx, ws, aligned, key in G.PAIR_CASES:
        if key[0] != 0:
            continue
        w, x = G.pair_descs(L, B, M, N, Kx, ws=ws, a=G.ALIGNED if aligned else G.MISALIGNED)
        _, pw, px = G.pair_plan(L, w, x)
        for d, p in ((w, pw), (x, px)):
            q = G.single_plan(L, d.trans_a, d.trans_b, d.M, d.N, d.K, a=d.A, lda=d.lda, b=d.B, ldb=d.ldb,
                              ws=d.ws is not None, ws_bytes=d.ws_bytes)
            assert G.plan_tuple(p) == G.plan_tuple(q)


def test_train_step_plans_are_pinned(L):
    """The train step's own GEMMs (hvae/executor.py) at the Syn-10M shard's model, B = 4096 and B = 64."""
    for (ta, tb, M, N, K), want in G.PINS.items():
        assert G.plan_tuple(G.single_plan(L, ta, tb, M, N, K)) == want, (ta, tb, M, N, K)
    for (B, M, N, Kx), (kind, pw, px) in G.PAIR_PINS.items():
        w, x = G.pair_descs(L, B, M, N, Kx, ws="shared")
        k, gw, gx = G.pair_plan(L, w, x)
        assert (k, G.plan_tuple(gw), G.plan_tuple(gx)) == (kind, pw, px), (B, M, N, Kx)
    assert len(G.PINS) >= 12 and len(G.PAIR_PINS) == 6


def test_degenerate_inputs_answer(L):
    from hvae import _lib
    # empty products: nothing is launched
    for M, N in ((0, 64), (64, 0), (0, 0)):
        p = G.single_plan(L, 1, 0, M, N, 4096)
        assert (p.bm, p.bn, p.splits) == (0, 0, 1)
    # K = 0: one k range of nothing, on the register-staged kernel
    for ta, tb in G.TRANS:
        p = G.single_plan(L, ta, tb, 130, 67, 0)
        assert (p.family, p.splits, p.kps, p.long_k) == (0, 1, 0, 0) and p.bm == p.bn == 32
    # a workspace one byte short of the query's answer: the split count falls back as the launch's does
    # (shapes whose queried workspace holds exactly the planned k ranges, so that one byte less changes the plan;
    # (family, splits, kps) with the whole workspace and one byte short. 384 x 768 x 1056 leaves the LDS-DMA kernel
    # with it: three k ranges give under 256 64-square tiles, and the 32-square tile is refused for A^T B)
    for (ta, tb, M, N, K), want_full, want_short in (((1, 0, 384, 768, 1056), (2, 4, 288), (1, 3, 352)),
                                                     ((0, 0, 130, 67, 512), (0, 4, 128), (0, 3, 192)),
                                                     ((0, 1, 257, 384, 1537), (0, 9, 192), (0, 7, 224)),
                                                     ((0, 0, 64, 96, 512), (2, 4, 128), (2, 3, 192))):
        need = int(L.hvae_gemm_f32_workspace(M, N, K))
        slab = (M * N + M) * 4  # one k range's partial tiles and row sums
        assert need == want_full[1] * slab
        for ws_bytes, want in ((need, want_full), (need - 1, want_short)):
            p = G.single_plan(L, ta, tb, M, N, K, ws_bytes=ws_bytes)
            assert (p.family, p.splits, p.kps) == want, (ta, tb, M, N, K, ws_bytes)
        for ws_bytes in (2 * slab - 1, 0):  # room for fewer than two k ranges: one range over all of K
            p = G.single_plan(L, ta, tb, M, N, K, ws_bytes=ws_bytes)
            assert (p.splits, p.kps) == (1, K), (ta, tb, M, N, K, ws_bytes)
    # bad arguments are errors, not traps
    p = _lib.GemmPlan()
    assert L.hvae_gemm_f32_plan(0, 0, -1, 4, 4, None, 4, None, 4, 0, 0, C.byref(p)) == -1
    assert L.hvae_gemm_f32_plan(0, 0, 4, 4, 4, None, 4, None, 4, 0, 0, None) == -1
    assert L.hvae_gemm_f32_pair_plan(None, None, None, None) == -1
