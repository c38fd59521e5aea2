"""Every fp32 GEMM kernel instance the planner can choose, exactly.

The kernels are an fp32 fmaf chain on the exact-f32 MFMA, so with small integer operands every product and every
partial sum is an integer below 2^24 (|a|, |b| <= 8, K <= 4096: at most 64 K = 2^18) and the result must be bitwise
the integer answer whatever the k order, tile, LDS swizzle or split-K reduction order: one dropped, doubled or
misplaced k term in one element fails torch.equal. The case tables live in tests/gemm_plan_cases.py; each case
first asserts, through the host plan query on the very pointers it launches with, that it runs the instance the
table names (tests/test_gemm_plan_cpu.py keeps the table complete).

test_instance_randn keeps one pass with real numbers. Its bar is elementwise,
|c - ref| <= 8 sqrt(K + 1) 2^-24 (|alpha| (|A| |B|)_ij + |beta C0_ij|): sqrt(K + 1) 2^-24 is the random-walk estimate
of an fmaf chain's rounding error against the sum of magnitudes, 8 the margin over it. Largest observed
error / bar on an MI355X over the cases: 0.158, at 70 x 45 x 5 (A B, register-staged); K = 1 gives 0.15 (there the
bar is 11 half-ulps of the one product plus beta C0), 256 x 4096 x 32 on the LDS-DMA kernel 0.124, and long-K split-K
cases stay under 0.01. That is under the 0.25 at which the constant would have to widen; test_instance_randn prints
each case's ratio.
"""
import ctypes as C
import math

import pytest
import torch

import gemm_plan_cases as G
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

# the table's rows and the further keyed shapes on the same instances
ALL_SINGLE = G.SINGLE_CASES + G.EXTRA_SINGLE_CASES

ALPHAS, BETAS = (1.0, 0.5, -2.0), (0.0, 1.0, -0.5)
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops(hip_device):
    from hvae import ops
    return ops


def _ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _embed(t, dev, ld=None, offset=0, fill=float("nan"), extra_rows=0):
    """t [R, C] as a view with row stride ld, `offset` floats into a larger device buffer whose other elements are
    `fill`. Returns (view, buffer)."""
    Rr, Cc = t.shape
    ld = Cc if ld is None else ld
    buf = torch.full((offset + (Rr + extra_rows) * ld + 8,), fill, device=dev)
    view = buf[offset:offset + Rr * ld].as_strided((Rr, Cc), (ld, 1)) if Rr and Cc else buf[offset:offset].view(Rr, Cc)
    if Rr and Cc:
        view.copy_(t)
    return view, buf


class Operands:
    """A = op(A) [M, K] and B = op(B) [K, N] stored as the transposition flags say, each a view into a NaN-filled
    buffer: pad floats of leading-dimension padding, the base pointer `offset` floats into the buffer."""

    def __init__(self, dev, ta, tb, A, B, pad=0, offset=0):
        self.ta, self.tb = int(ta), int(tb)
        (self.M, self.K), self.N = A.shape, B.shape[1]
        As, Bs = (A.t() if ta else A).contiguous(), (B.t() if tb else B).contiguous()
        self.Av, self.Abuf = _embed(As, dev, As.shape[1] + pad, offset)
        self.Bv, self.Bbuf = _embed(Bs, dev, Bs.shape[1] + pad, offset)
        self.lda, self.ldb = As.shape[1] + pad, Bs.shape[1] + pad
        self.pa, self.pb = self.Abuf.data_ptr() + 4 * offset, self.Bbuf.data_ptr() + 4 * offset

    def plan(self, ws_bytes):
        from hvae._lib import lib
        return G.single_plan(lib(), self.ta, self.tb, self.M, self.N, self.K, a=self.pa, lda=self.lda, b=self.pb,
                             ldb=self.ldb, ws=ws_bytes > 0, ws_bytes=ws_bytes)


def _workspace(dev, nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _launch(o, alpha, beta, Cv, ldc, epi=None, ws=None, ws_bytes=0):
    from hvae._lib import check, lib
    st = torch.cuda.current_stream(Cv.device).cuda_stream
    check(lib().hvae_gemm_f32(o.ta, o.tb, o.M, o.N, o.K, float(alpha), o.pa, o.lda, o.pb, o.ldb, float(beta),
                              Cv.data_ptr(), ldc, C.byref(epi) if epi is not None else None,
                              ws.data_ptr() if ws is not None and ws_bytes else None, ws_bytes, st), "hvae_gemm_f32")


def _ws_for(dev, M, N, K, want):
    from hvae._lib import lib
    need = int(lib().hvae_gemm_f32_workspace(M, N, K)) if want else 0
    return _workspace(dev, need), need


def _ref64(A, B, C0, alpha, beta, dev):
    """alpha A B + beta C0 in float64 (on the device: exact for the integer operands whatever its order)."""
    return alpha * (A.to(dev).double() @ B.to(dev).double()) + beta * C0.to(dev).double()


def _case_id(c):
    return "-".join(str(v) for v in c[:-1]) + "-key" + "".join(str(v) for v in c[-1])


# ----------------------------------------------------------------------------------------------- one instance --
@pytest.mark.parametrize("case", ALL_SINGLE, ids=_case_id)
def test_instance_exact(ops, hip_device, case):
    """Integer operands: C and the fused row sums are bitwise the integer answer; split-K twice gives the same bits."""
    from hvae import _lib
    ta, tb, M, N, K, ws_on, aligned, key = case
    i = ALL_SINGLE.index(case)
    alpha, beta = ALPHAS[i % 3], BETAS[(i // 3) % 3]
    g = _gen(M, N, K, ta, tb)
    A, B, C0 = _ints(g, M, K), _ints(g, K, N), _ints(g, M, N)
    o = Operands(hip_device, ta, tb, A, B, offset=0 if aligned else 1)
    ws, nws = _ws_for(hip_device, M, N, K, ws_on)
    p = o.plan(nws)
    assert G.single_key(ta, tb, p) == key, "the case no longer runs the instance it is listed for"
    ref = _ref64(A, B, C0, alpha, beta, hip_device).float()
    rs_ref = (alpha * A.double().sum(1)).float().to(hip_device)
    outs = []
    for rep in range(2 if p.splits > 1 else 1):
        out = C0.to(hip_device).clone()
        _launch(o, alpha, beta, out, N, None, ws, nws)
        outs.append(out)
        assert torch.equal(out, ref), f"plan {G.plan_tuple(p)}: {(out != ref).sum().item()} elements differ"
        # the same launch with the fused row sums of op(A) (the bias gradient beside a weight gradient)
        out2, rs = C0.to(hip_device).clone(), torch.full((M,), float("nan"), device=hip_device)
        _launch(o, alpha, beta, out2, N, ops.epilogue(_lib.EPI_NONE, opa_rowsum=rs), ws, nws)
        assert torch.equal(out2, ref) and torch.equal(rs, rs_ref)
    assert all(torch.equal(outs[0], x) for x in outs[1:])


@pytest.mark.parametrize("case", ALL_SINGLE, ids=_case_id)
def test_instance_randn(ops, hip_device, case):
    """Real (denormal-free, non-integer) operands on every instance, elementwise against float64."""
    ta, tb, M, N, K, ws_on, aligned, key = case
    alpha, beta = 0.5, 0.25
    g = _gen(M, N, K, ta, tb, 1)
    A, B, C0 = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(M, N, generator=g)
    o = Operands(hip_device, ta, tb, A, B, offset=0 if aligned else 1)
    ws, nws = _ws_for(hip_device, M, N, K, ws_on)
    p = o.plan(nws)
    assert G.single_key(ta, tb, p) == key
    ref = _ref64(A, B, C0, alpha, beta, hip_device)
    mag = _ref64(A.abs(), B.abs(), C0.abs(), abs(alpha), abs(beta), hip_device)
    bar = 8.0 * math.sqrt(K + 1) * 2.0 ** -24 * mag
    outs = []
    for rep in range(2 if p.splits > 1 else 1):
        out = C0.to(hip_device).clone()
        _launch(o, alpha, beta, out, N, None, ws, nws)
        outs.append(out)
    err = (outs[0].double() - ref).abs()
    ratio = float((err / bar).max()) if M * N else 0.0
    print(f"randn ratio {ratio:.4f} case {case[:-1]} plan {G.plan_tuple(p)}")
    assert bool((err <= bar).all()), f"max error / bar = {ratio}"
    assert all(torch.equal(outs[0], x) for x in outs[1:])  # split-K: deterministic in real numbers too


# ----------------------------------------------------------------------------- operands as a caller may pass --
RAGGED, WHOLE = (130, 67, 300), (128, 96, 64)
# trans_a without trans_b: whole tiles on the fast kernel (K >= 1024) and on the LDS-DMA kernel (split-K)
WHOLE_TN = ((64, 96, 1024), (384, 768, 1056))
OPERAND_CASES = [(ta, tb, shape, var)
                 for ta, tb in G.TRANS
                 for shape in ((RAGGED, WHOLE) + (WHOLE_TN if (ta, tb) == (1, 0) else ()))
                 for var in ("pad4", "pad3_off1", "dense")]


@pytest.mark.parametrize("ta,tb,shape,var", OPERAND_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_operand_views(ops, hip_device, ta, tb, shape, var):
    """Padded leading dimensions, a base pointer that is not 16-byte aligned, and ldc = N + 5: every operand is a
    view into a larger buffer of NaN, C's padding columns and the rows after M hold a sentinel. The result is exact,
    NaN-free, and no sentinel is touched."""
    M, N, K = shape
    g = _gen(M, N, K, ta, tb, 2)
    A, B, C0 = _ints(g, M, K), _ints(g, K, N), _ints(g, M, N)
    pad, off = {"pad4": (4, 0), "pad3_off1": (3, 1), "dense": (0, 0)}[var]
    o = Operands(hip_device, ta, tb, A, B, pad=pad, offset=off)
    ws, nws = _ws_for(hip_device, M, N, K, True)
    p = o.plan(nws)
    dense = G.single_plan(_lib_(), ta, tb, M, N, K)
    if var == "pad4":  # the fast and LDS-DMA plans survive a padded leading dimension
        assert G.plan_tuple(p) == G.plan_tuple(dense)
        assert shape == RAGGED or p.family == (1 if shape == WHOLE_TN[0] else 0 if (ta, tb, shape) == (1, 0, WHOLE) else 2)
    elif var == "pad3_off1":  # not vectorisable: the register-staged kernel and load4's scalar branch
        assert (p.family, p.vec_a, p.vec_b) == (0, 0, 0)
    ldc = N + 5
    Cv, Cbuf = _embed(C0, hip_device, ldc, 0, fill=SENTINEL, extra_rows=2)
    alpha, beta = -2.0, -0.5
    _launch(o, alpha, beta, Cv, ldc, None, ws, nws)
    ref = _ref64(A, B, C0, alpha, beta, hip_device).float()
    assert torch.equal(Cv, ref)
    mask = torch.ones_like(Cbuf, dtype=torch.bool)
    mask[:M * ldc].view(M, ldc)[:, :N] = False
    assert bool((Cbuf[mask] == SENTINEL).all()), "a store outside C[:M, :N]"


def _lib_():
    from hvae._lib import lib
    return lib()


# -------------------------------------------------------------------------------------------------- epilogues --
# x W^T products (trans_b): (M, N, K) -> (family, bm, bn, split) as the plan query must answer
EPI_SHAPES = [((70, 45, 33), (0, 32, 32, 0)), ((64, 96, 32), (2, 32, 32, 0)), ((256, 4096, 32), (2, 64, 32, 0)),
              ((512, 4096, 32), (2, 64, 64, 0)), ((130, 67, 769), (0, 32, 32, 1)), ((64, 96, 512), (2, 32, 32, 1))]


def _maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


@pytest.mark.parametrize("shape,want", EPI_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_epilogues_on_each_family(ops, hip_device, shape, want):
    """BIAS and DROP_BWD exactly, BIAS_GELU_DROP's pre-activation exactly and its output against a float64 GELU,
    GELU_DROP_BWD against float64 (both at test_gemm_epilogues' 1e-5 max-rel)."""
    from hvae import _lib
    M, N, K = shape
    g = _gen(M, N, K, 3)
    A, W, bias = _ints(g, M, K), _ints(g, N, K), _ints(g, N)
    mult = 2.0 * (torch.rand(M, N, generator=g) >= 0.5).float()  # p = 0.5: multipliers in {0, 2}
    o = Operands(hip_device, 0, 1, A, W.t())
    ws, nws = _ws_for(hip_device, M, N, K, True)
    p = o.plan(nws)
    assert (p.family, p.bm, p.bn, int(p.splits > 1)) == want
    bd, md = bias.to(hip_device), mult.to(hip_device)
    acc = (A.double() @ W.double().t())

    def run(epi):
        out = torch.full((M, N), float("nan"), device=hip_device)
        _launch(o, 1.0, 0.0, out, N, epi, ws, nws)
        return out

    assert torch.equal(run(ops.epilogue(_lib.EPI_BIAS, bias=bd)).cpu(), (acc + bias.double()).float())
    out = run(ops.epilogue(_lib.EPI_DROP_BWD, p_drop=0.5, drop_mult=md, train=True))
    assert torch.equal(out.cpu(), (acc * mult.double()).float())
    pre = torch.full((M, N), float("nan"), device=hip_device)
    out = run(ops.epilogue(_lib.EPI_BIAS_GELU_DROP, bias=bd, pre_out=pre, p_drop=0.5, drop_mult=md, train=True))
    ref_pre = acc + bias.double()
    assert torch.equal(pre.cpu(), ref_pre.float())
    assert _maxrel(out, R.gelu(ref_pre) * mult.double()) < 1e-5
    # backward: c * mult * gelu'(pre_in), pre_in real numbers
    pre_in = torch.randn(M, N, generator=g)
    pd = pre_in.to(hip_device)  # (held: the epilogue keeps only its address)
    out = run(ops.epilogue(_lib.EPI_GELU_DROP_BWD, pre_in=pd, p_drop=0.5, drop_mult=md, train=True))
    x = pre_in.double().requires_grad_(True)
    (R.gelu(x) * mult.double() * acc).sum().backward()
    assert _maxrel(out, x.grad) < 1e-5


@pytest.mark.parametrize("shape,want", [((70, 45, 33), (0, 32, 32)), ((128, 64, 96), (2, 32, 32)),
                                        ((4096, 256, 64), (2, 64, 32))], ids=lambda v: str(v).replace(" ", ""))
def test_reparam_bwd_epilogue(ops, hip_device, shape, want):
    """REPARAM_BWD (C = [dmu | dlogvar], ldc = 2 N) on a ragged shape and on whole LDS-DMA tiles, against
    hvae_reparam_kl_bwd on the exact dz."""
    from hvae import _lib
    M, N, K = shape
    g = _gen(M, N, K, 4)
    Gm, W = _ints(g, M, K), _ints(g, K, N)
    heads = (0.5 * torch.randn(M, 2 * N, generator=g)).to(hip_device)
    eps = torch.randn(M, N, generator=g).to(hip_device)
    ks = 0.2 / M
    o = Operands(hip_device, 0, 0, Gm, W)
    p = o.plan(0)
    assert (p.family, p.bm, p.bn) == want
    dz = (Gm.double() @ W.double()).float().to(hip_device)
    dmu, dlv = ops.reparam_kl_bwd(dz, heads[:, :N], heads[:, N:], eps, ks, True)
    dheads = torch.full((M, 2 * N), float("nan"), device=hip_device)
    _launch(o, 1.0, 0.0, dheads, 2 * N, ops.epilogue(_lib.EPI_REPARAM_BWD, pre_in=heads, train=True, aux=eps,
                                                     aux_scale=ks))
    assert torch.isfinite(dheads).all()
    assert _maxrel(dheads[:, :N], dmu) < 1e-5 and _maxrel(dheads[:, N:], dlv) < 1e-5


@pytest.mark.parametrize("ta,tb,shape,want", [(1, 0, (70, 45, 33), (0, 0)), (1, 0, (64, 96, 1056), (1, 1)),
                                              (1, 0, (384, 768, 1056), (2, 1)), (1, 0, (256, 4096, 32), (2, 0)),
                                              (1, 0, (130, 67, 769), (0, 1)), (0, 0, (64, 96, 512), (2, 1))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_rowsum_beside_bias_epilogue(ops, hip_device, ta, tb, shape, want):
    """opa_rowsum together with a BIAS epilogue, with and without split-K, on each family: both exact."""
    from hvae import _lib
    M, N, K = shape
    g = _gen(M, N, K, 5)
    A, B, bias = _ints(g, M, K), _ints(g, K, N), _ints(g, N)
    o = Operands(hip_device, ta, tb, A, B)
    ws, nws = _ws_for(hip_device, M, N, K, True)
    p = o.plan(nws)
    assert (p.family, int(p.splits > 1)) == want
    out, rs = torch.full((M, N), float("nan"), device=hip_device), torch.full((M,), float("nan"), device=hip_device)
    bd = bias.to(hip_device)
    _launch(o, 0.5, 0.0, out, N, ops.epilogue(_lib.EPI_BIAS, bias=bd, opa_rowsum=rs), ws, nws)
    assert torch.equal(out.cpu(), (0.5 * (A.double() @ B.double()) + bias.double()).float())
    assert torch.equal(rs.cpu(), (0.5 * A.double().sum(1)).float())


# ------------------------------------------------------------------------------------------------------ pairs --
def _pair_problem(dev, B, M, N, Kx, ws_mode, aligned, seed, ints=True):
    """dY [B, M], X [B, N], W [M, Kx] as views (integers, or randn); the (w, x) descriptors over them with fresh
    outputs at each call."""
    from hvae import _lib
    from hvae._lib import GemmDesc, lib
    g = _gen(B, M, N, Kx, seed)
    draw = _ints if ints else (lambda g_, *s: torch.randn(*s, generator=g_))
    dY, X, W = draw(g, B, M), draw(g, B, N), draw(g, M, Kx)
    off = 0 if aligned else 1
    views = [_embed(t, dev, None, off) for t in (dY, X, W)]
    nw, nx = int(lib().hvae_gemm_f32_workspace(M, N, B)), int(lib().hvae_gemm_f32_workspace(B, Kx, M))
    if ws_mode == "none":
        wsw = wsx = (None, 0)
        keep = None
    elif ws_mode == "shared":
        keep = _workspace(dev, max(nw, nx))
        wsw = wsx = (keep.data_ptr(), max(nw, nx)) if max(nw, nx) else (None, 0)
    else:
        keep = (_workspace(dev, nw), _workspace(dev, nx))
        wsw = (keep[0].data_ptr(), nw) if nw else (None, 0)
        wsx = (keep[1].data_ptr(), nx) if nx else (None, 0)

    def descs():
        dW = torch.full((M, N), float("nan"), device=dev)
        dXb = torch.full((B * Kx + 8,), float("nan"), device=dev)  # (B = 0: still a pointer)
        dX = dXb[:B * Kx].view(B, Kx)
        rs = torch.full((M,), float("nan"), device=dev)
        epi = _lib.Epilogue(_lib.EPI_NONE, None, None, None, 0.0, None, 0, None, 0, 0, rs.data_ptr())
        pa = lambda i: views[i][1].data_ptr() + 4 * off  # noqa: E731
        w = GemmDesc(1, 0, M, N, B, 1.0, pa(0), M, pa(1), N, 0.0, dW.data_ptr(), N, C.pointer(epi), *wsw)
        x = GemmDesc(0, 0, B, Kx, M, 1.0, pa(0), M, pa(2), Kx, 0.0, dXb.data_ptr(), Kx, None, *wsx)
        return w, x, (dW, dX, rs, epi)

    ref = ((dY.double().t() @ X.double()).float(), (dY.double() @ W.double()).float(), dY.double().sum(0).float())
    return descs, ref, (views, keep)


def _pair_id(c):
    return "-".join(str(v) for v in c[:-1]) + "-key" + "".join(str(v) for v in (c[-1] or ("two-launches",)))


@pytest.mark.parametrize("case", G.PAIR_CASES + [G.PAIR_SHARED_SPLIT + ("shared", 1, None)], ids=_pair_id)
def test_pair_exact_and_bitwise_two_launches(ops, hip_device, case):
    """hvae_gemm_f32_pair for every launch kind and tile pairing: bitwise the two hvae_gemm_f32 launches, and exact.
    The last case has both halves split-K into one shared workspace: it must report two launches."""
    from hvae._lib import check, lib
    B, M, N, Kx, ws_mode, aligned, key = case
    descs, ref, keep = _pair_problem(hip_device, B, M, N, Kx, ws_mode, aligned, 6)
    st = torch.cuda.current_stream(hip_device).cuda_stream
    w, x, (dW2, dX2, rs2, e2) = descs()
    kind, pw, px = G.pair_plan(lib(), w, x)
    if key is None:
        assert kind == 0 and pw.splits > 1 and px.splits > 1
    else:
        assert G.pair_key(kind, pw, px) == key, "the case no longer runs the launch it is listed for"
    check(lib().hvae_gemm_f32_pair(C.byref(w), C.byref(x), st), "gemm_pair")
    w1, x1, (dW1, dX1, rs1, e1) = descs()
    for d in (w1, x1):
        check(lib().hvae_gemm_f32(d.trans_a, d.trans_b, d.M, d.N, d.K, d.alpha, d.A, d.lda, d.B, d.ldb, d.beta, d.C,
                                  d.ldc, d.epi, d.ws, d.ws_bytes, st), "hvae_gemm_f32")
    torch.cuda.synchronize()
    for got2, got1, want in ((dW2, dW1, ref[0]), (dX2, dX1, ref[1]), (rs2, rs1, ref[2])):
        assert torch.equal(got2, got1)
        assert torch.equal(got2.cpu(), want)


@pytest.mark.parametrize("case", [c for c in G.PAIR_CASES if c[-1][0] != 0], ids=_pair_id)
def test_pair_randn_bitwise_two_launches(ops, hip_device, case):
    """The fused launches on real numbers: bitwise what the two single launches write (same k order per element)."""
    from hvae._lib import check, lib
    B, M, N, Kx, ws_mode, aligned, key = case
    descs, _, keep = _pair_problem(hip_device, B, M, N, Kx, ws_mode, aligned, 7, ints=False)
    st = torch.cuda.current_stream(hip_device).cuda_stream
    res = []
    for fused in (True, False):
        w, x, out = descs()
        if fused:
            assert G.pair_key(*G.pair_plan(lib(), w, x)) == key
            check(lib().hvae_gemm_f32_pair(C.byref(w), C.byref(x), st), "gemm_pair")
        else:
            for d in (w, x):
                check(lib().hvae_gemm_f32(d.trans_a, d.trans_b, d.M, d.N, d.K, d.alpha, d.A, d.lda, d.B, d.ldb, d.beta,
                                          d.C, d.ldc, d.epi, d.ws, d.ws_bytes, st), "hvae_gemm_f32")
        torch.cuda.synchronize()
        res.append(out[:3])
    assert all(torch.isfinite(a).all() and torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------------ multi --
MULTI_SHAPES = [(70, 45, 300), (33, 1, 129), (0, 40, 64), (130, 67, 5), (64, 96, 160), (7, 130, 513), (96, 33, 33),
                (257, 1, 769)]


@pytest.mark.parametrize("n", [1, 3, 8])
def test_multi_exact_and_bitwise_single_launches(ops, hip_device, n):
    """hvae_gemm_f32_multi over 1, 3 and 8 weight gradients of different ragged sizes (one of them empty when there is
    more than one) with the fused row sums: each exact, and bitwise its own hvae_gemm_f32 launch without a workspace."""
    from hvae import _lib
    from hvae._lib import GemmDesc, check, lib
    shapes = MULTI_SHAPES[:n]
    st = torch.cuda.current_stream(hip_device).cuda_stream
    keep, descs, outs = [], [], []
    for i, (M, N, K) in enumerate(shapes):
        g = _gen(M, N, K, 8 + i)
        A, B = _ints(g, K, M), _ints(g, K, N)  # dW = A^T B
        Ad, Bd = A.to(hip_device), B.to(hip_device)
        for _ in range(2):  # [0] the multi launch's outputs, [1] the single launch's
            Cd = torch.full((M, N), float("nan"), device=hip_device)
            rs = torch.full((M,), float("nan"), device=hip_device)
            epi = _lib.Epilogue(_lib.EPI_NONE, None, None, None, 0.0, None, 0, None, 0, 0, rs.data_ptr())
            keep.append((Ad, Bd, Cd, rs, epi))
        ref = ((A.double().t() @ B.double()).float(), A.double().sum(0).float())
        outs.append((keep[-2], keep[-1], ref))
        descs.append([GemmDesc(1, 0, M, N, K, 1.0, Ad.data_ptr(), max(M, 1), Bd.data_ptr(), max(N, 1), 0.0,
                               k[2].data_ptr(), max(N, 1), C.pointer(k[4]), None, 0) for k in (keep[-2], keep[-1])])
    arr = (GemmDesc * n)(*[d[0] for d in descs])
    check(lib().hvae_gemm_f32_multi(arr, n, st), "gemm_multi")
    for d in descs:
        d = d[1]
        if d.M == 0:
            continue
        check(lib().hvae_gemm_f32(d.trans_a, d.trans_b, d.M, d.N, d.K, d.alpha, d.A, d.lda, d.B, d.ldb, d.beta, d.C,
                                  d.ldc, d.epi, None, 0, st), "hvae_gemm_f32")
    torch.cuda.synchronize()
    for (M, N, K), (km, ks, ref) in zip(shapes, outs):
        if M == 0:
            continue
        assert torch.equal(km[2], ks[2]) and torch.equal(km[3], ks[3]), (M, N, K)
        assert torch.equal(km[2].cpu(), ref[0]) and torch.equal(km[3].cpu(), ref[1]), (M, N, K)
