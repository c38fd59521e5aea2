"""Tensor-level wrappers of the libhvae C ABI.

Every function here takes/returns torch tensors that live on the HIP device,
checks shapes, allocates outputs, and launches on the current stream. They
are the building blocks of the module-API autograd path (hvae/autograd.py)
and of the parity tests. The fused trainer (hvae/executor.py) calls the C ABI
directly with preallocated buffers instead.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import (ROWSQ_PARTS, CsrBatch, Epilogue, RowGrad, Adam, check, lib, ptr, require_hip, stream_of)

_WS: dict[torch.device, torch.Tensor] = {}


def workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Per-device scratch buffer, grown on demand (never shrunk)."""
    nbytes = max(int(nbytes), 256)
    ws = _WS.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes + (nbytes >> 2), dtype=torch.uint8, device=device)
        _WS[device] = ws
    return ws


class Csr:
    """A device CSR batch view (keeps the tensors alive for the C struct)."""

    def __init__(self, row_ptr: torch.Tensor, col_idx: torch.Tensor, vals: torch.Tensor, n_items: int,
                 rows: torch.Tensor | None = None, nb: int | None = None,
                 rows_offset: torch.Tensor | None = None):
        require_hip(row_ptr, col_idx, vals, rows)
        assert row_ptr.dtype == torch.int64 and col_idx.dtype == torch.int32 and vals.dtype == torch.float32
        assert rows is None or rows.dtype == torch.int32
        self.row_ptr, self.col_idx, self.vals, self.rows = row_ptr, col_idx, vals, rows
        self.rows_offset = rows_offset
        self.n_items = int(n_items)
        self.nb = int(nb if nb is not None else (rows.numel() if rows is not None else row_ptr.numel() - 1))
        self.struct = CsrBatch(ptr(row_ptr), ptr(col_idx), ptr(vals), ptr(rows), ptr(rows_offset), self.nb,
                               self.n_items)

    def rows_from_elsewhere(self):
        """The rows will be written by something other than the library's row-gradient apply (an injected
        DPExchange merge_fn): the clip must then read the rows, not the apply's per-row sums of squares
        (hvae_rowgrad.rowsq, include/hvae.h: non-NULL only where hvae_w1_rowgrad_apply produced the rows)."""
        self.struct.rowsq = None

    @property
    def ref(self):
        return C.byref(self.struct)


def csr_from_scipy(mat, device) -> Csr:
    """Upload a scipy.sparse CSR matrix (float values, summed duplicates kept) to the device."""
    mat = mat.tocsr()
    mat.sum_duplicates()
    row_ptr = torch.as_tensor(mat.indptr.astype("int64"), device=device)
    col = torch.as_tensor(mat.indices.astype("int32"), device=device)
    vals = torch.as_tensor(mat.data.astype("float32"), device=device)
    return Csr(row_ptr, col, vals, mat.shape[1])


def dense_to_csr(x: torch.Tensor) -> Csr:
    """Dense [B, N] (any values, zeros skipped) -> device CSR of the nonzeros."""
    require_hip(x)
    x = x.contiguous().float()
    B, N = x.shape
    cap = max(B * N, 1)
    row_ptr = torch.empty(B + 1, dtype=torch.int64, device=x.device)
    col = torch.empty(cap, dtype=torch.int32, device=x.device)
    vals = torch.empty(cap, dtype=torch.float32, device=x.device)
    check(lib().hvae_dense_to_csr(ptr(x), B, N, ptr(row_ptr), ptr(col), ptr(vals), cap, None, 0,
                                  stream_of(x)), "hvae_dense_to_csr")
    return Csr(row_ptr, col, vals, N)


# ------------------------------------------------------------------ encoder --
def encoder_fwd(x: Csr, w1t, b1, ln_w, ln_b, p_drop: float, train: bool, seed: int, step=None,
                drop_mult=None, save=True):
    H = w1t.shape[1]
    dev = w1t.device
    require_hip(w1t, b1, ln_w, ln_b, drop_mult)
    h = torch.empty(x.nb, H, device=dev)
    xhat = torch.empty(x.nb, H, device=dev) if save else None
    rstd = torch.empty(x.nb, device=dev) if save else None
    check(lib().hvae_encoder_fwd(x.ref, ptr(w1t), ptr(b1), ptr(ln_w), ptr(ln_b), H, float(p_drop), ptr(drop_mult),
                                 seed, ptr(step), int(train), ptr(h), ptr(xhat), ptr(rstd), stream_of(w1t)),
          "hvae_encoder_fwd")
    return h, xhat, rstd


def ln_gelu_drop_fwd(a, ln_w, ln_b, p_drop, train, seed, layer, step=None, drop_mult=None, save=True):
    require_hip(a, ln_w, ln_b, drop_mult)
    a = a.contiguous()
    nb, H = a.shape
    h = torch.empty_like(a)
    xhat = torch.empty_like(a) if save else None
    rstd = torch.empty(nb, device=a.device) if save else None
    check(lib().hvae_ln_gelu_drop_fwd(ptr(a), ptr(ln_w), ptr(ln_b), nb, H, float(p_drop), ptr(drop_mult), seed,
                                      ptr(step), layer, int(train), ptr(h), ptr(xhat), ptr(rstd), stream_of(a)),
          "hvae_ln_gelu_drop_fwd")
    return h, xhat, rstd


def ln_gelu_drop_bwd(dh, xhat, rstd, ln_w, ln_b, p_drop, train, seed, layer, step=None, drop_mult=None,
                     want_dbias=False):
    """-> (da, d_ln_w, d_ln_b) or, with want_dbias, (da, d_ln_w, d_ln_b, sum_rows(da))."""
    require_hip(dh, xhat, rstd, ln_w, ln_b)
    dh = dh.contiguous()
    nb, H = dh.shape
    da = torch.empty_like(dh)
    dw = torch.empty(H, device=dh.device)
    db = torch.empty(H, device=dh.device)
    dbias = torch.empty(H, device=dh.device) if want_dbias else None
    need = lib().hvae_ln_gelu_drop_bwd_workspace(nb, H)
    ws = workspace(dh.device, need)
    check(lib().hvae_ln_gelu_drop_bwd(ptr(dh), ptr(xhat), ptr(rstd), ptr(ln_w), ptr(ln_b), nb, H, float(p_drop),
                                      ptr(drop_mult), seed, ptr(step), layer, int(train), ptr(da), ptr(dw), ptr(db),
                                      ptr(dbias), ptr(ws), ws.numel(), stream_of(dh)), "hvae_ln_gelu_drop_bwd")
    return (da, dw, db, dbias) if want_dbias else (da, dw, db)


class RowGradBuffers:
    """Device buffers of the row-sparse first-layer weight gradient."""

    def __init__(self, n_items: int, H: int, cap: int, device, width: int | None = None):
        """width: the widest row the buffers must hold (default H): the fused step with trainable item embeddings
        also gathers rows of the decoder input u (width d) through the same plan."""
        W = max(H, width or H)
        i32 = dict(dtype=torch.int32, device=device)
        self.cnt = torch.zeros(n_items, **i32)
        self.slot_of = torch.full((n_items,), -1, **i32)
        self.item_of = torch.zeros(cap, **i32)
        self.seg_off = torch.zeros(cap + 1, **i32)
        self.fill = torch.zeros(cap, **i32)
        self.contrib_row = torch.zeros(cap, **i32)
        self.contrib_val = torch.zeros(cap, dtype=torch.float32, device=device)
        self.rows = torch.zeros(cap * W, dtype=torch.float32, device=device)[:cap * H].view(cap, H)
        self.n_unique = torch.zeros(1, **i32)
        self.contrib_slot = torch.zeros(cap, **i32)
        self.part = torch.empty(int(lib().hvae_rowgrad_part_floats(cap, W)), dtype=torch.float32, device=device)
        self.rowsq = torch.zeros(cap * ROWSQ_PARTS, dtype=torch.float64, device=device)
        self.cap, self.n_items, self.H = cap, n_items, H
        self.struct = RowGrad(ptr(self.cnt), ptr(self.slot_of), ptr(self.item_of), ptr(self.seg_off), ptr(self.fill),
                              ptr(self.contrib_row), ptr(self.contrib_val), ptr(self.rows), ptr(self.n_unique), cap,
                              n_items, ptr(self.contrib_slot), ptr(self.part), self.part.numel(), ptr(self.rowsq))
        self.ws = torch.empty(max(int(lib().hvae_w1_rowgrad_workspace(n_items)), 256), dtype=torch.uint8,
                              device=device)

    def rows_from_elsewhere(self):
        """The rows will be written by something other than the library's row-gradient apply (an injected
        DPExchange merge_fn): the clip must then read the rows, not the apply's per-row sums of squares
        (hvae_rowgrad.rowsq, include/hvae.h: non-NULL only where hvae_w1_rowgrad_apply produced the rows)."""
        self.struct.rowsq = None

    @property
    def ref(self):
        return C.byref(self.struct)


def w1_rowgrad(x: Csr, da: torch.Tensor, rg: RowGradBuffers) -> None:
    require_hip(da)
    check(lib().hvae_w1_rowgrad(x.ref, ptr(da), da.shape[1], rg.ref, ptr(rg.ws), rg.ws.numel(), stream_of(da)),
          "hvae_w1_rowgrad")


def w1_rowgrad_plan(x: Csr, rg: RowGradBuffers) -> None:
    """The plan half of w1_rowgrad (needs the batch only), on the current stream."""
    check(lib().hvae_w1_rowgrad_plan(x.ref, rg.ref, ptr(rg.ws), rg.ws.numel(),
                                     torch.cuda.current_stream(rg.rows.device).cuda_stream), "hvae_w1_rowgrad_plan")


def w1_rowgrad_apply(da: torch.Tensor, rg: RowGradBuffers) -> None:
    """The apply half of w1_rowgrad: rows from da over a plan already made."""
    require_hip(da)
    check(lib().hvae_w1_rowgrad_apply(ptr(da), da.shape[1], rg.ref, stream_of(da)), "hvae_w1_rowgrad_apply")


def rowgrad_to_dense(rg: RowGradBuffers, out: torch.Tensor) -> None:
    """out: zero-filled [N, ld] item-major buffer."""
    check(lib().hvae_rowgrad_to_dense(rg.ref, rg.H, ptr(out), out.stride(0), stream_of(out)),
          "hvae_rowgrad_to_dense")


# --------------------------------------------------------------------- GEMM --
def _as_operand(t: torch.Tensor):
    """(base tensor, transposed?, ld) such that t == base or t == base.T with base row-major."""
    if t.dim() != 2:
        raise ValueError("GEMM operands must be 2-D")
    if t.stride(1) == 1 and t.stride(0) >= max(t.shape[1], 1):
        return t, False, t.stride(0)
    if t.stride(0) == 1 and t.stride(1) >= max(t.shape[0], 1):
        return t, True, t.stride(1)
    return t.contiguous(), False, t.shape[1]


def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None, alpha=1.0, beta=0.0, epi=None):
    """out[M,N] = alpha * a[M,K] @ b[K,N] + beta * out (fp32 MFMA), then the epilogue.

    a and b may be transposed views (e.g. a Linear weight .t()); no copies are made.
    """
    require_hip(a, b)
    M, K = a.shape
    K2, N = b.shape
    assert K == K2, f"gemm shape mismatch {a.shape} @ {b.shape}"
    A, ta, lda = _as_operand(a)
    B, tb, ldb = _as_operand(b)
    if out is None:
        out = torch.empty(M, N, device=a.device)
        beta = 0.0
    assert out.stride(1) == 1
    need = lib().hvae_gemm_f32_workspace(M, N, K)
    ws = workspace(a.device, need) if need else None
    check(lib().hvae_gemm_f32(int(ta), int(tb), M, N, K, float(alpha), ptr(A), lda, ptr(B), ldb, float(beta),
                              ptr(out), out.stride(0), C.byref(epi) if epi is not None else None, ptr(ws),
                              ws.numel() if ws is not None else 0, stream_of(a)), "hvae_gemm_f32")
    return out


def epilogue(kind, bias=None, pre_out=None, pre_in=None, p_drop=0.0, drop_mult=None, seed=0, step=None,
             tag=0, train=False, opa_rowsum=None, aux=None, aux_scale=0.0, aux_scale_dev=None) -> Epilogue:
    return Epilogue(kind, ptr(bias), ptr(pre_out), ptr(pre_in), float(p_drop), ptr(drop_mult), int(seed), ptr(step),
                    int(tag), int(train), ptr(opa_rowsum), ptr(aux), float(aux_scale), ptr(aux_scale_dev))


def colsum(x: torch.Tensor, out: torch.Tensor | None = None, beta=0.0):
    require_hip(x)
    assert x.stride(1) == 1
    M, N = x.shape
    if out is None:
        out = torch.empty(N, device=x.device)
        beta = 0.0
    need = lib().hvae_colsum_workspace(M, N)
    ws = workspace(x.device, need)
    check(lib().hvae_colsum(ptr(x), M, N, x.stride(0), float(beta), ptr(out), ptr(ws), ws.numel(), stream_of(x)),
          "hvae_colsum")
    return out


# ------------------------------------------------------------------- latent --
def reparam_kl_fwd(mu, logvar, train: bool, seed: int, step=None, eps_in=None):
    require_hip(mu, logvar, eps_in)
    assert mu.stride(1) == 1 and logvar.stride(1) == 1 and mu.stride(0) == logvar.stride(0)
    nb, L = mu.shape
    z = torch.empty(nb, L, device=mu.device)
    eps = torch.empty(nb, L, device=mu.device) if train else None
    kl_rows = torch.empty(nb, device=mu.device)
    check(lib().hvae_reparam_kl_fwd(ptr(mu), ptr(logvar), mu.stride(0), nb, L, int(train), ptr(eps_in), seed,
                                    ptr(step), ptr(z), ptr(eps), ptr(kl_rows), stream_of(mu)), "hvae_reparam_kl_fwd")
    return z, eps, kl_rows


def reparam_kl_bwd(dz, mu, logvar, eps, kl_scale: float, train: bool, dmu=None, dlv=None, kl_scale_dev=None):
    nb, L = mu.shape
    if dmu is None:
        dmu = torch.empty(nb, L, device=mu.device)
        dlv = torch.empty(nb, L, device=mu.device)
    check(lib().hvae_reparam_kl_bwd(ptr(dz), ptr(mu), ptr(logvar), mu.stride(0), ptr(eps), nb, L, float(kl_scale),
                                    ptr(kl_scale_dev), int(train), ptr(dmu), ptr(dlv), dmu.stride(0), stream_of(mu)),
          "hvae_reparam_kl_bwd")
    return dmu, dlv


# ------------------------------------------------------------------ decoder --
class DecoderImage:
    """The frozen embeddings as the bf16 or fp8 decoder reads them (hvae_decoder_image): bf16 E [N, D]
    followed by its tile-transposed copy (bf16) or by the e4m3 fragment-order tiles and E's scale exponent
    (fp8). `bf16` is a view of the first part."""

    def __init__(self, E32: torch.Tensor, dtype: int = _lib.HVAE_BF16):
        require_hip(E32)
        if dtype not in (_lib.HVAE_BF16, _lib.HVAE_FP8):
            raise ValueError(f"decoder image dtype must be HVAE_BF16 or HVAE_FP8, got {dtype}")
        E32 = E32.contiguous()
        self.N, self.D = E32.shape
        self.dtype = dtype
        nbytes = int(lib().hvae_decoder_image_bytes(self.dtype, self.N, self.D))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=E32.device)
        check(lib().hvae_decoder_image(self.dtype, ptr(E32), self.N, self.D, ptr(self.buf), stream_of(E32)),
              "hvae_decoder_image")
        self.bf16 = self.buf[: self.N * self.D * 2].view(torch.bfloat16).view(self.N, self.D)
        self.device = E32.device

    def refresh(self, E32: torch.Tensor) -> None:
        """Rewrite the image from new values of E in place (same shape; captured graphs keep their pointers)."""
        require_hip(E32)
        if tuple(E32.shape) != (self.N, self.D):
            raise ValueError(f"refresh: E shape {tuple(E32.shape)} != image shape {(self.N, self.D)}")
        E32 = E32.contiguous()
        check(lib().hvae_decoder_image(self.dtype, ptr(E32), self.N, self.D, ptr(self.buf), stream_of(E32)),
              "hvae_decoder_image")

    def data_ptr(self) -> int:
        return self.buf.data_ptr()


def decoder_image(E32: torch.Tensor, dtype: int = _lib.HVAE_BF16) -> DecoderImage:
    return DecoderImage(E32, dtype)


def _dec_operand(E):
    """(dtype code, N, pointer holder) of a decoder E argument: a DecoderImage (bf16) or an fp32 [N, D]."""
    if isinstance(E, DecoderImage):
        return E.dtype, E.N, E
    if E.dtype == torch.bfloat16:
        raise TypeError("the bf16 decoder takes a DecoderImage (ops.decoder_image), not a bf16 tensor")
    return _lib.HVAE_F32, E.shape[0], E


def row_norm_max(E, out: torch.Tensor | None = None) -> torch.Tensor:
    """max_i ||E_i|| of an fp32 / bf16 [N, D] matrix or of a DecoderImage's bf16 values (device scalar; written
    into `out` when given)."""
    if isinstance(E, DecoderImage):
        E = E.bf16
    require_hip(E)
    out = torch.empty(1, device=E.device) if out is None else out
    dtype = _lib.HVAE_BF16 if E.dtype == torch.bfloat16 else _lib.HVAE_F32
    check(lib().hvae_row_norm_max(dtype, ptr(E), E.shape[0], E.shape[1], ptr(out), stream_of(E)),
          "hvae_row_norm_max")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    require_hip(x)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().hvae_cast_bf16(ptr(x), ptr(y), x.numel(), stream_of(x)), "hvae_cast_bf16")
    return y


def decoder_supported(dtype: int, D: int) -> bool:
    return bool(lib().hvae_decoder_supported(dtype, D))


def decoder_fwd(U: torch.Tensor, E, enorm: torch.Tensor | None, with_o: bool = True):
    """(lse [nb], O [nb, D] or None) of the streaming decoder; E a DecoderImage (bf16) or fp32 [N, D]."""
    dtype, N, Eh = _dec_operand(E)
    require_hip(U)
    assert U.stride(1) == 1
    nb, D = U.shape
    lse = torch.empty(nb, device=U.device)
    O = torch.empty(nb, D, device=U.device) if with_o else None
    need = lib().hvae_decoder_workspace(dtype, nb, N, D)
    ws = workspace(U.device, need)
    check(lib().hvae_decoder_fwd(dtype, ptr(U), U.stride(0), ptr(Eh), ptr(enorm), nb, N, D, ptr(lse), ptr(O),
                                 ptr(ws), ws.numel(), stream_of(U)), "hvae_decoder_fwd")
    return lse, O


def decoder_bwd(x: Csr, U, E32, lse, O, grad_scale: float, want_du: bool = True):
    nb, D = U.shape
    recon_rows = torch.empty(nb, device=U.device)
    dU = torch.empty(nb, D, device=U.device) if want_du else None
    check(lib().hvae_decoder_bwd(x.ref, ptr(U), U.stride(0), ptr(E32), D, ptr(lse), ptr(O), float(grad_scale),
                                 ptr(recon_rows), ptr(dU), stream_of(U)), "hvae_decoder_bwd")
    return recon_rows, dU


def decoder_train(x: Csr, U, E, enorm, E32, grad_scale: float, want_du: bool = True, want_o: bool = False,
                  kl_rows=None, beta: float = 0.0, loss3=None, accum3=None):
    """Fused sweep + finalize: (lse, O or None, recon_rows, dU or None).

    With kl_rows and loss3 given, the finalize also writes the batch loss means
    (total, recon, kl) into loss3 (and adds them to accum3), as hvae_loss_finalize.
    """
    dtype, N, Eh = _dec_operand(E)
    require_hip(U, E32)
    assert U.stride(1) == 1
    nb, D = U.shape
    lse = torch.empty(nb, device=U.device)
    O = torch.empty(nb, D, device=U.device) if want_o else None
    recon_rows = torch.empty(nb, device=U.device)
    dU = torch.empty(nb, D, device=U.device) if want_du else None
    ws = workspace(U.device, lib().hvae_decoder_workspace(dtype, nb, N, D))
    check(lib().hvae_decoder_train(dtype, ptr(U), U.stride(0), ptr(Eh), ptr(enorm), ptr(E32), x.ref, D,
                                   float(grad_scale), ptr(lse), ptr(O), ptr(recon_rows), ptr(dU), ptr(kl_rows),
                                   float(beta), None, ptr(loss3), ptr(accum3), ptr(ws), ws.numel(), stream_of(U)),
          "hvae_decoder_train")
    return lse, O, recon_rows, dU


def nll_rows_fwd(S, X):
    require_hip(S, X)
    nb, N = S.shape
    lse = torch.empty(nb, device=S.device)
    recon = torch.empty(nb, device=S.device)
    check(lib().hvae_nll_rows_fwd(ptr(S), S.stride(0), ptr(X), X.stride(0), nb, N, ptr(lse), ptr(recon),
                                  stream_of(S)), "hvae_nll_rows_fwd")
    return lse, recon


def nll_rows_bwd(S, X, lse, scale: float):
    nb, N = S.shape
    dS = torch.empty(nb, N, device=S.device)
    check(lib().hvae_nll_rows_bwd(ptr(S), S.stride(0), ptr(X), X.stride(0), ptr(lse), nb, N, float(scale), ptr(dS),
                                  dS.stride(0), stream_of(S)), "hvae_nll_rows_bwd")
    return dS


def loss_finalize(recon_rows, kl_rows, beta: float, out3=None, accum3=None):
    nb = recon_rows.numel()
    if out3 is None:
        out3 = torch.empty(3, device=recon_rows.device)
    check(lib().hvae_loss_finalize(ptr(recon_rows), ptr(kl_rows), nb, float(beta), ptr(out3), ptr(accum3),
                                   stream_of(recon_rows)), "hvae_loss_finalize")
    return out3


# ---------------------------------------------------------------- optimiser --
def clip_grad_norm(g_dense: torch.Tensor | None, rg: RowGradBuffers | None, max_norm: float,
                   norm_out=None, coef_out=None):
    dev = (g_dense if g_dense is not None else rg.rows).device
    if norm_out is None:
        norm_out = torch.empty(1, device=dev)
        coef_out = torch.empty(1, device=dev)
    n = g_dense.numel() if g_dense is not None else 0
    need = lib().hvae_clip_grad_norm_workspace(n, rg.cap if rg else 0, rg.H if rg else 0)
    ws = workspace(dev, need)
    check(lib().hvae_clip_grad_norm(ptr(g_dense), n, rg.ref if rg else None, rg.H if rg else 0, float(max_norm),
                                    ptr(norm_out), ptr(coef_out), ptr(ws), ws.numel(), torch.cuda.current_stream(
                                        dev).cuda_stream), "hvae_clip_grad_norm")
    return norm_out, coef_out


def adam_config(lr, betas, eps, weight_decay, step_dev, coef_dev=None) -> Adam:
    return Adam(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), ptr(step_dev),
                ptr(coef_dev))


def adam_dense(cfg: Adam, p, m, v, g):
    check(lib().hvae_adam_dense(C.byref(cfg), ptr(p), ptr(m), ptr(v), ptr(g), p.numel(), stream_of(p)),
          "hvae_adam_dense")


def adam_rows(cfg: Adam, p, m, v, rg: RowGradBuffers):
    N, H = p.shape
    check(lib().hvae_adam_rows(C.byref(cfg), ptr(p), ptr(m), ptr(v), rg.ref, N, H, stream_of(p)), "hvae_adam_rows")


def counter_add(c: torch.Tensor, delta: int = 1):
    check(lib().hvae_counter_add(ptr(c), int(delta), stream_of(c)), "hvae_counter_add")


# --------------------------------------------------------------------- eval --
def score_candidates(U, user_row, E32, cand):
    require_hip(U, user_row, E32, cand)
    R, Cn = cand.shape
    scores = torch.empty(R, Cn, device=U.device)
    check(lib().hvae_score_candidates(ptr(U), U.stride(0), ptr(user_row), ptr(E32), E32.shape[1], ptr(cand), R, Cn,
                                      ptr(scores), stream_of(U)), "hvae_score_candidates")
    return scores


def rank_first(scores):
    R, Cn = scores.shape
    rank = torch.empty(R, dtype=torch.int32, device=scores.device)
    check(lib().hvae_rank_first(ptr(scores), R, Cn, ptr(rank), stream_of(scores)), "hvae_rank_first")
    return rank


def topk(scores: torch.Tensor, k: int, exclude: Csr | None = None):
    """Exact top-k per row (score desc, ties -> larger index first); masks `exclude` in place."""
    require_hip(scores)
    R, N = scores.shape
    idx = torch.empty(R, k, dtype=torch.int32, device=scores.device)
    val = torch.empty(R, k, device=scores.device)
    check(lib().hvae_topk(ptr(scores), R, N, scores.stride(0), exclude.ref if exclude is not None else None, k,
                          ptr(idx), ptr(val), stream_of(scores)), "hvae_topk")
    return idx, val


def topk_fused_supported(d: int, k: int) -> bool:
    """Whether hvae_topk_fused serves embedding width d and k results per row: what its plan (hvae_topk_fused_plan, a
    host query) answers, asked for k items so that nothing but the pair (d, k) can be refused as unsupported."""
    p = _lib.TopkPlan()
    return lib().hvae_topk_fused_plan(0, max(k, 1), d, k, C.byref(p)) != _lib.HVAE_ERR_UNSUPPORTED


def topk_fused(U: torch.Tensor, E_img: "DecoderImage", E32: torch.Tensor, e32_maxnorm: torch.Tensor, k: int,
               exclude: Csr | None = None, with_flags: bool = False):
    """Exact top-k of U E32^T per row (score desc, ties -> larger index first; `exclude`'s items of each row
    left out) without the [R, N] score matrix (hvae_topk_fused). Rows the fused path flags are ranked by the
    exact path (hvae_gemm_f32 scores + hvae_topk) for those rows only. Returns idx int32 [R, k], val [R, k]
    (and the flags when with_flags)."""
    require_hip(U, E32, e32_maxnorm)
    assert U.stride(1) == 1 and E32.is_contiguous()
    assert exclude is None or exclude.rows_offset is None
    R, D = U.shape
    N = E32.shape[0]
    idx = torch.empty(R, k, dtype=torch.int32, device=U.device)
    val = torch.empty(R, k, device=U.device)
    flag = torch.empty(R, dtype=torch.int32, device=U.device)
    ws = workspace(U.device, lib().hvae_topk_fused_workspace(R, N, D, k))
    check(lib().hvae_topk_fused(ptr(U), U.stride(0), ptr(E_img.bf16), ptr(E32), ptr(e32_maxnorm), N, D,
                                exclude.ref if exclude is not None else None, R, k, ptr(idx), ptr(val), ptr(flag),
                                ptr(ws), ws.numel(), stream_of(U)), "hvae_topk_fused")
    bad = torch.nonzero(flag).flatten()
    if bad.numel():
        rows = bad.to(torch.int32)
        S = gemm(U.index_select(0, bad), E32.t())
        ex = None
        if exclude is not None:
            sel = exclude.rows.index_select(0, bad) if exclude.rows is not None else rows
            ex = Csr(exclude.row_ptr, exclude.col_idx, exclude.vals, exclude.n_items, rows=sel.contiguous())
        i2, v2 = topk(S, k, exclude=ex)
        idx.index_copy_(0, bad, i2)
        val.index_copy_(0, bad, v2)
    return (idx, val, flag) if with_flags else (idx, val)


def negatives_legacy(indptr, indices, n_items: int, users, tests, n_neg: int, arrays: bool = False):
    """The 99-negative protocol's negatives for test rows (users[r], tests[r]) over a training CSR
    (indptr / indices), drawn by libhvae from numpy's global legacy RandomState exactly as the reference's
    per-row np.random.choice(available, n_neg, replace=False) would (src/ml/evaluate.py:159-170), which
    leaves the global state where those calls would have (hvae_negatives_legacy). Returns a list of int64
    arrays, one per row (shorter where fewer than n_neg items are available); with arrays=True the int32
    [rows, n_neg] block and the per-row counts instead (entries past a row's count are undefined)."""
    import numpy as np
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    users = np.ascontiguousarray(users, dtype=np.int32)
    tests = np.ascontiguousarray(tests, dtype=np.int32)
    R = len(users)
    st = np.random.get_state(legacy=True)
    if st[0] != "MT19937":
        raise RuntimeError(f"negatives_legacy: numpy global bit generator {st[0]}, not MT19937")
    key = np.array(st[1], dtype=np.uint32, copy=True)
    pos = np.array([st[2]], dtype=np.int32)
    out = np.empty((R, n_neg), dtype=np.int32)
    counts = np.empty(R, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(lib().hvae_negatives_legacy(p(key), p(pos), p(indptr), len(indptr) - 1, p(indices), int(n_items), p(users),
                                      p(tests), R, int(n_neg), p(out), p(counts)), "hvae_negatives_legacy")
    np.random.set_state((st[0], key, int(pos[0]), st[3], st[4]))
    if arrays:
        return out, counts
    return [out[r, :counts[r]].astype(np.int64) for r in range(R)]


def negatives_legacy_rows(indptr, indices, n_items: int, users, n_draw, tests=None):
    """Row r draws np.random.choice(available, n_draw[r], replace=False) from numpy's global legacy RandomState,
    available = the items outside row users[r] of the CSR (and tests[r], when tests is given): the per-user draws of
    DatasetBuilder.create_negative_samples (src/preprocessing/dataset.py:111-123), by the sampler of negatives_legacy
    (hvae_negatives_legacy_rows). Returns (flat int32 draws, int64 offsets [rows + 1]). A row with fewer available
    items than draws (numpy's replace=True path) raises RuntimeError and leaves numpy's state untouched."""
    import numpy as np
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    users = np.ascontiguousarray(users, dtype=np.int32)
    n_draw = np.ascontiguousarray(n_draw, dtype=np.int32)
    if tests is not None:
        tests = np.ascontiguousarray(tests, dtype=np.int32)
    R = len(users)
    if len(n_draw) != R or (tests is not None and len(tests) != R):
        raise ValueError("negatives_legacy_rows: users, n_draw and tests must have one entry per row")
    if R and int(n_draw.min()) < 0:
        raise ValueError("negatives_legacy_rows: negative draw count")
    out_ptr = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(n_draw, dtype=np.int64, out=out_ptr[1:])
    st = np.random.get_state(legacy=True)
    if st[0] != "MT19937":
        raise RuntimeError(f"negatives_legacy_rows: numpy global bit generator {st[0]}, not MT19937")
    key = np.array(st[1], dtype=np.uint32, copy=True)
    pos = np.array([st[2]], dtype=np.int32)
    out = np.empty(max(int(out_ptr[-1]), 1), dtype=np.int32)
    counts = np.empty(max(R, 1), dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(lib().hvae_negatives_legacy_rows(p(key), p(pos), p(indptr), len(indptr) - 1, p(indices), int(n_items),
                                           p(users), p(tests), p(n_draw), p(out_ptr), R, p(out), p(counts)),
          "hvae_negatives_legacy_rows")
    np.random.set_state((st[0], key, int(pos[0]), st[3], st[4]))
    return out[:int(out_ptr[-1])], out_ptr


# ---------------------------------------------------------------- baselines --
class Csc:
    """A device item-major (CSC) image of an interaction matrix: col_ptr int64 [N + 1], row_idx int32 (user ids
    ascending per column), vals fp32 (duplicates summed)."""

    def __init__(self, col_ptr: torch.Tensor, row_idx: torch.Tensor, vals: torch.Tensor, n_users: int, n_items: int):
        require_hip(col_ptr, row_idx, vals)
        assert col_ptr.dtype == torch.int64 and row_idx.dtype == torch.int32 and vals.dtype == torch.float32
        assert col_ptr.numel() == n_items + 1 and row_idx.numel() == vals.numel()
        self.col_ptr, self.row_idx, self.vals = col_ptr, row_idx, vals
        self.n_users, self.n_items = int(n_users), int(n_items)


def csc_from_scipy(mat, device) -> Csc:
    """Upload a scipy.sparse matrix as canonical CSC (duplicates summed, user ids sorted within a column)."""
    mat = mat.tocsc()
    mat.sum_duplicates()
    mat.sort_indices()
    n_users, n_items = mat.shape
    if mat.nnz and (int(mat.indices.min()) < 0 or int(mat.indices.max()) >= n_users):
        raise ValueError("csc_from_scipy: a row index lies outside the matrix")
    col_ptr = torch.as_tensor(mat.indptr.astype("int64"), device=device)
    row = torch.as_tensor(mat.indices.astype("int32"), device=device)
    vals = torch.as_tensor(mat.data.astype("float32"), device=device)
    return Csc(col_ptr, row, vals, n_users, n_items)


def csc_col_stats(m: Csc):
    """(col_sum fp32 [N], inv_norm fp64 [N]) of a CSC image: column sums and 1 / column norms, 0 where the
    column is empty (hvae_csc_col_stats)."""
    dev = m.col_ptr.device
    col_sum = torch.empty(m.n_items, dtype=torch.float32, device=dev)
    inv_norm = torch.empty(m.n_items, dtype=torch.float64, device=dev)
    check(lib().hvae_csc_col_stats(ptr(m.col_ptr), ptr(m.row_idx), ptr(m.vals), m.n_items, ptr(col_sum),
                                   ptr(inv_norm), stream_of(m.col_ptr)), "hvae_csc_col_stats")
    return col_sum, inv_norm


def knn_workspace_bytes(nb: int, n_users: int) -> int:
    return int(lib().hvae_knn_workspace(int(nb), int(n_users)))


def knn_user_weights(x: Csr, m: Csc, inv_norm: torch.Tensor, T: torch.Tensor | None = None) -> torch.Tensor:
    """Stage 1 of Item-KNN for the batch x (x.rows = its users): T [n_users, nb] fp64, cleared and filled
    (hvae_knn_user_weights). T: a uint8 / fp64 buffer of at least knn_workspace_bytes(nb, n_users) to reuse."""
    require_hip(inv_norm, T)
    assert inv_norm.dtype == torch.float64 and inv_norm.numel() == m.n_items and x.n_items == m.n_items
    need = knn_workspace_bytes(x.nb, m.n_users)
    if T is None:
        T = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=inv_norm.device)
    t_bytes = T.numel() * T.element_size()
    check(lib().hvae_knn_user_weights(x.ref, ptr(m.col_ptr), ptr(m.row_idx), ptr(m.vals), ptr(inv_norm), m.n_users,
                                      ptr(T), t_bytes, stream_of(inv_norm)), "hvae_knn_user_weights")
    return T


def knn_score_candidates(x: Csr, m: Csc, inv_norm: torch.Tensor, T: torch.Tensor, cand: torch.Tensor,
                         zero_diag: bool) -> torch.Tensor:
    """fp32 [nb, C] Item-KNN scores of cand [nb, C] int32 from the T of the same batch
    (hvae_knn_score_candidates)."""
    require_hip(inv_norm, T, cand)
    assert cand.dtype == torch.int32 and cand.is_contiguous() and cand.shape[0] == x.nb
    out = torch.empty(cand.shape, dtype=torch.float32, device=cand.device)
    check(lib().hvae_knn_score_candidates(x.ref, ptr(m.col_ptr), ptr(m.row_idx), ptr(m.vals), ptr(inv_norm),
                                          m.n_users, ptr(T), T.numel() * T.element_size(), ptr(cand),
                                          cand.shape[1], int(bool(zero_diag)), ptr(out), stream_of(cand)),
          "hvae_knn_score_candidates")
    return out


def knn_scores(x: Csr, m: Csc, inv_norm: torch.Tensor, T: torch.Tensor, zero_diag: bool,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [nb, N] Item-KNN scores of every item from the T of the same batch (hvae_knn_scores)."""
    require_hip(inv_norm, T, out)
    if out is None:
        out = torch.empty(x.nb, m.n_items, dtype=torch.float32, device=inv_norm.device)
    assert out.dtype == torch.float32 and out.shape == (x.nb, m.n_items) and out.stride(1) == 1
    check(lib().hvae_knn_scores(x.ref, ptr(m.col_ptr), ptr(m.row_idx), ptr(m.vals), ptr(inv_norm), m.n_users,
                                ptr(T), T.numel() * T.element_size(), int(bool(zero_diag)), ptr(out),
                                out.stride(0), stream_of(inv_norm)), "hvae_knn_scores")
    return out


# ----------------------------------------------------------------- LightGCN --
LGCN_DIMS = (64, 128)  # hvae_lgcn_propagate / hvae_lgcn_bpr (include/hvae.h)


class LgcnGraph:
    """The bipartite user-item graph of an interaction matrix as hvae_lgcn_* read it: the device CSR and CSC of the
    structure (duplicates merged, explicit zeros dropped) and the degree scales deg^-1/2 (fp64, lgcn_norm)."""

    def __init__(self, csr: Csr, csc: Csc):
        if csr.nb != csc.n_users or csr.n_items != csc.n_items:
            raise ValueError("LgcnGraph: the CSR and the CSC are of different matrices")
        if csr.col_idx.numel() != csc.row_idx.numel():
            raise ValueError("LgcnGraph: the CSR and the CSC hold different numbers of entries")
        self.csr, self.csc = csr, csc
        self.n_users, self.n_items = csc.n_users, csc.n_items
        self.n_nodes = self.n_users + self.n_items
        self.nnz = int(csr.col_idx.numel())
        self.device = csr.row_ptr.device
        self.scale = torch.empty(self.n_nodes, dtype=torch.float64, device=self.device)
        self.struct = _lib.LgcnGraph(ptr(csr.row_ptr), ptr(csr.col_idx), ptr(csc.col_ptr), ptr(csc.row_idx),
                                     ptr(self.scale), self.n_users, self.n_items)
        lgcn_norm(self)

    @property
    def ref(self):
        return C.byref(self.struct)


def lgcn_graph_from_scipy(mat, device) -> LgcnGraph:
    """Upload the structure of a scipy.sparse interaction matrix (mat.nonzero(): duplicates are one edge, explicit
    zeros none) as an LgcnGraph."""
    m = mat.tocsr().copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return LgcnGraph(csr_from_scipy(m, device), csc_from_scipy(m, device))


def lgcn_norm(graph: LgcnGraph) -> torch.Tensor:
    """graph.scale[r] = deg(r)^-1/2 in double, 0 for an isolated node (hvae_lgcn_norm); returns it."""
    check(lib().hvae_lgcn_norm(ptr(graph.csr.row_ptr), graph.n_users, ptr(graph.csc.col_ptr), graph.n_items,
                               ptr(graph.scale), stream_of(graph.scale)), "hvae_lgcn_norm")
    return graph.scale


def _lgcn_table(graph: LgcnGraph, name: str, t: torch.Tensor | None):
    if t is None:
        return
    require_hip(t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != graph.n_nodes or not t.is_contiguous():
        raise ValueError(f"lgcn: {name} must be a contiguous fp32 [{graph.n_nodes}, d] table, got "
                         f"{tuple(t.shape)} {t.dtype}")
    if t.shape[1] not in LGCN_DIMS:
        raise ValueError(f"lgcn: embedding_dim {t.shape[1]} is not served; served: {LGCN_DIMS[0]} and {LGCN_DIMS[1]}")


def lgcn_propagate(graph: LgcnGraph, x: torch.Tensor, add: torch.Tensor | None = None,
                   out: torch.Tensor | None = None, alpha: float = 1.0) -> torch.Tensor:
    """out[r] = alpha * (add[r] + sum_{j in N(r)} w_rj x[j]) over every node (hvae_lgcn_propagate); out may not
    alias x."""
    _lgcn_table(graph, "x", x)
    _lgcn_table(graph, "add", add)
    if out is None:
        out = torch.empty_like(x)
    _lgcn_table(graph, "out", out)
    if out.data_ptr() == x.data_ptr():
        raise ValueError("lgcn_propagate: out may not alias x")
    if (add is not None and add.shape != x.shape) or out.shape != x.shape:
        raise ValueError("lgcn_propagate: x, add and out must have one shape")
    check(lib().hvae_lgcn_propagate(graph.ref, x.shape[1], ptr(x), ptr(add), ptr(out), float(alpha), stream_of(x)),
          "hvae_lgcn_propagate")
    return out


def lgcn_chain(graph: LgcnGraph, e: torch.Tensor, n_layers: int, out: torch.Tensor, tmp_a: torch.Tensor,
               tmp_b: torch.Tensor) -> torch.Tensor:
    """The mean of e, A e, ..., A^n_layers e as a Horner chain of n_layers launches into out (tmp_a, tmp_b: two
    tables of e's shape). The adjacency is symmetric, so this is also the backward of itself."""
    if not 1 <= n_layers <= 8:
        raise ValueError(f"lgcn: n_layers {n_layers} is not served; served: 1 to 8")
    x = e
    for k in range(n_layers):
        last = k == n_layers - 1
        dst = out if last else (tmp_a if k % 2 == 0 else tmp_b)
        lgcn_propagate(graph, x, e, dst, 1.0 / (n_layers + 1) if last else 1.0)
        x = dst
    return out


def lgcn_bpr_plan(users, pos, neg, n_users: int):
    """Host plan of one batch for lgcn_bpr: (slots int32 [3 nb], seg_off int32 [n_seg + 1]) -- the occurrence ids
    role * nb + b (role 0 user, 1 positive, 2 negative) grouped by node and ascending within a node (a stable sort
    by node id), and the groups' bounds."""
    import numpy as np
    node = np.concatenate([np.asarray(users, np.int64), np.asarray(pos, np.int64) + n_users,
                           np.asarray(neg, np.int64) + n_users])
    order = np.argsort(node, kind="stable")
    srt = node[order]
    starts = np.flatnonzero(np.concatenate([[True], srt[1:] != srt[:-1]]))
    return order.astype(np.int32), np.concatenate([starts, [len(node)]]).astype(np.int32)


def lgcn_bpr(F: torch.Tensor, n_users: int, users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, reg: float,
             g: torch.Tensor | None = None, loss_accum: torch.Tensor | None = None, plan=None, n_seg: int | None = None):
    """(loss fp32 [1], g) of one BPR batch over the propagated table F (hvae_lgcn_bpr): g [n_nodes, d] is cleared
    and holds the gradient with respect to F; the loss is also added to loss_accum (fp64 [1]) when given. plan:
    device (slots, seg_off) of lgcn_bpr_plan with n_seg groups; built here from the indices (one device-to-host
    copy) when not given."""
    require_hip(F, users, pos, neg, g, loss_accum)
    n_nodes, d = F.shape
    if d not in LGCN_DIMS:
        raise ValueError(f"lgcn: embedding_dim {d} is not served; served: {LGCN_DIMS[0]} and {LGCN_DIMS[1]}")
    nb = users.numel()
    if not 1 <= nb <= _lib.LGCN_MAX_BATCH or pos.numel() != nb or neg.numel() != nb:
        raise ValueError(f"lgcn_bpr: a batch of {nb} triples (served: 1 to {_lib.LGCN_MAX_BATCH}, three equal lengths)")
    for t in (users, pos, neg):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert F.dtype == torch.float32 and F.is_contiguous()
    if plan is None:
        s, o = lgcn_bpr_plan(users.cpu().numpy(), pos.cpu().numpy(), neg.cpu().numpy(), n_users)
        plan, n_seg = (torch.as_tensor(s, device=F.device), torch.as_tensor(o, device=F.device)), len(o) - 1
    slots, seg_off = plan
    assert slots.dtype == torch.int32 and seg_off.dtype == torch.int32
    assert slots.numel() >= 3 * nb and seg_off.numel() >= n_seg + 1
    if g is None:
        g = torch.empty_like(F)
    assert g.shape == F.shape and g.dtype == torch.float32 and g.is_contiguous()
    assert loss_accum is None or loss_accum.dtype == torch.float64
    loss = torch.empty(1, dtype=torch.float32, device=F.device)
    ws = workspace(F.device, lib().hvae_lgcn_bpr_workspace(nb))
    check(lib().hvae_lgcn_bpr(ptr(F), n_users, n_nodes - n_users, d, ptr(users), ptr(pos), ptr(neg), nb, ptr(slots),
                              ptr(seg_off), int(n_seg), float(reg), ptr(g), ptr(loss), ptr(loss_accum), ptr(ws),
                              ws.numel(), stream_of(F)), "hvae_lgcn_bpr")
    return loss, g


# ---------------------------------------------------------------------- SVD --
SVD_LD = _lib.SVD_LD  # the fixed leading dimension of a tall fp64 matrix (include/hvae.h HVAE_SVD_LD)


def _svd_width(what: str, W: int) -> int:
    if not 1 <= int(W) <= SVD_LD:
        raise ValueError(f"{what}: W = {W} is not served; served: 1 to {SVD_LD} live columns")
    return int(W)


def _svd_tall(what: str, name: str, t: torch.Tensor, n: int | None = None):
    require_hip(t)
    if t.dtype != torch.float64:
        raise ValueError(f"{what}: {name} must be float64, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != SVD_LD or not t.is_contiguous() or (n is not None and t.shape[0] != n) \
            or t.shape[0] < 1:
        raise ValueError(f"{what}: {name} must be a contiguous [{'n' if n is None else n}, {SVD_LD}] matrix (leading "
                         f"dimension {SVD_LD}), got {tuple(t.shape)} with strides {tuple(t.stride())}")


def _svd_alias(what: str, a: torch.Tensor, b: torch.Tensor, names: str):
    a0, b0 = a.data_ptr(), b.data_ptr()
    if a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size():
        raise ValueError(f"{what}: {names} may not alias (their memory overlaps)")


def svd_tall(n: int, device, src=None) -> torch.Tensor:
    """A zeroed [n, SVD_LD] fp64 device matrix; with src (a host [n, W] array) its first W columns filled."""
    t = torch.zeros(n, SVD_LD, dtype=torch.float64, device=device)
    if src is not None:
        t[:, :src.shape[1]] = torch.as_tensor(src, dtype=torch.float64).to(device)
    return t


def svd_spmm(m, X: torch.Tensor, W: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """out [n_rows, 64] = m X in fp64 over the compressed image m (hvae_svd_spmm): a Csr gives A X (X [n_items, 64]),
    a Csc gives A^T X (X [n_users, 64]). out may not alias X."""
    if isinstance(m, Csr):
        if m.rows is not None:
            raise ValueError("svd_spmm: the CSR must hold the whole matrix, not a batch view")
        p, idx, vals, n_rows, n_cols = m.row_ptr, m.col_idx, m.vals, m.nb, m.n_items
    elif isinstance(m, Csc):
        p, idx, vals, n_rows, n_cols = m.col_ptr, m.row_idx, m.vals, m.n_items, m.n_users
    else:
        raise TypeError("svd_spmm takes an ops.Csr or an ops.Csc")
    W = _svd_width("svd_spmm", W)
    _svd_tall("svd_spmm", "X", X, n_cols)
    if out is None:
        out = torch.empty(n_rows, SVD_LD, dtype=torch.float64, device=X.device)
    require_hip(out)
    _svd_alias("svd_spmm", X, out, "X and out")
    _svd_tall("svd_spmm", "out", out, n_rows)
    if p.numel() != n_rows + 1 or idx.numel() != vals.numel():
        raise ValueError("svd_spmm: the compressed image is inconsistent")
    if idx.numel() == 0:
        return out.zero_()
    check(lib().hvae_svd_spmm(ptr(p), ptr(idx), ptr(vals), n_rows, n_cols, ptr(X), ptr(out), W, stream_of(X)),
          "hvae_svd_spmm")
    return out


def svd_gram(Y: torch.Tensor, W: int, G: torch.Tensor | None = None) -> torch.Tensor:
    """G [64, 64] fp64 = Y^T Y, zero outside W x W, exactly symmetric (hvae_svd_gram)."""
    W = _svd_width("svd_gram", W)
    _svd_tall("svd_gram", "Y", Y)
    if G is None:
        G = torch.empty(SVD_LD, SVD_LD, dtype=torch.float64, device=Y.device)
    _svd_tall("svd_gram", "G", G, SVD_LD)
    _svd_alias("svd_gram", Y, G, "Y and G")
    n = Y.shape[0]
    ws = workspace(Y.device, lib().hvae_svd_gram_workspace(n))
    check(lib().hvae_svd_gram(ptr(Y), n, W, ptr(G), ptr(ws), ws.numel(), stream_of(Y)), "hvae_svd_gram")
    return G


def svd_chol_inv(G: torch.Tensor, W: int, flag: torch.Tensor, Rinv: torch.Tensor | None = None) -> torch.Tensor:
    """Rinv [64, 64] fp64 = R^-1 with G[:W, :W] = R^T R (hvae_svd_chol_inv); flag (int32 [1], device) is set to 1
    where G is not positive definite to working precision and is never cleared here."""
    W = _svd_width("svd_chol_inv", W)
    _svd_tall("svd_chol_inv", "G", G, SVD_LD)
    require_hip(flag)
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError(f"svd_chol_inv: flag must be one int32, got {tuple(flag.shape)} {flag.dtype}")
    if Rinv is None:
        Rinv = torch.empty_like(G)
    _svd_tall("svd_chol_inv", "Rinv", Rinv, SVD_LD)
    _svd_alias("svd_chol_inv", G, Rinv, "G and Rinv")
    check(lib().hvae_svd_chol_inv(ptr(G), W, ptr(Rinv), ptr(flag), stream_of(G)), "hvae_svd_chol_inv")
    return Rinv


def svd_apply(Y: torch.Tensor, W: int, T: torch.Tensor, W_out: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[:, :W_out] = Y[:, :W] T[:W, :W_out], zeros from W_out up (hvae_svd_apply); out may be Y (in place), T may
    alias neither."""
    W = _svd_width("svd_apply", W)
    W_out = _svd_width("svd_apply", W_out)
    _svd_tall("svd_apply", "Y", Y)
    _svd_tall("svd_apply", "T", T, SVD_LD)
    if out is None:
        out = torch.empty_like(Y)
    _svd_tall("svd_apply", "out", out, Y.shape[0])
    _svd_alias("svd_apply", T, Y, "T and Y")
    _svd_alias("svd_apply", T, out, "T and out")
    check(lib().hvae_svd_apply(ptr(Y), Y.shape[0], W, ptr(T), W_out, ptr(out), stream_of(Y)), "hvae_svd_apply")
    return out


def svd_orthonormalize(Y: torch.Tensor, W: int, flag: torch.Tensor, G: torch.Tensor | None = None,
                       Rinv: torch.Tensor | None = None) -> torch.Tensor:
    """CholeskyQR2 in place: Y's W live columns orthonormalised by gram -> chol_inv -> apply, twice. Sound while the
    condition number of Y^T Y stays far below 2^53 (the sketches of the subspace iteration: at most a few thousand);
    linearly dependent columns set flag. G, Rinv: two [64, 64] fp64 buffers to reuse."""
    for _ in range(2):
        G = svd_gram(Y, W, G)
        Rinv = svd_chol_inv(G, W, flag, Rinv)
        svd_apply(Y, W, Rinv, W, out=Y)
    return Y


# ----------------------------------------------------------------- Mult-VAE --
MVAE_MAX_HIDDEN = 2048  # hvae_mvae_encoder_fwd (include/hvae.h)
MVAE_MAX_LATENT = 1024


def _mvae_width(what: str, name: str, W: int, hi: int) -> int:
    if not (4 <= int(W) <= hi and int(W) % 4 == 0):
        raise ValueError(f"{what}: {name} = {W} is not served; served: multiples of 4 from 4 to {hi}")
    return int(W)


def _mvae_mat(what: str, name: str, t: torch.Tensor | None, nb: int, W: int, contiguous: bool = False):
    if t is None:
        return
    require_hip(t)
    if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (nb, W) or t.stride(1) != 1 \
            or t.stride(0) % 4 or t.stride(0) < W or t.data_ptr() % 16 or (contiguous and t.stride(0) != W):
        raise ValueError(f"{what}: {name} must be a float32 [{nb}, {W}] matrix with unit column stride, a leading "
                         f"dimension that is a multiple of 4{' and equal to its width' if contiguous else ''} and a "
                         f"16-byte aligned base, got {tuple(t.shape)} {t.dtype} with strides {tuple(t.stride())}")


def mvae_encoder_fwd(x: Csr, w1t: torch.Tensor, b1: torch.Tensor, p_in: float, p_drop: float, train: bool,
                     seed: int = 0, step=None, in_mult=None, drop_mult=None, xs_out=None, t_out=None, h_out=None,
                     save: bool = True):
    """The Mult-VAE first layer over sparse rows (hvae_mvae_encoder_fwd) -> (h [nb, H], t [nb, H] or None, xs or
    None). xs and in_mult are indexed like x.vals; drop_mult is [nb, H]."""
    what = "mvae_encoder_fwd"
    require_hip(w1t, b1, in_mult, drop_mult, xs_out, t_out, h_out)
    if w1t.dim() != 2 or not w1t.is_contiguous() or w1t.shape[0] != x.n_items or w1t.dtype != torch.float32:
        raise ValueError(f"{what}: w1t must be a contiguous float32 [n_items = {x.n_items}, H] matrix, got "
                         f"{tuple(w1t.shape)}")
    H = _mvae_width(what, "H", w1t.shape[1], MVAE_MAX_HIDDEN)
    if tuple(b1.shape) != (H,) or not b1.is_contiguous():
        raise ValueError(f"{what}: b1 must be a contiguous [{H}] vector, got {tuple(b1.shape)}")
    if in_mult is not None and (in_mult.numel() != x.vals.numel() or in_mult.dtype != torch.float32):
        raise ValueError(f"{what}: in_mult must be float32 and indexed like x.vals ({x.vals.numel()} entries)")
    dev = w1t.device
    if h_out is None:
        h_out = torch.empty(x.nb, H, device=dev)
    if t_out is None and save:
        t_out = torch.empty(x.nb, H, device=dev)
    if xs_out is None and save:
        xs_out = torch.empty_like(x.vals)
    if xs_out is not None and (xs_out.numel() != x.vals.numel() or xs_out.dtype != torch.float32):
        raise ValueError(f"{what}: xs_out must be float32 and indexed like x.vals ({x.vals.numel()} entries)")
    for name, t in (("drop_mult", drop_mult), ("t_out", t_out), ("h_out", h_out)):
        _mvae_mat(what, name, t, x.nb, H, contiguous=True)
    check(lib().hvae_mvae_encoder_fwd(x.ref, ptr(w1t), ptr(b1), H, float(p_in), float(p_drop), ptr(in_mult),
                                      ptr(drop_mult), int(seed), ptr(step), int(train), ptr(xs_out), ptr(t_out),
                                      ptr(h_out), stream_of(w1t)), "hvae_mvae_encoder_fwd")
    return h_out, t_out, xs_out


def mvae_tanh_drop_fwd(a: torch.Tensor, p_drop: float, train: bool, tag: int, seed: int = 0, step=None,
                       drop_mult=None, t_out=None, h_out=None):
    """t = tanh(a), h = t * mult over [nb, W] views (hvae_mvae_tanh_drop_fwd) -> (h, t). t_out may be a; without a
    mask h_out may be t_out (the default then: one tensor)."""
    what = "mvae_tanh_drop_fwd"
    nb, W = a.shape
    _mvae_width(what, "W", W, 1 << 24)
    masked = bool(train) and (drop_mult is not None or p_drop > 0)
    if t_out is None:
        t_out = torch.empty(nb, W, device=a.device)
    if h_out is None:
        h_out = torch.empty(nb, W, device=a.device) if masked else t_out
    if t_out.stride(0) != h_out.stride(0):
        raise ValueError(f"{what}: t_out and h_out must share a leading dimension")
    _mvae_mat(what, "a", a, nb, W)
    _mvae_mat(what, "t_out", t_out, nb, W)
    _mvae_mat(what, "h_out", h_out, nb, W)
    _mvae_mat(what, "drop_mult", drop_mult, nb, W, contiguous=True)
    if masked and h_out.data_ptr() in (t_out.data_ptr(), a.data_ptr()):
        raise ValueError(f"{what}: h_out may alias t_out or a only without a mask")
    check(lib().hvae_mvae_tanh_drop_fwd(ptr(a), a.stride(0), nb, W, float(p_drop), ptr(drop_mult), int(seed),
                                        ptr(step), int(tag), int(train), ptr(t_out), ptr(h_out), h_out.stride(0),
                                        stream_of(a)), "hvae_mvae_tanh_drop_fwd")
    return h_out, t_out


def mvae_tanh_drop_bwd(dh: torch.Tensor, t: torch.Tensor, p_drop: float, train: bool, tag: int, seed: int = 0,
                       step=None, drop_mult=None, da=None):
    """da = dh * mult * (1 - t^2) (hvae_mvae_tanh_drop_bwd); da may be dh."""
    what = "mvae_tanh_drop_bwd"
    nb, W = t.shape
    _mvae_width(what, "W", W, 1 << 24)
    if da is None:
        da = torch.empty(nb, W, device=t.device)
    _mvae_mat(what, "dh", dh, nb, W)
    _mvae_mat(what, "t", t, nb, W)
    _mvae_mat(what, "da", da, nb, W)
    _mvae_mat(what, "drop_mult", drop_mult, nb, W, contiguous=True)
    if da.data_ptr() == t.data_ptr():
        raise ValueError(f"{what}: da may alias dh, not t")
    check(lib().hvae_mvae_tanh_drop_bwd(ptr(dh), dh.stride(0), ptr(t), t.stride(0), nb, W, float(p_drop),
                                        ptr(drop_mult), int(seed), ptr(step), int(tag), int(train), ptr(da),
                                        da.stride(0), stream_of(t)), "hvae_mvae_tanh_drop_bwd")
    return da


def mvae_nll(x: Csr, S: torch.Tensor, grad_scale: float, lse=None, recon_rows=None):
    """The multinomial loss against the sparse rows x and its gradient, in place over the stored logits S [nb, >= N]
    (hvae_mvae_nll) -> (lse [nb], recon_rows [nb]); S[:, :N] becomes grad_scale * (n softmax(S) - x). No column may
    occur twice in a row of x."""
    require_hip(S, lse, recon_rows)
    if S.dtype != torch.float32 or S.dim() != 2 or S.shape[0] != x.nb or S.stride(1) != 1 or S.shape[1] < x.n_items \
            or S.stride(0) < S.shape[1]:
        raise ValueError(f"mvae_nll: S must be a float32 [nb = {x.nb}, >= {x.n_items}] matrix with unit column "
                         f"stride, got {tuple(S.shape)} {S.dtype} with strides {tuple(S.stride())}")
    if lse is None:
        lse = torch.empty(x.nb, device=S.device)
    if recon_rows is None:
        recon_rows = torch.empty(x.nb, device=S.device)
    if lse.numel() != x.nb or recon_rows.numel() != x.nb:
        raise ValueError(f"mvae_nll: lse and recon_rows must hold nb = {x.nb} floats")
    check(lib().hvae_mvae_nll(x.ref, ptr(S), S.stride(0), float(grad_scale), ptr(lse), ptr(recon_rows),
                              stream_of(S)), "hvae_mvae_nll")
    return lse, recon_rows


# -------------------------------------------------------------------- t-SNE --
TSNE_SERVED = (f"served: {_lib.TSNE_MIN_N} <= n <= {_lib.TSNE_MAX_N} points of {_lib.TSNE_MIN_L} <= L <= "
               f"{_lib.TSNE_MAX_L} columns, 0 < perplexity < n, k = min(n - 1, int(3 * perplexity + 1)) <= "
               f"{_lib.TSNE_MAX_K} neighbours")


def tsne_neighbours(n: int, L: int | None, perplexity: float, what: str = "tsne") -> int:
    """k = min(n - 1, int(3 * perplexity + 1)), scikit-learn's neighbour count, for a served shape; a ValueError that
    names the served range otherwise (before any launch)."""
    n, perplexity = int(n), float(perplexity)
    if not _lib.TSNE_MIN_N <= n <= _lib.TSNE_MAX_N:
        raise ValueError(f"{what}: n = {n} points is not served; {TSNE_SERVED}")
    if L is not None and not _lib.TSNE_MIN_L <= int(L) <= _lib.TSNE_MAX_L:
        raise ValueError(f"{what}: L = {L} columns is not served; {TSNE_SERVED}")
    if not 0.0 < perplexity < n:
        raise ValueError(f"{what}: perplexity = {perplexity} with n = {n} is not served; {TSNE_SERVED}")
    k = min(n - 1, int(3.0 * perplexity + 1))
    if not 1 <= k <= _lib.TSNE_MAX_K:
        raise ValueError(f"{what}: perplexity = {perplexity} needs k = {k} neighbours, which is not served; "
                         f"{TSNE_SERVED}")
    return k


def _tsne_mat(what: str, name: str, t: torch.Tensor, n: int, w: int, dtype=torch.float64):
    require_hip(t)
    if t.dtype != dtype or t.dim() != 2 or tuple(t.shape) != (n, w) or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} [{n}, {w}] matrix, got {tuple(t.shape)} "
                         f"{t.dtype} with strides {tuple(t.stride())}")


def tsne_knn(X: torch.Tensor, perplexity: float):
    """The k = min(n - 1, int(3 perplexity + 1)) nearest other rows of each row of X (fp32 [n, L], unit column
    stride) by squared Euclidean distance in fp64 (hvae_tsne_knn) -> (idx int32 [n, k], d2 float64 [n, k]), each row
    ascending by (distance, index)."""
    if X.dim() != 2:
        raise ValueError(f"tsne_knn: X must be a float32 [n, L] matrix, got {tuple(X.shape)}; {TSNE_SERVED}")
    n, L = X.shape
    k = tsne_neighbours(n, L, perplexity, "tsne_knn")
    require_hip(X)
    if X.dtype != torch.float32 or X.stride(1) != 1 or X.stride(0) < L:
        raise ValueError(f"tsne_knn: X must be float32 with unit column stride, got {X.dtype} with strides "
                         f"{tuple(X.stride())}")
    idx = torch.empty(n, k, dtype=torch.int32, device=X.device)
    d2 = torch.empty(n, k, dtype=torch.float64, device=X.device)
    ws = workspace(X.device, lib().hvae_tsne_knn_workspace(n))
    check(lib().hvae_tsne_knn(ptr(X), n, L, X.stride(0), k, ptr(idx), ptr(d2), ptr(ws), ws.numel(), stream_of(X)),
          "hvae_tsne_knn")
    return idx, d2


def tsne_perplexity(d2: torch.Tensor, perplexity: float) -> torch.Tensor:
    """The conditional P [n, k] of the neighbour distances d2 [n, k]: scikit-learn's binary search for the
    perplexity, one row per wave (hvae_tsne_perplexity)."""
    if d2.dim() != 2:
        raise ValueError(f"tsne_perplexity: d2 must be a float64 [n, k] matrix, got {tuple(d2.shape)}")
    n, k = d2.shape
    if k != tsne_neighbours(n, None, perplexity, "tsne_perplexity"):
        raise ValueError(f"tsne_perplexity: d2 holds {k} neighbours per row, perplexity = {perplexity} takes "
                         f"{tsne_neighbours(n, None, perplexity)}; {TSNE_SERVED}")
    _tsne_mat("tsne_perplexity", "d2", d2, n, k)
    P = torch.empty_like(d2)
    check(lib().hvae_tsne_perplexity(ptr(d2), n, k, float(perplexity), ptr(P), stream_of(d2)), "hvae_tsne_perplexity")
    return P


class TsneP:
    """The symmetric joint P as a device CSR with sorted columns: ptr int64 [n + 1], col int32, val float64."""

    def __init__(self, row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor):
        require_hip(row_ptr, col, val)
        if row_ptr.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float64 \
                or col.numel() != val.numel():
            raise ValueError("TsneP: ptr int64, col int32 and val float64 of equal length are needed")
        self.ptr, self.col, self.val, self.n = row_ptr, col, val, row_ptr.numel() - 1

    def to_scipy(self):
        from scipy.sparse import csr_matrix
        return csr_matrix((self.val.cpu().numpy(), self.col.cpu().numpy(), self.ptr.cpu().numpy()),
                          shape=(self.n, self.n))


def tsne_joint(idx: torch.Tensor, cond: torch.Tensor) -> TsneP:
    """P = (P_cond + P_cond^T) / max(sum, eps) as a CSR with sorted columns: the fit's one host step (scipy on the
    downloaded [n, k] arrays, one upload), as scikit-learn's _joint_probabilities_nn forms it."""
    import numpy as np
    from scipy.sparse import csr_matrix
    idx_h, c = idx.cpu().numpy(), cond.cpu().numpy()
    n, k = idx_h.shape
    if idx_h.min() < 0 or not np.isfinite(c).all():
        raise ValueError("tsne_joint: the input holds non-finite values (a row found fewer than k neighbours)")
    P = csr_matrix((c.ravel(), idx_h.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    P.sort_indices()
    P = P + P.T
    P /= np.maximum(P.sum(), np.finfo(np.double).eps)
    P.sort_indices()
    dev = idx.device
    return TsneP(torch.as_tensor(P.indptr.astype(np.int64), device=dev),
                 torch.as_tensor(P.indices.astype(np.int32), device=dev),
                 torch.as_tensor(P.data.astype(np.float64), device=dev))


def tsne_forces(Y: torch.Tensor, P: TsneP, attr=None, rep=None, z=None):
    """One force evaluation at the embedding Y [n, 2] (hvae_tsne_forces) -> (attr [n, 2], rep [n, 2], z [n])."""
    if Y.dim() != 2:
        raise ValueError(f"tsne_forces: Y must be a float64 [n, 2] matrix, got {tuple(Y.shape)}")
    n = Y.shape[0]
    if not _lib.TSNE_MIN_N <= n <= _lib.TSNE_MAX_N or P.n != n:
        raise ValueError(f"tsne_forces: n = {n} points (P holds {P.n} rows) is not served; {TSNE_SERVED}")
    _tsne_mat("tsne_forces", "Y", Y, n, 2)
    attr = torch.empty_like(Y) if attr is None else attr
    rep = torch.empty_like(Y) if rep is None else rep
    z = torch.empty(n, dtype=torch.float64, device=Y.device) if z is None else z
    _tsne_mat("tsne_forces", "attr", attr, n, 2)
    _tsne_mat("tsne_forces", "rep", rep, n, 2)
    _tsne_mat("tsne_forces", "z", z.view(n, 1) if z.dim() == 1 else z, n, 1)
    check(lib().hvae_tsne_forces(ptr(Y), n, ptr(P.ptr), ptr(P.col), ptr(P.val), ptr(attr), ptr(rep), ptr(z),
                                 stream_of(Y)), "hvae_tsne_forces")
    return attr, rep, z


def tsne_update(attr, rep, z, gains, upd, y_in, y_out, exaggeration: float, momentum: float, lr: float,
                P: TsneP | None = None, stats: torch.Tensor | None = None, grad_out=None, z_out=None):
    """scikit-learn's gradient-descent step from one force evaluation (hvae_tsne_update): gains and upd in place,
    y_out = y_in + update. With stats (float64 [2], device; P is then needed) it receives the KL error at y_in and
    the gradient norm after the gains; grad_out [n, 2] receives the gradient before the gains, z_out [1] receives Z."""
    n = y_in.shape[0]
    if not _lib.TSNE_MIN_N <= n <= _lib.TSNE_MAX_N:
        raise ValueError(f"tsne_update: n = {n} points is not served; {TSNE_SERVED}")
    for name, t in (("attr", attr), ("rep", rep), ("gains", gains), ("upd", upd), ("y_in", y_in), ("y_out", y_out)):
        _tsne_mat("tsne_update", name, t, n, 2)
    if grad_out is not None:
        _tsne_mat("tsne_update", "grad_out", grad_out, n, 2)
    _tsne_mat("tsne_update", "z", z.view(n, 1), n, 1)
    if y_in.data_ptr() == y_out.data_ptr():
        raise ValueError("tsne_update: y_out may not alias y_in")
    want = stats is not None
    ws = None
    if want:
        if P is None or P.n != n or stats.dtype != torch.float64 or stats.numel() != 2:
            raise ValueError("tsne_update: the statistics need P over the same n points and a float64 [2] stats")
        require_hip(stats)
        ws = workspace(y_in.device, lib().hvae_tsne_update_workspace(n))
    if z_out is not None and (z_out.dtype != torch.float64 or z_out.numel() != 1):
        raise ValueError("tsne_update: z_out must be one float64")
    check(lib().hvae_tsne_update(ptr(attr), ptr(rep), ptr(z), n, float(exaggeration), float(momentum), float(lr),
                                 ptr(gains), ptr(upd), ptr(y_in), ptr(y_out), ptr(P.ptr) if want else None,
                                 ptr(P.col) if want else None, ptr(P.val) if want else None, int(want), ptr(stats),
                                 ptr(grad_out), ptr(z_out), ptr(ws), ws.numel() if want else 0, stream_of(y_in)),
          "hvae_tsne_update")
    return y_out


# -------------------------------------------------------------------- SBERT --
SBERT_MAX_LEN, SBERT_MAX_H, SBERT_CHUNK = 512, 1024, 64  # csrc/hvae_sbert.hip kSbMaxLen, kSbMaxH, kSbQB
SBERT_SERVED = (f"served: head width 32 or 64, H a multiple of 4 up to {SBERT_MAX_H}, sequences of 1 to "
                f"{SBERT_MAX_LEN} tokens")


def sbert_supported(H: int, heads: int, max_len: int) -> bool:
    return bool(lib().hvae_sbert_supported(int(H), int(heads), int(max_len)))


class SbertPack:
    """The packed sequences of one pass: ids int32 [T], cu int32 [S + 1] and the attention's work list int32
    [n_work, 2] of (sequence, 64-query chunk) pairs, on the device. Built from host arrays, so that what the device
    cannot report is refused here: an id below 0 (the upper bound is checked against the table in sbert_embed_ln), an
    empty sequence or a non-monotone cu, a sequence of more than 512 tokens."""

    def __init__(self, ids, cu, device):
        import numpy as np
        ids = np.ascontiguousarray(ids)
        cu = np.ascontiguousarray(cu)
        if ids.ndim != 1 or cu.ndim != 1 or cu.size < 2 or ids.dtype.kind not in "iu" or cu.dtype.kind not in "iu":
            raise ValueError("SbertPack: ids [T] and cu [S + 1] must be integer vectors")
        ids, cu = ids.astype(np.int64), cu.astype(np.int64)
        if cu[0] != 0 or cu[-1] != ids.size or (np.diff(cu) < 1).any():
            raise ValueError(f"SbertPack: cu must start at 0, end at T = {ids.size} and increase strictly "
                             f"(no empty sequence); got cu[0] = {cu[0]}, cu[-1] = {cu[-1]}, smallest step "
                             f"{int(np.diff(cu).min())}")
        lens = np.diff(cu)
        if lens.max() > SBERT_MAX_LEN:
            raise ValueError(f"SbertPack: a sequence of {int(lens.max())} tokens is not served; {SBERT_SERVED}")
        if ids.size and ids.min() < 0:
            raise ValueError(f"SbertPack: token id {int(ids.min())} is outside [0, vocab)")
        self.S, self.T = int(cu.size - 1), int(ids.size)
        self.max_len, self.id_max = int(lens.max()), int(ids.max())
        chunks = (lens + SBERT_CHUNK - 1) // SBERT_CHUNK
        seq = np.repeat(np.arange(self.S), chunks)
        first = np.repeat(np.cumsum(chunks) - chunks, chunks)
        work = np.stack([seq, np.arange(seq.size) - first], axis=1).astype(np.int32)
        self.n_work = int(work.shape[0])
        self.ids = torch.as_tensor(ids.astype(np.int32), device=device)
        self.cu = torch.as_tensor(cu.astype(np.int32), device=device)
        self.work = torch.as_tensor(work, device=device)
        require_hip(self.ids)


def _sbert_mat(what: str, name: str, t: torch.Tensor, rows: int, cols: int):
    require_hip(t)
    if t.dtype != torch.float32 or tuple(t.shape) != (rows, cols) or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{what}: {name} must be a contiguous, 16-byte aligned float32 [{rows}, {cols}] matrix, got "
                         f"{tuple(t.shape)} {t.dtype} with strides {tuple(t.stride())}")


def _sbert_width(what: str, H: int, T: int) -> None:
    if H < 4 or H > SBERT_MAX_H or H % 4:
        raise ValueError(f"{what}: H = {H} is not served; {SBERT_SERVED}")
    if 3 * H * T >= 2 ** 31:
        raise ValueError(f"{what}: T = {T} rows of width {H} in one pass is not served (3 H T < 2^31)")


def sbert_embed_ln(pack: SbertPack, word, pos, type0, ln_w, ln_b, eps: float, out=None):
    """out[t] = LayerNorm(word[ids[t]] + pos[t - cu[s]] + type0) over the packed rows (hvae_sbert_embed_ln)."""
    what = "sbert_embed_ln"
    if word.dim() != 2 or pos.dim() != 2:
        raise ValueError(f"{what}: word [vocab, H] and pos [max_pos, H] must be matrices")
    vocab, H = word.shape
    _sbert_width(what, H, pack.T)
    _sbert_mat(what, "word", word, vocab, H)
    _sbert_mat(what, "pos", pos, pos.shape[0], H)
    for name, v in (("type0", type0), ("ln_w", ln_w), ("ln_b", ln_b)):
        _sbert_mat(what, name, v.view(1, -1), 1, H)
    if pack.id_max >= vocab:
        raise ValueError(f"{what}: token id {pack.id_max} is outside [0, vocab = {vocab})")
    if pack.max_len > pos.shape[0]:
        raise ValueError(f"{what}: a sequence of {pack.max_len} tokens is longer than the position table "
                         f"({pos.shape[0]} rows)")
    out = torch.empty(pack.T, H, device=word.device) if out is None else out
    _sbert_mat(what, "out", out, pack.T, H)
    check(lib().hvae_sbert_embed_ln(ptr(pack.ids), ptr(pack.cu), pack.S, pack.T, ptr(word), vocab, ptr(pos),
                                    pos.shape[0], ptr(type0), ptr(ln_w), ptr(ln_b), float(eps), H, ptr(out),
                                    stream_of(word)), "hvae_sbert_embed_ln")
    return out


def sbert_add_ln(x, res, ln_w, ln_b, eps: float, out=None):
    """out = LayerNorm(x + res) per row (hvae_sbert_add_ln); out may be x or res."""
    what = "sbert_add_ln"
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be a float32 [T, H] matrix")
    T, H = x.shape
    _sbert_width(what, H, T)
    out = torch.empty_like(x) if out is None else out
    for name, t in (("x", x), ("res", res), ("out", out)):
        _sbert_mat(what, name, t, T, H)
    for name, v in (("ln_w", ln_w), ("ln_b", ln_b)):
        _sbert_mat(what, name, v.view(1, -1), 1, H)
    check(lib().hvae_sbert_add_ln(ptr(x), ptr(res), ptr(ln_w), ptr(ln_b), float(eps), T, H, ptr(out), stream_of(x)),
          "hvae_sbert_add_ln")
    return out


def sbert_attention(qkv, pack: SbertPack, heads: int, ctx=None, rel=None, rel_len=None):
    """ctx [T, H] = softmax(Q K^T / sqrt(dh)) V inside each sequence and head, from qkv [T, 3 H]
    (hvae_sbert_attention). ctx may have more than T rows: rows from T on are not touched.

    With rel, a float32 [heads, 2 L - 1] table (L = rel_len, 1 .. 512), score (query i, key j) of head h gets
    rel[h][(j - i) + L - 1] added after the scale (hvae_sbert_attention_relbias, MPNet's relative-position bias). The
    device leaves a sequence longer than L untouched and cannot report it, so a pack that holds one is refused here."""
    what = "sbert_attention"
    if (rel is None) != (rel_len is None):
        raise ValueError(f"{what}: rel and rel_len are given together or not at all")
    if qkv.dim() != 2 or qkv.shape[1] % 3:
        raise ValueError(f"{what}: qkv must be a float32 [T, 3 H] matrix, got {tuple(qkv.shape)}")
    H = qkv.shape[1] // 3
    if not sbert_supported(H, heads, pack.max_len):
        raise ValueError(f"{what}: H = {H} with {heads} heads and {pack.max_len} tokens is not served; {SBERT_SERVED}")
    _sbert_width(what, H, pack.T)
    _sbert_mat(what, "qkv", qkv, pack.T, 3 * H)
    ctx = torch.empty(pack.T, H, device=qkv.device) if ctx is None else ctx
    if ctx.dim() != 2 or ctx.shape[0] < pack.T:
        raise ValueError(f"{what}: ctx needs at least {pack.T} rows")
    _sbert_mat(what, "ctx", ctx, ctx.shape[0], H)
    if rel is not None:
        L = int(rel_len)
        if L < 1 or L > SBERT_MAX_LEN:
            raise ValueError(f"{what}: rel_len = {L} is not served (1 .. {SBERT_MAX_LEN})")
        require_hip(rel)
        if rel.dtype != torch.float32 or tuple(rel.shape) != (int(heads), 2 * L - 1) or not rel.is_contiguous():
            raise ValueError(f"{what}: rel must be a contiguous float32 [{int(heads)}, {2 * L - 1}] matrix (heads, "
                             f"2 rel_len - 1), got {tuple(rel.shape)} {rel.dtype} with strides {tuple(rel.stride())}")
        if pack.max_len > L:
            raise ValueError(f"{what}: a sequence of {pack.max_len} tokens is longer than the relative-bias table "
                             f"covers (rel_len = {L})")
        check(lib().hvae_sbert_attention_relbias(ptr(qkv), ptr(pack.cu), pack.S, pack.T, H, int(heads),
                                                 ptr(pack.work), pack.n_work, ptr(rel), L, ptr(ctx),
                                                 stream_of(qkv)), "hvae_sbert_attention_relbias")
        return ctx
    check(lib().hvae_sbert_attention(ptr(qkv), ptr(pack.cu), pack.S, pack.T, H, int(heads), ptr(pack.work),
                                     pack.n_work, ptr(ctx), stream_of(qkv)), "hvae_sbert_attention")
    return ctx


def sbert_pool_norm(x, pack: SbertPack, out=None):
    """out[s] = the mean of sequence s's rows of x, divided by max(its L2 norm, 1e-12) (hvae_sbert_pool_norm)."""
    what = "sbert_pool_norm"
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be a float32 [T, H] matrix")
    H = x.shape[1]
    _sbert_width(what, H, pack.T)
    _sbert_mat(what, "x", x, pack.T, H)
    out = torch.empty(pack.S, H, device=x.device) if out is None else out
    _sbert_mat(what, "out", out, pack.S, H)
    check(lib().hvae_sbert_pool_norm(ptr(x), ptr(pack.cu), pack.S, pack.T, H, ptr(out), stream_of(x)),
          "hvae_sbert_pool_norm")
    return out


# ------------------------------------------------------- preprocessing (K23) --
PREP_MAX_ID_BYTES = _lib.PREP_MAX_ID_BYTES
_PREP_MAX_N = (1 << 31) - 1


def prep_pack_ids(values, what: str = "id"):
    """String ids -> (uint64 [n, W] host array, W): each id's UTF-8 bytes, NUL-padded to 8 W bytes (W = 1 .. 4, the
    smallest that holds the longest id) and read as big-endian 64-bit words, the keys of hvae_prep_encode. Refused
    with a ValueError that names the row: an id that is no str, holds a NUL, or is longer than 32 bytes of UTF-8."""
    import numpy as np
    objs = np.asarray(values, dtype=object)
    if objs.ndim != 1:
        raise ValueError(f"prep_pack_ids: {what} must be one column, got shape {objs.shape}")
    for r, v in enumerate(objs):
        if not isinstance(v, str):
            raise ValueError(f"{what}: row {r}: {v!r} is {type(v).__name__}, not a string")
        if "\x00" in v:
            raise ValueError(f"{what}: row {r}: {v!r} contains NUL")
    n = len(objs)
    raw = np.char.encode(objs.astype(str), "utf-8") if n else np.zeros(0, dtype="S1")
    width = raw.dtype.itemsize
    if width > PREP_MAX_ID_BYTES:
        r = int(np.argmax(np.char.str_len(raw) > PREP_MAX_ID_BYTES))
        raise ValueError(f"{what}: row {r}: {objs[r]!r} is {len(objs[r].encode('utf-8'))} bytes of UTF-8, more than "
                         f"the {PREP_MAX_ID_BYTES} an id may have")
    W = max(1, -(-width // 8))
    buf = np.zeros((n, 8 * W), dtype=np.uint8)
    if n:
        buf[:, :width] = np.frombuffer(raw.tobytes(), dtype=np.uint8).reshape(n, width)
    return buf.view(">u8").astype(np.uint64), W


def prep_unpack_ids(words) -> list[str]:
    """The ids that prep_pack_ids packed."""
    import numpy as np
    words = np.ascontiguousarray(words, dtype=np.uint64)
    rows = words.astype(">u8").view(np.uint8).reshape(len(words), -1)
    return [bytes(r).rstrip(b"\x00").decode("utf-8") for r in rows]


def _prep_vec(what: str, name: str, t: torch.Tensor, dtype, n: int | None = None):
    require_hip(t)
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} vector" + (f" of {n}" if n is not None else "") +
                         f", got {tuple(t.shape)} {t.dtype}")
    if not 1 <= t.numel() <= _PREP_MAX_N:
        raise ValueError(f"{what}: {name} holds {t.numel()} records; served: 1 .. 2^31 - 1")


def _prep_codes(what: str, name: str, t: torch.Tensor, hi: int):
    lo_v, hi_v = (int(x) for x in torch.aminmax(t))
    if lo_v < 0 or hi_v >= hi:
        raise ValueError(f"{what}: {name} must lie in [0, {hi}), got [{lo_v}, {hi_v}]")


def _prep_ws(what: str, dev, nbytes: int) -> torch.Tensor:
    if nbytes <= 0:
        raise ValueError(f"{what}: sizes outside the served range (1 .. 2^31 - 1 records, users and items)")
    ws = workspace(dev, nbytes + 256)
    off = (-ws.data_ptr()) % 256
    return ws[off:off + nbytes]


def prep_encode(keys: torch.Tensor):
    """LabelEncoder.fit + transform on packed ids (keys int64 [n, W]: the bits of prep_pack_ids' words) ->
    (codes int32 [n], first int32 [n_classes]): each id's rank among the distinct ids in ascending byte order, and
    the smallest record index that carries each class (hvae_prep_encode). One read-back, of the class count."""
    require_hip(keys)
    if keys.dtype != torch.int64 or keys.dim() != 2 or not keys.is_contiguous() or not 1 <= keys.shape[1] <= 4:
        raise ValueError(f"prep_encode: keys must be a contiguous int64 [n, 1 .. 4] matrix, got {tuple(keys.shape)} "
                         f"{keys.dtype}")
    n, W = keys.shape
    if not 1 <= n <= _PREP_MAX_N:
        raise ValueError(f"prep_encode: {n} records; served: 1 .. 2^31 - 1")
    dev = keys.device
    codes = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    n_classes = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _prep_ws("prep_encode", dev, lib().hvae_prep_encode_workspace(n, W))
    check(lib().hvae_prep_encode(ptr(keys), n, W, ptr(codes), ptr(n_classes), ptr(first), ptr(ws), ws.numel(),
                                 stream_of(keys)), "hvae_prep_encode")
    return codes, first[:int(n_classes.item())].clone()


def prep_kcore(ucode: torch.Tensor, icode: torch.Tensor, n_users: int, n_items: int, min_user: int = 5,
               min_item: int = 5, max_iterations: int = 10):
    """filter_by_interactions over codes -> (alive bool [n], live count, rounds that removed a record)
    (hvae_prep_kcore). All rounds are enqueued at once; the two counts are read back afterwards."""
    _prep_vec("prep_kcore", "ucode", ucode, torch.int32)
    n = ucode.numel()
    _prep_vec("prep_kcore", "icode", icode, torch.int32, n)
    _prep_codes("prep_kcore", "ucode", ucode, n_users)
    _prep_codes("prep_kcore", "icode", icode, n_items)
    if not 0 <= int(max_iterations) <= 1 << 20:
        raise ValueError(f"prep_kcore: max_iterations = {max_iterations}; served: 0 .. 2^20")
    dev = ucode.device
    alive = torch.empty(n, dtype=torch.uint8, device=dev)
    n_alive = torch.zeros(1, dtype=torch.int64, device=dev)
    rounds = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _prep_ws("prep_kcore", dev, lib().hvae_prep_kcore_workspace(n_users, n_items, int(max_iterations)))
    clamp = lambda v: max(-(1 << 31), min(int(v), (1 << 31) - 1))  # noqa: E731
    check(lib().hvae_prep_kcore(ptr(ucode), ptr(icode), n, n_users, n_items, clamp(min_user), clamp(min_item),
                                int(max_iterations), ptr(alive), ptr(n_alive), ptr(rounds), ptr(ws), ws.numel(),
                                stream_of(ucode)), "hvae_prep_kcore")
    return alive.bool(), int(n_alive.item()), int(rounds.item())


def prep_split(ucode: torch.Tensor, ts: torch.Tensor, n_users: int):
    """leave_one_out_split over (user code, int64 timestamp) -> (perm, train, val, test), int32 record indices: the
    stable (user, timestamp) order, and each part's records in that order (hvae_prep_split)."""
    _prep_vec("prep_split", "ucode", ucode, torch.int32)
    n = ucode.numel()
    _prep_vec("prep_split", "ts", ts, torch.int64, n)
    _prep_codes("prep_split", "ucode", ucode, n_users)
    dev = ucode.device
    perm, train, val, test = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    lens = torch.zeros(3, dtype=torch.int64, device=dev)
    ws = _prep_ws("prep_split", dev, lib().hvae_prep_split_workspace(n))
    check(lib().hvae_prep_split(ptr(ucode), ptr(ts), n, n_users, ptr(perm), ptr(train), ptr(val), ptr(test),
                                ptr(lens), ptr(ws), ws.numel(), stream_of(ucode)), "hvae_prep_split")
    n_train, n_val, n_test = (int(x) for x in lens.tolist())
    return perm, train[:n_train].clone(), val[:n_val].clone(), test[:n_test].clone()


def prep_csr(ucode: torch.Tensor, icode: torch.Tensor, vals: torch.Tensor, n_users: int, n_items: int) -> Csr:
    """create_interaction_matrix: the canonical device CSR [n_users, n_items] of all records, duplicate pairs summed
    in input order, columns ascending, entries that sum to zero kept (hvae_prep_csr)."""
    _prep_vec("prep_csr", "ucode", ucode, torch.int32)
    n = ucode.numel()
    _prep_vec("prep_csr", "icode", icode, torch.int32, n)
    _prep_vec("prep_csr", "vals", vals, torch.float32, n)
    _prep_codes("prep_csr", "ucode", ucode, n_users)
    _prep_codes("prep_csr", "icode", icode, n_items)
    dev = ucode.device
    row_ptr = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _prep_ws("prep_csr", dev, lib().hvae_prep_csr_workspace(n, n_users))
    check(lib().hvae_prep_csr(ptr(ucode), ptr(icode), ptr(vals), n, n_users, n_items, ptr(row_ptr), ptr(col), ptr(out),
                              ptr(nnz), ptr(ws), ws.numel(), stream_of(ucode)), "hvae_prep_csr")
    k = int(nnz.item())
    return Csr(row_ptr, col[:k].clone(), out[:k].clone(), n_items)
