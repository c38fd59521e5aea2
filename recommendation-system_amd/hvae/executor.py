"""Fused, graph-captured HybridVAE train/validation step on MI355X.

Replaces the body of VAETrainer.train_epoch / validate (src/ml/train.py:81-124):
per batch the reference densifies every user row on the host, copies a dense
[B, N] batch to the device, runs ~60 eager aten ops through autograd, clips
with clip_grad_norm_, steps torch.optim.Adam and syncs three times with
.item(). Here one step is a fixed sequence of ~30 libhvae launches over
device-resident data, captured once per batch size into a hipGraph (through
torch.cuda.CUDAGraph) and replayed:

  * the interaction CSR lives in HBM; a batch is a window of a permuted
    user-id array whose start is a device counter (rows_offset), advanced by
    the graph itself -- no host work per step besides the replay;
  * parameters, gradients and Adam moments live in flat fp32 buffers; the
    module's nn.Parameters are rebound to views of the flat parameter buffer,
    so state_dict() and checkpoints always see the current values;
  * the first-layer weight is stored item-major (W1t [N, H]) -- the
    ``encoder.0.weight`` parameter is its [H, N] transposed view -- and its
    gradient is row-sparse (only the batch's items);
  * dropout masks and reparameterisation noise are Philox streams keyed by
    (seed, device step counter), so replays draw fresh randomness;
  * losses accumulate on the device in fp64 and are read once per epoch.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, ops
from ._lib import CsrBatch, Epilogue, GemmDesc, check, lib, ptr

ALIGN = 4  # floats: every flat segment starts 16-B aligned
# A single-GPU deferring step runs its recorded W1t update as a guest under the decoder sweep by default where it
# fits (FusedTrainer._use_guest: the d = 768 bf16 sweep); HVAE_DEFER_AT=guest asks for it either way, data-parallel
# steps included (not measured: they keep "sweep" by default), any other value turns it off. Syn-10M bf16: 10.344 -> 10.131 and, on another device, 10.029 -> 9.891 ms per step, every run of
# three faster, 8.7 x the parent's own range both times (DESIGN.md 4.2 "The recorded update as a guest of the
# sweep", profiles/adam_guest_ab.jsonl).
GUEST_DEFAULT = True
# The hold in front of the guest on its stream (hvae_adam_guest_hold), microseconds. The hold starts when the last
# forward kernel ends (the fork event). In the step's kernel trace the sweep starts 12 us after that kernel's end
# with the fork in the graph (0 us without it) and 6 us after the hold does (medians over 29 steps,
# profiles/adam_guest_ab.jsonl); its 256 blocks are dispatched within a few microseconds more, which a kernel trace
# does not show. The hold is that plus a margin, after which the guest's first block starts 15.5 us behind the sweep's.
GUEST_HOLD_US = 20


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


@dataclass
class Seg:
    name: str
    offset: int
    shape: tuple
    numel: int


class FlatLayout:
    """Parameter layout: W1t [N, H1] first, then the small parameters.

    Small parameters keep the reference's parameter order (src/ml/model.py
    modules() order) except that fc_mu/fc_logvar weights (and biases) are
    adjacent, so that the two heads run as one [2L, H] GEMM.
    """

    def __init__(self, model):
        self.n_items = model.n_items
        self.hidden = list(model.hidden_dims)
        # one hidden layer of at most 512: the shape whose encoder layer the row-parallel MLP forward can take on
        self.one_hidden_512 = len(self.hidden) == 1 and self.hidden[0] <= 512
        self.L = model.latent_dim
        self.d = model.embedding_dim
        self.has_proj = self.L != self.d
        segs: list[Seg] = []
        off = 0

        def add(name, shape, align=True):
            nonlocal off
            n = int(np.prod(shape))
            segs.append(Seg(name, off, tuple(shape), n))
            off = off + (_align(n) if align else n)

        add("w1t", (self.n_items, self.hidden[0]))
        self.small_offset = off
        # trainable item embeddings (HybridVAE(freeze_embeddings=False), reference model.py:72-75): E is the
        # reference's first parameter and has a dense gradient, so it opens the dense segment (clip + Adam cover it)
        self.train_e = bool(getattr(model, "item_embeddings_trainable", False))
        if self.train_e:
            add("item_embeddings", (self.n_items, self.d))
        prev = self.hidden[0]
        for k, hd in enumerate(self.hidden):
            i = 4 * k
            if k > 0:
                add(f"encoder.{i}.weight", (hd, prev))
            add(f"encoder.{i}.bias", (hd,))
            add(f"encoder.{i + 1}.weight", (hd,))
            add(f"encoder.{i + 1}.bias", (hd,))
            prev = hd
        add("fc_mu.weight", (self.L, prev), align=False)
        add("fc_logvar.weight", (self.L, prev))
        add("fc_mu.bias", (self.L,), align=False)
        add("fc_logvar.bias", (self.L,))
        if self.has_proj:
            add("projection_layer.0.weight", (self.d, self.L))
            add("projection_layer.0.bias", (self.d,))
            add("projection_layer.3.weight", (self.d, self.d))
            add("projection_layer.3.bias", (self.d,))
        self.total = off
        self.n_small = off - self.small_offset
        self.segs = {s.name: s for s in segs}

    def view(self, buf: torch.Tensor, name: str, base: int = 0) -> torch.Tensor:
        s = self.segs[name]
        return buf[s.offset - base: s.offset - base + s.numel].view(s.shape)

    def heads(self, buf: torch.Tensor, base: int = 0):
        """(W_heads [2L, H], b_heads [2L]) views spanning fc_mu and fc_logvar."""
        w, b = self.segs["fc_mu.weight"], self.segs["fc_mu.bias"]
        H = w.shape[1]
        W = buf[w.offset - base: w.offset - base + 2 * self.L * H].view(2 * self.L, H)
        B = buf[b.offset - base: b.offset - base + 2 * self.L]
        return W, B


@dataclass
class DeviceData:
    """Interaction CSR resident in HBM + the user ids a loader iterates over."""
    row_ptr: torch.Tensor
    col_idx: torch.Tensor
    vals: torch.Tensor
    users: torch.Tensor       # int32 [n] (rows of the matrix this dataset yields)
    n_items: int
    row_nnz: np.ndarray       # host copy of nnz per listed user (capacity planning)
    perm: torch.Tensor = field(default=None)  # int32 [n] current epoch order
    host_indptr: np.ndarray = field(default=None)   # host CSR (data-parallel exchange sizing)
    host_indices: np.ndarray = field(default=None)
    users_host: np.ndarray = field(default=None)
    dp_global: bool = False   # data parallel: every rank holds every user (hvae/dist.py dp_shard)
    _cap_cache: dict = field(default_factory=dict, repr=False)  # max_batch_nnz per batch size

    @staticmethod
    def from_scipy(mat, users, device) -> "DeviceData":
        mat = mat.tocsr()
        mat.sum_duplicates()
        users = np.asarray(users, dtype=np.int64)
        rp = mat.indptr.astype(np.int64)
        users_d = torch.as_tensor(users.astype(np.int32), device=device)
        return DeviceData(
            row_ptr=torch.as_tensor(rp, device=device),
            col_idx=torch.as_tensor(mat.indices.astype(np.int32), device=device),
            vals=torch.as_tensor(mat.data.astype(np.float32), device=device),
            users=users_d,
            n_items=mat.shape[1],
            row_nnz=(rp[users + 1] - rp[users]) if len(users) else np.zeros(0, np.int64),
            perm=users_d.clone(),  # fixed address: captured graphs read the epoch order from here
            host_indptr=rp, host_indices=mat.indices, users_host=users,
        )

    def max_batch_nnz(self, B: int) -> int:
        """Entries of the largest batch of B users (the sum of the B largest row lengths). Cached per B: the run
        loop asks once per step, and a sort of a million row lengths on the host (~1-4 ms) outlasted the Syn-1M
        step's GPU work, leaving the device idle between graph replays (~105 us a step, r06 kernel trace)."""
        if len(self.row_nnz) == 0:
            return 1
        hit = self._cap_cache.get(B)
        if hit is None:
            k = min(B, len(self.row_nnz))
            top = np.partition(self.row_nnz, len(self.row_nnz) - k)[len(self.row_nnz) - k:]
            hit = self._cap_cache[B] = max(int(top.sum()), 1)
        return hit


def _sampler_order(n: int, generator: torch.Generator | None, device) -> torch.Tensor:
    """The order DataLoader(shuffle=True) draws (torch RandomSampler.__iter__): with no generator, a fresh CPU
    generator seeded from the global RNG; with a CPU generator, randperm from it and a second draw the sampler
    makes when its iterator finishes; a device generator (benchmarks) draws on the device."""
    if generator is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(n, generator=g)
    if generator.device.type != "cpu":
        return torch.randperm(n, generator=generator, device=generator.device)
    order = torch.randperm(n, generator=generator)
    torch.randperm(n, generator=generator)  # RandomSampler's trailing (empty-slice) draw
    return order


@dataclass(frozen=True)
class StepSchedule:
    """Which arrangement of its launches one step gets (step_schedule)."""
    rows: bool            # heads -> reparameterisation -> projection run in hvae_mlp_*_rows
    fused_enc: bool       # ... and the first encoder layer inside that launch
    enc_lazy: bool        # ... which reads W1t through lazy Adam itself: no catch-up launch precedes it
    plan: str | None      # the W1 row-gradient plan: None (not training), "dp", "stream", "in_rows" or "inline"
    catchup: str | None   # the catch-up before the forward: None, "csr", "csr_pending" or "rowgrad"
    wgrad_side: bool      # the weight-gradient GEMMs run on the side stream
    defer: bool           # the step records its W1t update (hvae_adam_lazy_defer) instead of applying it


def step_schedule(*, B: int, train: bool, dp: bool, lazy_adam: bool, adam_defer: bool, enc_lazy_read: bool,
                  rows_ok: bool, one_hidden_512: bool, side_min_batch: int, cap: int) -> StepSchedule:
    """The one place that decides a step's arrangement, from plain values (FusedTrainer._schedule gathers them).

    rows_ok: the row-parallel MLP serves this batch (FusedTrainer._mlp_rows_ok); cap: entries of the batch's row
    gradient; side_min_batch: HVAE_PLAN_SIDE_MIN_BATCH.
    """
    # one hidden layer of H <= 512 with the row-parallel MLP: the encoder layer runs in hvae_mlp_fwd_rows, which
    # can read W1t through lazy Adam itself (rows replayed in registers)
    fused_enc = rows_ok and one_hidden_512
    enc_lazy = train and not dp and lazy_adam and enc_lazy_read and fused_enc
    # From side_min_batch up the plan runs on its own stream beside the catch-up, the encoder and the forward
    # GEMMs (it needs only the batch; forking it before the catch-up: Syn-1M 1.197 -> 1.189 ms per step, Syn-10M
    # +-0.1 %, profiles/r06_step_ab.jsonl) and the weight-gradient GEMMs run on the side stream beside the
    # data-gradient chain (Syn-1M 1.082 -> 1.061 ms per step, Syn-10M bf16 / fp8 -0.1 / -0.3 %,
    # profiles/r06_wgrad_side_ab.jsonl). Below it the plan is short and the CSR catch-up's dependent loads cost more
    # than the overlap saves (All_Beauty B = 64: 0.1815 ms/step with the plan in line, 0.1965 beside; Syn-1M
    # B = 4096: 1.545 -> 1.293 ms/step beside), and every cross-stream edge of the captured graph costs 5-10 us,
    # more than the short kernels it would overlap.
    big = B >= side_min_batch
    # A deferred update pays where few of a step's rows recur in the next batch (FusedTrainer.__init__); it needs
    # the CSR catch-up in front of the forward, so not the steps whose fused encoder reads W1t through lazy Adam.
    defer = train and adam_defer and lazy_adam and (dp or (big and not (enc_lazy_read and fused_enc)))
    plan = catchup = None
    if train:
        # "dp": the union batch's plan, on the plan stream; "in_rows": the plan fits one block, which rides in
        # hvae_mlp_fwd_rows' launch; "inline": on the main stream in front of the forward
        one_block = rows_ok and cap <= _lib.PLAN_SMALL_CAP and B <= _lib.PLAN_SMALL_CAP
        plan = "dp" if dp else "stream" if big else "in_rows" if one_block else "inline"
        if lazy_adam and not enc_lazy:
            # the batch's rows from the plan in line before it, else from the CSR entries (no wait for the plan)
            catchup = "rowgrad" if plan == "inline" else "csr_pending" if defer else "csr"
    return StepSchedule(rows=rows_ok, fused_enc=fused_enc, enc_lazy=enc_lazy, plan=plan, catchup=catchup,
                        wgrad_side=train and big, defer=defer)


class _StepBuffers:
    """Activations / gradients for one batch size (graph-static pointers).

    cap: entries of the batch's first-layer row gradient (single GPU); with data parallelism the union
    batch's (world x the per-rank packet cap), which the clip workspace must cover."""

    def __init__(self, ex: "FusedTrainer", B: int, cap: int, train: bool):
        dev, lay = ex.device, ex.layout
        f = lambda *s: torch.empty(*s, device=dev)
        self.B = B
        H = lay.hidden
        L, d = lay.L, lay.d
        self.h = [f(B, hd) for hd in H]
        self.xhat = [f(B, hd) for hd in H]
        self.rstd = [f(B) for _ in H]
        self.a = [None] + [f(B, hd) for hd in H[1:]]
        self.heads = f(B, 2 * L)
        self.z = f(B, L)
        self.eps = f(B, L)
        self.kl_rows = f(B)
        self.p1 = f(B, d) if lay.has_proj else None
        self.q = f(B, d) if lay.has_proj else None
        self.u = f(B, d) if lay.has_proj else self.z
        self.lse = f(B)
        self.recon_rows = f(B)
        self.dU = f(B, d)
        self.dp1 = f(B, d) if lay.has_proj else None
        self.dz = f(B, L) if lay.has_proj else self.dU
        self.dheads = f(B, 2 * L)
        self.dh = [f(B, hd) for hd in H]
        self.da = [f(B, hd) for hd in H]
        self.loss3 = f(3)
        # the local row gradient (single GPU); data parallel steps build the union's in the exchange
        # (with trainable E the plan also gathers rows of u, width d)
        self.rg = (ops.RowGradBuffers(lay.n_items, H[0], cap, dev, width=d if ex.train_e else None)
                   if (train and ex.dp is None) else None)
        self.cap = cap
        # trainable E: dE's dense term in item chunks of e_chunk columns (S = u E_c^T, at most 64 M floats)
        self.e_chunk = 0
        if train and ex.train_e:
            self.e_chunk = int(min(lay.n_items, max(64, (1 << 26) // max(B, 1) // 64 * 64)))
            self.S = f(B, self.e_chunk)
            self.nrow = f(B)
        L_ = lib()
        need = [
            L_.hvae_decoder_workspace(ex.dec_dtype, B, lay.n_items, d),
            L_.hvae_clip_grad_norm_workspace(lay.n_small, cap, H[0]),
        ]
        dims = [(B, hd) for hd in H] + [(B, 2 * L), (B, d), (B, L)]
        for (_, n) in dims:
            need.append(L_.hvae_colsum_workspace(B, n))
        for hd in H:
            need.append(L_.hvae_ln_gelu_drop_bwd_workspace(B, hd))
        if B <= _lib.MLP_ROWS_MAX_NB:  # the row-parallel MLP backward's LayerNorm column sums
            need.append(L_.hvae_mlp_bwd_rows_workspace(B, H[-1]))
        # (m, n, k) of every split-K-capable GEMM of the step: forward, data- and weight-gradient products
        gemms = [(B, 2 * L, H[-1]), (2 * L, H[-1], B), (B, H[-1], 2 * L)]
        if lay.has_proj:
            gemms += [(B, d, L), (B, d, d), (d, d, B), (d, L, B), (B, d, d), (B, L, d)]
        for k in range(1, len(H)):
            gemms += [(B, H[k], H[k - 1]), (H[k], H[k - 1], B), (B, H[k - 1], H[k])]
        if self.e_chunk:
            gemms += [(B, self.e_chunk, d), (self.e_chunk, d, B)]
        for (m_, n_, k_) in gemms:
            need.append(L_.hvae_gemm_f32_workspace(m_, n_, k_))
        self.ws = torch.empty(max(int(max(need)), 256), dtype=torch.uint8, device=dev)
        # side-stream GEMMs: their split-K slabs must not alias the main stream's (as large as ws: hvae_gemm_f32
        # clamps its split-K count by the workspace it is given, and with it the order of its sums)
        self.ws2 = torch.empty_like(self.ws) if ex._schedule(B, train, cap).wgrad_side else None
        self.graph = None
        self.graph_k, self.graph_k_steps = None, 0  # single GPU: K consecutive steps in one graph (host-bound steps)
        self.graph_pre = self.graph_up = None  # data parallel: the CSR-packet and update graphs of a step
        self.graph_data = None  # the DeviceData a captured graph reads (held, compared by identity)


class _Step:
    """What the stages of one FusedTrainer._launch_fwd_bwd call share: the batch, its schedule, streams, workspaces."""

    def __init__(self, ex: "FusedTrainer", bf: _StepBuffers, csr: CsrBatch, train: bool, beta: float, p_drop: float,
                 ext: dict | None):
        self.bf, self.csr, self.csr_ref = bf, csr, C.byref(csr)
        self.train, self.tr, self.beta, self.p_drop = train, int(train), beta, p_drop
        self.sched = sc = ex._schedule(bf.B, train, bf.cap)
        if sc.wgrad_side and bf.ws2 is None:
            raise RuntimeError("fused trainer: this buffer set was built for a schedule without the side stream")
        self.main = torch.cuda.current_stream(ex.device)
        self.side = ex.side if sc.wgrad_side else self.main
        self.st, self.st2 = self.main.cuda_stream, self.side.cuda_stream
        self.ws, self.wsn = ptr(bf.ws), bf.ws.numel()
        self.ws2 = ptr(bf.ws2) if sc.wgrad_side else self.ws
        self.ext = ext or {}
        self.encm = self.ext.get("enc_masks", [None] * len(bf.h))
        self.beta_dev = self.ks_dev = None  # (beta, beta / B) on the device in an annealed epoch (the prologue)
        self.rows = None      # the row-parallel MLP's arguments (the forward sets them, the backward adds its own)


def _epi_bias(b: torch.Tensor) -> Epilogue:
    return Epilogue(kind=_lib.EPI_BIAS, bias=ptr(b))


def _epi_rowsum(out: torch.Tensor) -> Epilogue:
    """A weight-gradient GEMM's bias gradient = sum_k op(A)[m, k], fused into it."""
    return Epilogue(kind=_lib.EPI_NONE, opa_rowsum=ptr(out))


class FusedTrainer:
    """Owns the flat parameter/optimizer state of one HybridVAE on one device."""

    def __init__(self, model, device, lr: float = 1e-3, weight_decay: float = 0.0, betas=(0.9, 0.999),
                 eps: float = 1e-8, max_norm: float = 5.0, precision: str | None = None, seed: int | None = None,
                 use_graphs: bool = True, process_group=None):
        if device.type != "cuda":
            raise RuntimeError("FusedTrainer runs the MI355X HIP path only (device must be the HIP device)")
        lib()  # fail loudly now if libhvae.so is missing
        self.model = model
        self.device = device
        self.layout = lay = FlatLayout(model)
        self.lr, self.wd, self.betas, self.eps, self.max_norm = lr, weight_decay, betas, eps, max_norm
        self.use_graphs = use_graphs
        # trainable item embeddings: E lives in the flat dense segment; each step refreshes the decoder's image of
        # it, adds its gradient (hvae_embed.hip) and Adam moves it with the other dense parameters
        self.train_e = lay.train_e
        if self.train_e and process_group is not None and torch.distributed.get_world_size(process_group) > 1:
            raise NotImplementedError("fused trainer: data parallelism covers frozen item embeddings only (a "
                                      "trainable E would need its dense [N, d] gradient all-reduced every step)")
        self.seed = int(seed if seed is not None else torch.randint(0, 2 ** 62, (1,)).item())
        # ---- flat state
        self.flat = torch.zeros(lay.total, device=device)
        self.m = torch.zeros(lay.total, device=device)
        self.v = torch.zeros(lay.total, device=device)
        self.g_small = torch.zeros(lay.n_small, device=device)
        self._adopt_parameters()
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.step_snap = torch.zeros(1, dtype=torch.int64, device=device)  # step before this update (Adam's t - 1)
        # Exact lazy Adam for W1t (hvae_adam_lazy): rows outside a batch replay their g = 0 steps when next
        # read -- bitwise equal to torch's every-row update, without streaming all N*H each step.
        self.lazy_adam = not bool(int(os.environ.get("HVAE_DENSE_ADAM", "0")))
        self.last_step = torch.zeros(lay.n_items, dtype=torch.int32, device=device)
        self.tab_len = 1 << 22
        self.adam_tab = torch.zeros(2 * self.tab_len, dtype=torch.float32, device=device)
        # Deferred W1t update (hvae_adam_lazy_defer, HVAE_ADAM_DEFER=1): a step's update records its gradient rows
        # as pending instead of moving them; the next step's catch-up applies it to its batch's rows before the
        # forward reads them, and hvae_adam_lazy_pending moves the rest (and the step's sweep range) on the defer
        # stream beside the next step, joined before that step's row-gradient apply. Bitwise the same parameters.
        # HVAE_DEFER_AT: "sweep" (after the decoder sweep, beside the finalize and the backward) or "fwd" (forked
        # after the catch-up, beside the forward). It pays where few of a step's rows recur in the next batch: the
        # Syn-10M shard (N = 1 M, ~20 % recur) bf16 / fp8 -0.2..-0.4 % / -0.5..-1.2 % per step with "sweep" in 3 A/B
        # pairs each, "fwd" +-0.2 %; at Syn-1M (N = 100 K, ~48 % recur) the catch-up takes on half the rows' updates
        # and the rest slows the encoder beside it: 1.051 -> 1.081 ("sweep") / 1.096 ("fwd") ms; at the W = 8 union
        # (emulated, scripts/bench_dp_emul.py) the update graph's 0.96 ms moves into the next step's whole
        # (12.32 -> 12.30 bf16, 7.32 -> 7.29 fp8 ms): profiles/r06_defer_ab.jsonl. So HVAE_ADAM_DEFER defaults to
        # on from 2^19 items (HVAE_ADAM_DEFER=0 / 1 forces it)
        env_defer = os.environ.get("HVAE_ADAM_DEFER")
        self.adam_defer = self.lazy_adam and (bool(int(env_defer)) if env_defer is not None
                                              else lay.n_items >= (1 << 19))
        self.defer_at = os.environ.get("HVAE_DEFER_AT", "sweep")
        # HVAE_DEFER_AT=guest: under the decoder sweep, as a guest kernel written to fit beside its waves
        # (hvae_adam_lazy_pending_guest), forked after the last forward launch; only where the loaded code objects
        # say it fits beside the sweep of that batch size (hvae_adam_pending_guest_fits), else "sweep". With
        # HVAE_DEFER_AT unset it is the default where it fits and was measured: single-GPU steps (GUEST_DEFAULT;
        # data-parallel steps take it only when asked); everywhere else the step is unchanged launch for launch.
        self._guest_asked = self.defer_at == "guest"
        self._guest_on = self.adam_defer and (self._guest_asked or
                                              (GUEST_DEFAULT and "HVAE_DEFER_AT" not in os.environ))
        if self.defer_at == "guest":
            self.defer_at = "sweep"  # where the guest does not fit
        self._guest_fits: dict[int, bool] = {}
        self._pend_open = False  # (host-tracked) a recorded update may still be pending on the device
        if self._guest_on:
            # the guest's stream has the lowest priority torch offers (the numerically largest of its range)
            self.guest_stream = torch.cuda.Stream(device, priority=max(torch.cuda.Stream.priority_range()))
        if self.adam_defer:
            self.pend_slot = torch.zeros(lay.n_items, dtype=torch.int32, device=device)
            self.pend_item = torch.zeros(lay.n_items, dtype=torch.int32, device=device)
            self.pend_hdr = torch.zeros(4, dtype=torch.int64, device=device)  # PendHdr (t = 0: nothing recorded)
            self._pend = _lib.AdamPend(ptr(self.pend_slot), ptr(self.pend_item), ptr(self.pend_hdr))
            self.defer_stream = torch.cuda.Stream(device)
        # the side stream takes the weight-gradient GEMMs of the backward, the plan stream the W1 row-gradient plan,
        # for batches from plan_side_min_batch up (HVAE_PLAN_SIDE_MIN_BATCH; step_schedule has the measurements)
        self.side = torch.cuda.Stream(device)
        self.plan_stream = torch.cuda.Stream(device)
        self.plan_side_min_batch = int(os.environ.get("HVAE_PLAN_SIDE_MIN_BATCH", "512"))
        # batches up to MLP_ROWS_MAX_NB run the latent / projection MLP row-parallel (hvae_mlp_*_rows)
        self.mlp_rows = bool(int(os.environ.get("HVAE_MLP_ROWS", "1")))
        self._mlp_rows_cache: dict[int, bool] = {}
        # small batches: the fused encoder layer reads W1t through lazy Adam (HVAE_ENC_LAZY_READ=0: a catch-up launch)
        self.enc_lazy_read = bool(int(os.environ.get("HVAE_ENC_LAZY_READ", "1")))
        self.ones = torch.ones(1024, dtype=torch.float32, device=device)
        self.boff = torch.zeros(1, dtype=torch.int64, device=device)
        self.norm = torch.zeros(1, device=device)
        self.coef = torch.ones(1, device=device)
        self.accum_train = torch.zeros(3, dtype=torch.float64, device=device)
        # annealed beta (AnnealedVAE): the schedule's step counter and (beta, beta / B) of the current step, both
        # on the device, so an annealed epoch replays one captured step (hvae_anneal_beta)
        self.anneal_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.beta_dev = torch.zeros(2, device=device)
        self._anneal = None  # (beta_min, beta_max, anneal_steps) while an annealed train epoch runs
        self.accum_val = torch.zeros(3, dtype=torch.float64, device=device)
        self.host_step = 0
        # ---- frozen embeddings: fp32 (sparse terms, eval) + bf16 copy (decoder MFMA)
        self.E32 = model.item_embeddings.detach().contiguous()
        if self.E32.device != device:
            raise RuntimeError("model must be moved to the device before building the trainer")
        d = lay.d
        if precision is None:
            precision = "bf16" if ops.decoder_supported(_lib.HVAE_BF16, d) else "fp32"

        def refuse(name: str, dtype: int):
            # the widths this precision's sweep is built for, as the library reports them
            widths = [w for w in range(1, 1025) if ops.decoder_supported(dtype, w)]
            return NotImplementedError(f"no {name} streaming decoder for embedding dim {d} "
                                       f"(supported widths: {', '.join(map(str, widths))})")

        if precision == "bf16":
            if not ops.decoder_supported(_lib.HVAE_BF16, d):
                raise refuse("bf16", _lib.HVAE_BF16)
            self.dec_dtype = _lib.HVAE_BF16
            self.E_dec = ops.decoder_image(self.E32)  # bf16 E + its tile-transposed copy
        elif precision == "fp8":
            if not ops.decoder_supported(_lib.HVAE_FP8, d):
                raise refuse("fp8", _lib.HVAE_FP8)
            self.dec_dtype = _lib.HVAE_FP8
            self.E_dec = ops.decoder_image(self.E32, _lib.HVAE_FP8)  # bf16 E + e4m3 fragment tiles
        elif precision == "fp32":
            if not ops.decoder_supported(_lib.HVAE_F32, d):
                raise refuse("fp32", _lib.HVAE_F32)
            self.dec_dtype = _lib.HVAE_F32
            self.E_dec = self.E32
        else:
            raise ValueError(f"precision must be 'bf16', 'fp8' or 'fp32', got {precision!r}")
        self.precision = precision
        self.enorm = ops.row_norm_max(self.E_dec)
        self._e_version = model.item_embeddings._version
        self._e_src_ptr = model.item_embeddings.data_ptr()
        self._bufs: dict[tuple, _StepBuffers] = {}
        self._views()
        self.dp = None
        self.dp_epoch = 0
        self.dp_val_epoch = 0
        self._dp_caps: dict = {}
        if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
            from .dist import DPExchange
            self.dp = DPExchange(process_group, device, lay.n_items, lay.hidden[0], lay.n_small)
            # replicas start from rank 0's parameters (identical seeds make this a no-op, but be explicit)
            on_dev = torch.distributed.get_backend(process_group) == "nccl"
            flat = self.flat if on_dev else self.flat.cpu()
            torch.distributed.broadcast(flat, 0, group=process_group)
            if flat is not self.flat:
                self.flat.copy_(flat)
            seed_t = torch.tensor([self.seed], dtype=torch.int64, device=device if on_dev else "cpu")
            torch.distributed.broadcast(seed_t, 0, group=process_group)
            # the epoch order is drawn from rank 0's seed on every rank (dp_shard); per-rank dropout streams must
            # differ (each rank sees different users)
            self.dp_seed = int(seed_t.item())
            self.seed = self.dp_seed + 7919 * torch.distributed.get_rank(process_group)

    # ------------------------------------------------------------ state ---
    def _adopt_parameters(self):
        """Copy the module's parameters into the flat buffer and rebind them as views."""
        lay, model = self.layout, self.model
        named = dict(model.named_parameters())
        with torch.no_grad():
            w1 = named["encoder.0.weight"]  # [H, N] (a view of item-major storage)
            w1t = lay.view(self.flat, "w1t")
            w1t.copy_(w1.detach().t())
            w1.data = w1t.t()
            for name, seg in lay.segs.items():
                if name == "w1t":
                    continue
                p = named[name]
                v = lay.view(self.flat, name)
                v.copy_(p.detach().reshape(seg.shape))
                p.data = v
        self.param_views = {n: p for n, p in named.items()}

    def _views(self):
        lay, f = self.layout, self.flat
        base = lay.small_offset
        V = lambda buf, n, b=0: lay.view(buf, n, b)
        self.w1t = V(f, "w1t")
        self.m_w1t, self.v_w1t = V(self.m, "w1t"), V(self.v, "w1t")
        self.small = f[base:]
        self.m_small, self.v_small = self.m[base:], self.v[base:]
        H = lay.hidden
        self.P = {}
        self.G = {}
        for k in range(len(H)):
            i = 4 * k
            names = [f"encoder.{i}.bias", f"encoder.{i + 1}.weight", f"encoder.{i + 1}.bias"]
            if k > 0:
                names.append(f"encoder.{i}.weight")
            for n in names:
                self.P[n] = V(f, n)
                self.G[n] = V(self.g_small, n, base)
        if lay.train_e:
            self.P["item_embeddings"] = V(f, "item_embeddings")
            self.G["item_embeddings"] = V(self.g_small, "item_embeddings", base)
        self.W_heads, self.b_heads = lay.heads(f)
        self.gW_heads, self.gb_heads = lay.heads(self.g_small, base)
        if lay.has_proj:
            for n in ("projection_layer.0.weight", "projection_layer.0.bias", "projection_layer.3.weight",
                      "projection_layer.3.bias"):
                self.P[n] = V(f, n)
                self.G[n] = V(self.g_small, n, base)

    def sync_embeddings(self):
        """E is frozen, but load_state_dict / copy_ may still write new values into the module's buffer (a
        checkpoint of another embedding file): bring the fp32 copy, the decoder image and max||E|| up to date in
        place, so captured graphs keep their pointers. Cheap when nothing changed (a version compare)."""
        E = self.model.item_embeddings
        # the source tensor last synced from (its address and version), not E32's address: E32 is a private copy
        # whenever the module's buffer is non-contiguous or has been reassigned
        if E._version == self._e_version and E.data_ptr() == self._e_src_ptr:
            return
        with torch.no_grad():
            if E.data_ptr() != self.E32.data_ptr():
                self.E32.copy_(E.detach())
            if isinstance(self.E_dec, ops.DecoderImage):
                self.E_dec.refresh(self.E32)
            ops.row_norm_max(self.E_dec, out=self.enorm)
        self._e_version = E._version
        self._e_src_ptr = E.data_ptr()

    def grad_of(self, name: str) -> torch.Tensor:
        """Current gradient of a small parameter (after the last step)."""
        return self.G[name]

    # ------------------------------------------------------------- data ---
    def device_data(self, mat, users) -> DeviceData:
        return DeviceData.from_scipy(mat, users, self.device)

    # ------------------------------------------------------------- step ---
    def _buffers(self, B: int, cap: int, train: bool) -> _StepBuffers:
        key = (B, train)
        b = self._bufs.get(key)
        if b is None or (train and b.cap < cap):
            if b is not None:
                self._resolve_pending()  # a recorded update may still read the gradient rows of the set it replaces
            b = _StepBuffers(self, B, cap, train)
            self._bufs[key] = b
        return b

    def _csr(self, data: DeviceData, B: int, rows: torch.Tensor | None, offset: torch.Tensor | None) -> CsrBatch:
        return CsrBatch(ptr(data.row_ptr), ptr(data.col_idx), ptr(data.vals), ptr(rows), ptr(offset), B,
                        data.n_items)

    def _launch(self, bf: _StepBuffers, csr: CsrBatch, train: bool, beta: float, p_drop: float,
                ext: dict | None = None, advance: int = 0, weight: float = 1.0):
        """Enqueue one full step on the current stream (captured into a graph by the caller).

        advance > 0 also moves the device batch offset (rows_offset) by that many users. Data parallel:
        the batch CSR is exchanged before the forward (the union batch's row-gradient plan then runs beside
        it), the small gradients and da between the backward and the update; weight = this rank's share of the
        union batch.
        """
        if train and self.dp is not None:
            self._launch_pack_csr(bf, csr, weight)
            self.dp.communicate_csr()
            self._launch_fwd_bwd(bf, csr, train, beta, p_drop, ext)
            self._launch_pack_grads(bf, weight)
            self.dp.communicate_grads()
            self._launch_dp_update(bf, advance)
            return
        if train and not self._defers(bf.B) and not torch.cuda.is_current_stream_capturing():
            self._resolve_pending()  # this step's forward reads rows without the deferred update's catch-up
        self._launch_fwd_bwd(bf, csr, train, beta, p_drop, ext)
        if train:
            self._launch_update(bf.rg, bf, advance)
        elif advance:
            self._advance(advance)

    def _launch_pack_csr(self, bf: _StepBuffers | None, csr: CsrBatch | None, weight: float):
        """Start of a data-parallel step: this rank's batch as compact CSR (values * weight) into its packet.
        bf None: no users in this step."""
        if bf is None:
            self.dp.pack_csr(None, 0, 0.0)
            return
        self.dp.pack_csr(C.byref(csr), bf.B, weight)

    def _launch_pack_grads(self, bf: _StepBuffers | None, weight: float):
        """End of a data-parallel forward/backward: the weighted small gradients and the first-layer
        pre-activation gradient da."""
        if bf is None:
            self.dp.pack_grads(self.g_small.zero_(), 0, None, 0.0)
            return
        self.dp.pack_grads(self.g_small, bf.B, bf.da[0], weight)

    def _launch_dp_update(self, bf: _StepBuffers, advance: int):
        merged = self.dp.merge_apply(self.g_small)
        self._launch_update(merged, bf, advance)

    def _fork(self, src, dst):
        """dst waits for everything enqueued on src so far (a graph edge under capture)."""
        if src is not dst:
            dst.wait_event(self._record(src))

    def _record(self, stream) -> torch.cuda.Event:
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    def _schedule(self, B: int, train: bool, cap: int) -> StepSchedule:
        """step_schedule of one step of B users, evaluated per launch: mlp_rows and lazy_adam may be set later."""
        return step_schedule(B=B, train=train, dp=self.dp is not None, lazy_adam=self.lazy_adam,
                             adam_defer=self.adam_defer, enc_lazy_read=self.enc_lazy_read,
                             rows_ok=self._mlp_rows_ok(B), one_hidden_512=self.layout.one_hidden_512,
                             side_min_batch=self.plan_side_min_batch, cap=cap)

    def _defers(self, B: int) -> bool:
        """Whether a train step of B users records its W1t update (hvae_adam_lazy_defer) instead of applying it."""
        return self._schedule(B, True, 0).defer  # (defer does not depend on cap)

    def _launch_fwd_bwd(self, bf: _StepBuffers, csr: CsrBatch, train: bool, beta: float, p_drop: float,
                        ext: dict | None = None):
        """Forward + loss (+ backward when train) of one batch, in the arrangement _schedule gives it. The main
        stream runs the dependent chain (forward, decoder, data-gradient GEMMs, LayerNorm backward, W1 row gather).
        What only feeds the optimizer may run beside it -- the W1 row-gradient plan (needs the batch only) on the
        plan stream, the weight-gradient GEMMs on the side stream, a recorded W1t update on the defer stream -- and
        is joined back before the update."""
        s = _Step(self, bf, csr, train, beta, p_drop, ext)
        ev_plan, ev_defer = self._step_prologue(s)
        self._step_forward(s)
        if train and s.sched.defer and ev_defer is None and self._use_guest(bf.B):
            # HVAE_DEFER_AT=guest: forked after the last forward launch, under the decoder sweep. The hazards are
            # those of "fwd", which forks even earlier: the batch's rows were claimed by the catch-up before the
            # fork, and the encoder (done by now) reads only those rows; the sweep reads no W1t row at all.
            ev_defer = self._launch_pending(s, guest=True)
        self._step_decoder(s)
        if not train:
            return
        if s.sched.defer and ev_defer is None:  # HVAE_DEFER_AT=sweep: beside the finalize and the backward
            ev_defer = self._launch_pending(s)
        self._step_backward(s)
        self._step_finish(s, ev_plan, ev_defer)

    def _launch_pending(self, s: "_Step", guest: bool = False) -> torch.cuda.Event:
        """The last step's recorded W1t update, for the rows this batch's catch-up did not take, on the defer
        stream (guest: on the guest's stream, by the guest kernel) from here on. Returns the event the row-gradient
        apply waits for."""
        ds = self.guest_stream if guest else self.defer_stream
        self._fork(s.main, ds)
        if guest:  # the sweep's blocks resident first
            check(lib().hvae_adam_guest_hold(GUEST_HOLD_US, ds.cuda_stream), "adam_guest_hold")
        # (the cap of this step's buffers is a grid-size hint: the record is the previous step's, whose batch may
        # have been larger -- a full batch before the epoch's tail -- and both kernels walk all of its rows)
        self._apply_pending(min(self.layout.n_items, s.bf.cap), ds.cuda_stream, guest)
        return self._record(ds)

    def _use_guest(self, B: int) -> bool:
        """Whether a deferring train step of B users runs its recorded update under the decoder sweep
        (HVAE_DEFER_AT=guest, or by default where GUEST_DEFAULT): only where the guest fits beside that sweep, and
        by default only on a single GPU, where it was measured."""
        if not self._guest_on or (self.dp is not None and not self._guest_asked):
            return False
        if B not in self._guest_fits:
            lay = self.layout
            self._guest_fits[B] = bool(lib().hvae_adam_pending_guest_fits(self.dec_dtype, B, lay.n_items, lay.d))
        return self._guest_fits[B]

    def _step_prologue(self, s: "_Step"):
        """What precedes the forward: the decoder's image of a trainable E, the annealed beta, and the placement of
        the row-gradient plan, the lazy-Adam catch-up and a recorded update. Returns the events (plan, recorded
        update) that _step_finish joins."""
        L_, bf, sc = lib(), s.bf, s.sched
        if self.train_e:
            # E moved with the last step's Adam: the decoder's image of it and max||E|| follow (in the captured step)
            if isinstance(self.E_dec, ops.DecoderImage):
                self.E_dec.refresh(self.E32)
            ops.row_norm_max(self.E_dec, out=self.enorm)
        if not s.train:
            return None, None
        if self._anneal is not None:  # this step's (beta, beta / B) from the device schedule counter, which it advances
            s.beta_dev, s.ks_dev, (b0, b1, n) = self.beta_dev, self.beta_dev[1:], self._anneal
            check(L_.hvae_anneal_beta(ptr(self.anneal_dev), b0, b1, n, bf.B, ptr(s.beta_dev), s.st), "anneal_beta")
        ps, ev_defer = self.plan_stream, None
        if sc.plan in ("stream", "inline"):
            if sc.plan == "stream":
                # forked before the catch-up, which it then overlaps too: it reads only the batch, and the previous
                # step's update that read the plan's buffers is behind it on the main stream
                self._fork(s.main, ps)
            check(L_.hvae_w1_rowgrad_plan(s.csr_ref, bf.rg.ref, ptr(bf.rg.ws), bf.rg.ws.numel(),
                                          ps.cuda_stream if sc.plan == "stream" else s.st), "w1_rowgrad_plan")
        # the batch's W1t rows replay their deferred steps before the forward reads them
        if sc.catchup == "rowgrad":
            self._catchup_rows(bf.rg.ref, s.st)
        elif sc.catchup is not None:
            self._catchup_csr(s.csr_ref, s.st, pending=sc.catchup == "csr_pending")
        if sc.defer and self.defer_at == "fwd":  # beside the forward
            ev_defer = self._launch_pending(s)
        if sc.plan == "dp":
            # no local row gradient: the union batch's plan, from the CSR packets gathered before this forward,
            # runs beside it; its apply follows the second exchange
            self._fork(s.main, ps)
            with torch.cuda.stream(ps):
                self.dp.merge_plan()
        return (self._record(ps) if sc.plan in ("dp", "stream") else None), ev_defer

    def _gemm(self, s: "_Step", ta, tb, M, N, K, A, lda, Bm, ldb, Cm, ldc, epi=None, side=False):
        check(lib().hvae_gemm_f32(ta, tb, M, N, K, 1.0, A, lda, Bm, ldb, 0.0, Cm, ldc,
                                  C.byref(epi) if epi is not None else None, s.ws2 if side else s.ws, s.wsn,
                                  s.st2 if side else s.st), "gemm")

    def _step_forward(self, s: "_Step"):
        """Encoder, heads, reparameterisation and projection: the batch's u (and the KL rows)."""
        L_, lay, bf, sc, P = lib(), self.layout, s.bf, s.sched, self.P
        B, H, Lt, d = bf.B, lay.hidden, lay.L, lay.d
        seed, step, st, encm = self.seed, ptr(self.step_dev), s.st, s.encm
        rows = s.rows = self._mlp_rows_args(bf, B, s.tr, s.p_drop, s.ext, seed) if sc.rows else None
        if sc.fused_enc:
            # one hidden layer: the encoder layer runs in the row-parallel MLP forward's launch below
            rows.enc_x, rows.w1t, rows.b1 = C.pointer(s.csr), ptr(self.w1t), ptr(P["encoder.0.bias"])
            rows.ln_w, rows.ln_b = ptr(P["encoder.1.weight"]), ptr(P["encoder.1.bias"])
            rows.enc_drop_mult, rows.xhat, rows.rstd = ptr(encm[0]), ptr(bf.xhat[0]), ptr(bf.rstd[0])
            if sc.enc_lazy:
                self._enc_adam = self._adam_cfg(self.step_dev)
                rows.adam = C.addressof(self._enc_adam)
                rows.adam_m, rows.adam_v = ptr(self.m_w1t), ptr(self.v_w1t)
                rows.last_step, rows.adam_tab = ptr(self.last_step), ptr(self.adam_tab)
        else:
            check(L_.hvae_encoder_fwd(s.csr_ref, ptr(self.w1t), ptr(P["encoder.0.bias"]),
                                      ptr(P["encoder.1.weight"]), ptr(P["encoder.1.bias"]), H[0], s.p_drop,
                                      ptr(encm[0]), seed, step, s.tr, ptr(bf.h[0]), ptr(bf.xhat[0]),
                                      ptr(bf.rstd[0]), st), "encoder_fwd")
        for k in range(1, len(H)):
            i = 4 * k
            self._gemm(s, 0, 1, B, H[k], H[k - 1], ptr(bf.h[k - 1]), H[k - 1], ptr(P[f"encoder.{i}.weight"]),
                       H[k - 1], ptr(bf.a[k]), H[k], _epi_bias(P[f"encoder.{i}.bias"]))
            check(L_.hvae_ln_gelu_drop_fwd(ptr(bf.a[k]), ptr(P[f"encoder.{i + 1}.weight"]),
                                           ptr(P[f"encoder.{i + 1}.bias"]), B, H[k], s.p_drop, ptr(encm[k]), seed,
                                           step, k, s.tr, ptr(bf.h[k]), ptr(bf.xhat[k]), ptr(bf.rstd[k]), st),
                  "ln_gelu_drop_fwd")
        if rows is not None:
            if sc.plan == "in_rows":  # the row-gradient plan as one more block of this launch
                rows.plan_x, rows.plan_rg = C.pointer(s.csr), C.pointer(bf.rg.struct)
            # heads -> reparameterisation -> projection, the rows of the batch spread over blocks: one launch
            check(L_.hvae_mlp_fwd_rows(C.byref(rows), st), "mlp_fwd_rows")
            return
        Hl, mu, lv = H[-1], bf.heads, bf.heads[:, Lt:]
        self._gemm(s, 0, 1, B, 2 * Lt, Hl, ptr(bf.h[-1]), Hl, ptr(self.W_heads), Hl, ptr(bf.heads), 2 * Lt,
                   _epi_bias(self.b_heads))
        check(L_.hvae_reparam_kl_fwd(ptr(mu), ptr(lv), 2 * Lt, B, Lt, s.tr, ptr(s.ext.get("eps")), seed, step,
                                     ptr(bf.z), ptr(bf.eps), ptr(bf.kl_rows), st), "reparam_kl_fwd")
        if lay.has_proj:
            epi1 = Epilogue(_lib.EPI_BIAS_GELU_DROP, ptr(P["projection_layer.0.bias"]), ptr(bf.p1), None, s.p_drop,
                            ptr(s.ext.get("proj_mask")), seed, step, _lib.TAG_PROJ_DROP, s.tr, None)
            self._gemm(s, 0, 1, B, d, Lt, ptr(bf.z), Lt, ptr(P["projection_layer.0.weight"]), Lt, ptr(bf.q), d, epi1)
            self._gemm(s, 0, 1, B, d, d, ptr(bf.q), d, ptr(P["projection_layer.3.weight"]), d, ptr(bf.u), d,
                       _epi_bias(P["projection_layer.3.bias"]))

    def _step_decoder(self, s: "_Step"):
        """Decoder sweep + finalize (split merge, sparse loss terms, du) + the batch loss means: one call."""
        bf, d = s.bf, self.layout.d
        accum = self.accum_train if s.train else self.accum_val
        check(lib().hvae_decoder_train(self.dec_dtype, ptr(bf.u), d, ptr(self.E_dec), ptr(self.enorm),
                                       ptr(self.E32), s.csr_ref, d, 1.0 / bf.B, ptr(bf.lse), None,
                                       ptr(bf.recon_rows), ptr(bf.dU) if s.train else None, ptr(bf.kl_rows), s.beta,
                                       ptr(s.beta_dev), ptr(bf.loss3), ptr(accum), s.ws, s.wsn, s.st),
              "decoder_train")

    def _layer_bwd(self, s: "_Step", wgrad: tuple, wrowsum, xgrad: tuple, xepi=None):
        """A layer's weight gradient (trans_a GEMM, the bias gradient = its row sums fused in) and data gradient:
        on the side and the main stream, or with one stream both in one launch (hvae_gemm_f32_pair) -- they read
        only finished inputs."""
        we = _epi_rowsum(wrowsum) if wrowsum is not None else None
        if s.side is not s.main:
            self._fork(s.main, s.side)
            self._gemm(s, 1, 0, *wgrad, epi=we, side=True)
            self._gemm(s, 0, 0, *xgrad, epi=xepi)
            return

        def desc(ta, args, e):
            M, N, K, A, lda, Bm, ldb, Cm, ldc = args
            return GemmDesc(ta, 0, M, N, K, 1.0, A, lda, Bm, ldb, 0.0, Cm, ldc,
                            C.pointer(e) if e is not None else None, s.ws, s.wsn)
        dw, dx = desc(1, wgrad, we), desc(0, xgrad, xepi)
        check(lib().hvae_gemm_f32_pair(C.byref(dw), C.byref(dx), s.st), "gemm_pair")

    def _step_backward(self, s: "_Step"):
        """Every gradient but W1t's rows: dE's dense term, the latent / projection MLP, the encoder layers."""
        L_, lay, bf, P, G = lib(), self.layout, s.bf, self.P, self.G
        B, H = bf.B, lay.hidden
        if self.train_e:
            self._embed_bwd_dense(s)
        if s.rows is not None:
            self._mlp_bwd_rows(s)
        else:
            self._mlp_bwd_gemms(s)
        for k in range(len(H) - 1, -1, -1):
            i = 4 * k
            if not (s.rows is not None and k == len(H) - 1):  # (the row-parallel MLP backward did the last one)
                check(L_.hvae_ln_gelu_drop_bwd(
                    ptr(bf.dh[k]), ptr(bf.xhat[k]), ptr(bf.rstd[k]), ptr(P[f"encoder.{i + 1}.weight"]),
                    ptr(P[f"encoder.{i + 1}.bias"]), B, H[k], s.p_drop, ptr(s.encm[k]), self.seed,
                    ptr(self.step_dev), k, s.tr, ptr(bf.da[k]), ptr(G[f"encoder.{i + 1}.weight"]),
                    ptr(G[f"encoder.{i + 1}.bias"]), ptr(G[f"encoder.{i}.bias"]), s.ws, s.wsn, s.st),
                    "ln_gelu_drop_bwd")
            if k > 0:
                self._layer_bwd(s, (H[k], H[k - 1], B, ptr(bf.da[k]), H[k], ptr(bf.h[k - 1]), H[k - 1],
                                    ptr(G[f"encoder.{i}.weight"]), H[k - 1]), None,
                                (B, H[k - 1], H[k], ptr(bf.da[k]), H[k], ptr(P[f"encoder.{i}.weight"]), H[k - 1],
                                 ptr(bf.dh[k - 1]), H[k - 1]))

    def _embed_bwd_dense(self, s: "_Step"):
        """Trainable E: dE's dense term (1/B) sum_b n_b softmax(u_b E^T)_i u_b in item chunks: S = u E_c^T,
        S <- (n_b / B) exp(S - lse_b), dE_c = S^T u (hvae_embed.hip; the sparse term follows the plan, in
        _step_finish)."""
        L_, bf, d, N_ = lib(), s.bf, self.layout.d, self.layout.n_items
        B, Cc, gE = bf.B, bf.e_chunk, self.G["item_embeddings"]
        check(L_.hvae_csr_row_sums(s.csr_ref, ptr(bf.nrow), s.st), "csr_row_sums")
        for c0 in range(0, N_, Cc):
            cn = min(Cc, N_ - c0)
            self._gemm(s, 0, 1, B, cn, d, ptr(bf.u), d, ptr(self.E32) + 4 * c0 * d, d, ptr(bf.S), Cc)
            check(L_.hvae_softmax_weights(ptr(bf.S), Cc, B, cn, ptr(bf.lse), ptr(bf.nrow), 1.0 / B, s.st),
                  "softmax_weights")
            self._gemm(s, 1, 0, cn, d, B, ptr(bf.S), Cc, ptr(bf.u), d, ptr(gE) + 4 * c0 * d, d)

    def _mlp_bwd_rows(self, s: "_Step"):
        """The row-parallel MLP's backward: the data gradients dp1 -> dheads -> dh of every row, with the last
        hidden layer's LayerNorm -> GELU -> Dropout backward (dh -> da), in one launch; then the three weight
        gradients (with their bias gradients) and the LayerNorm column sums in one more."""
        L_, lay, bf, P, G, rows = lib(), self.layout, s.bf, self.P, self.G, s.rows
        B, Lt, d, Hl, kl = bf.B, lay.L, lay.d, lay.hidden[-1], len(lay.hidden) - 1
        il = 4 * kl
        rows.dU, rows.dp1, rows.dheads, rows.dh = ptr(bf.dU), ptr(bf.dp1), ptr(bf.dheads), ptr(bf.dh[-1])
        rows.ks, rows.ks_dev = s.beta / B, ptr(s.ks_dev)
        rows.ln_w, rows.ln_b = ptr(P[f"encoder.{il + 1}.weight"]), ptr(P[f"encoder.{il + 1}.bias"])
        rows.xhat, rows.rstd, rows.enc_drop_mult = ptr(bf.xhat[kl]), ptr(bf.rstd[kl]), ptr(s.encm[kl])
        rows.enc_layer, rows.da = kl, ptr(bf.da[kl])
        # the LayerNorm column sums stop at per-block partials in ws; the weight-gradient launch below adds them in
        # block order (partials^T x ones), instead of an in-kernel cross-block hand-off
        rows.d_ln_w = rows.d_ln_b = rows.d_bias = None
        rows.ws, rows.ws_bytes = s.ws, s.wsn
        check(L_.hvae_mlp_bwd_rows(C.byref(rows), s.st), "mlp_bwd_rows")
        keep = []

        def wdesc(M, N, A, lda, Bm, ldb, Cm, ldc, rowsum):
            keep.append(_epi_rowsum(rowsum))
            return GemmDesc(1, 0, M, N, B, 1.0, A, lda, Bm, ldb, 0.0, Cm, ldc, C.pointer(keep[-1]), None, 0)
        dl = [wdesc(d, d, ptr(bf.dU), d, ptr(bf.q), d, ptr(G["projection_layer.3.weight"]), d,
                    G["projection_layer.3.bias"]),
              wdesc(d, Lt, ptr(bf.dp1), d, ptr(bf.z), Lt, ptr(G["projection_layer.0.weight"]), Lt,
                    G["projection_layer.0.bias"]),
              wdesc(2 * Lt, Hl, ptr(bf.dheads), 2 * Lt, ptr(bf.h[-1]), Hl, ptr(self.gW_heads), Hl, self.gb_heads)]
        nblk = int(L_.hvae_mlp_rows_blocks(B))
        for kind, g in enumerate((G[f"encoder.{il + 1}.weight"], G[f"encoder.{il + 1}.bias"], G[f"encoder.{il}.bias"])):
            dl.append(GemmDesc(1, 0, Hl, 1, nblk, 1.0, s.ws + 4 * kind * Hl, 3 * Hl, ptr(self.ones), 1, 0.0, ptr(g),
                               1, None, None, 0))
        descs = (GemmDesc * len(dl))(*dl)
        # (on the plan stream beside the W1 row gather this ran slower: All_Beauty 0.147 vs 0.129 ms per step,
        # profiles/r04_wgrad_beside_ab.jsonl)
        check(L_.hvae_gemm_f32_multi(descs, len(dl), s.st), "gemm_multi")

    def _mlp_bwd_gemms(self, s: "_Step"):
        """The GEMM chain's backward of projection, reparameterisation and heads: dU -> dp1 -> dheads -> dh."""
        lay, bf, P, G = self.layout, s.bf, self.P, self.G
        B, Lt, d, Hl = bf.B, lay.L, lay.d, lay.hidden[-1]
        if lay.has_proj:
            Wa, Wb = P["projection_layer.0.weight"], P["projection_layer.3.weight"]
            epi3 = Epilogue(_lib.EPI_GELU_DROP_BWD, None, None, ptr(bf.p1), s.p_drop, ptr(s.ext.get("proj_mask")),
                            self.seed, ptr(self.step_dev), _lib.TAG_PROJ_DROP, s.tr, None)
            self._layer_bwd(s, (d, d, B, ptr(bf.dU), d, ptr(bf.q), d, ptr(G["projection_layer.3.weight"]), d),
                            G["projection_layer.3.bias"], (B, d, d, ptr(bf.dU), d, ptr(Wb), d, ptr(bf.dp1), d), epi3)
            # dz = dp1 Wa with the reparameterisation + KL backward as its epilogue -> dheads = [dmu | dlogvar]
            epi_r = Epilogue(_lib.EPI_REPARAM_BWD, None, None, ptr(bf.heads), 0.0, None, 0, None, 0, s.tr, None,
                             ptr(bf.eps), s.beta / B, ptr(s.ks_dev))
            self._layer_bwd(s, (d, Lt, B, ptr(bf.dp1), d, ptr(bf.z), Lt, ptr(G["projection_layer.0.weight"]), Lt),
                            G["projection_layer.0.bias"],
                            (B, Lt, d, ptr(bf.dp1), d, ptr(Wa), Lt, ptr(bf.dheads), 2 * Lt), epi_r)
        else:
            mu, lv, dmu, dlv = bf.heads, bf.heads[:, Lt:], bf.dheads, bf.dheads[:, Lt:]
            check(lib().hvae_reparam_kl_bwd(ptr(bf.dz), ptr(mu), ptr(lv), 2 * Lt, ptr(bf.eps), B, Lt, s.beta / B,
                                            ptr(s.ks_dev), s.tr, ptr(dmu), ptr(dlv), 2 * Lt, s.st), "reparam_kl_bwd")
        self._layer_bwd(s, (2 * Lt, Hl, B, ptr(bf.dheads), 2 * Lt, ptr(bf.h[-1]), Hl, ptr(self.gW_heads), Hl),
                        self.gb_heads,
                        (B, Hl, 2 * Lt, ptr(bf.dheads), 2 * Lt, ptr(self.W_heads), Hl, ptr(bf.dh[-1]), Hl))

    def _step_finish(self, s: "_Step", ev_plan, ev_defer):
        """Join what ran beside the main stream and gather W1t's row gradient over the plan."""
        L_, bf, d = lib(), s.bf, self.layout.d
        if ev_plan is not None:
            s.main.wait_event(ev_plan)
        if ev_defer is not None:  # the recorded update's rows are done before this step's apply rewrites its rows
            s.main.wait_event(ev_defer)
        if s.sched.plan != "dp":
            if self.train_e:
                # dE's sparse term -(1/B) sum_b x_bi u_b over the plan's item segments (the apply with u for da),
                # before the W1 rows take the same buffer
                check(L_.hvae_w1_rowgrad_apply(ptr(bf.u), d, bf.rg.ref, s.st), "w1_rowgrad_apply(u)")
                check(L_.hvae_rowgrad_scatter_rows(bf.rg.ref, d, -1.0 / bf.B, ptr(self.G["item_embeddings"]), d,
                                                   s.st), "rowgrad_scatter_rows")
            check(L_.hvae_w1_rowgrad_apply(ptr(bf.da[0]), self.layout.hidden[0], bf.rg.ref, s.st),
                  "w1_rowgrad_apply")
        self._fork(s.side, s.main)  # join: every gradient is complete on the main stream

    def _mlp_rows_ok(self, B: int) -> bool:
        """The row-parallel latent / projection MLP (hvae_mlp_fwd_rows / _bwd_rows) serves this batch:
        a projection layer, B <= MLP_ROWS_MAX_NB, widths that are multiples of 32 up to 1024 whose
        activations fit the kernels' LDS. HVAE_MLP_ROWS=0 keeps the GEMM chain."""
        lay = self.layout
        if not self.mlp_rows or not lay.has_proj or B > _lib.MLP_ROWS_MAX_NB:
            return False
        ok = self._mlp_rows_cache.get(B)
        if ok is None:  # the library's own shape rules (rows per block, LDS of both directions), asked for the
            # configuration the step launches: the fused encoder layer needs its own LDS beside the MLP's
            ok = bool(lib().hvae_mlp_rows_supported(B, lay.hidden[-1], lay.L, lay.d, int(lay.one_hidden_512)))
            self._mlp_rows_cache[B] = ok
        return ok

    def _mlp_rows_args(self, bf: _StepBuffers, B: int, tr: int, p_drop: float, ext: dict, seed: int):
        lay = self.layout
        return _lib.MlpRows(
            nb=B, H=lay.hidden[-1], L=lay.L, D=lay.d,
            W_heads=ptr(self.W_heads), b_heads=ptr(self.b_heads),
            W_a=ptr(self.P["projection_layer.0.weight"]), b_a=ptr(self.P["projection_layer.0.bias"]),
            W_b=ptr(self.P["projection_layer.3.weight"]), b_b=ptr(self.P["projection_layer.3.bias"]),
            train=tr, p_drop=p_drop, drop_mult=ptr(ext.get("proj_mask")), eps_in=ptr(ext.get("eps")), seed=seed,
            step_dev=ptr(self.step_dev), h=ptr(bf.h[-1]), heads=ptr(bf.heads), z=ptr(bf.z), eps=ptr(bf.eps),
            kl_rows=ptr(bf.kl_rows), p1=ptr(bf.p1), q=ptr(bf.q), u=ptr(bf.u))

    def _launch_update(self, rg, bf: _StepBuffers, advance: int = 0):
        """clip_grad_norm_(5.0) + Adam over the flat state: two launches. The clip launch also advances the step
        counter (and the batch offset); Adam reads the pre-increment step from step_snap."""
        L_, lay = lib(), self.layout
        st = torch.cuda.current_stream(self.device).cuda_stream
        H0, ws, wsn = lay.hidden[0], ptr(bf.ws), bf.ws.numel()
        cfg = self._adam_cfg(self.step_snap, self.coef)
        clip = (ptr(self.g_small), lay.n_small, rg.ref, H0, self.max_norm, ptr(self.norm), ptr(self.coef),
                ptr(self.step_dev), ptr(self.step_snap), ptr(self.boff) if advance else None, advance)
        if not self.lazy_adam:
            check(L_.hvae_clip_grad_norm_step(*clip, ws, wsn, st), "clip_grad_norm_step")
            check(L_.hvae_adam_flat(C.byref(cfg), ptr(self.flat), ptr(self.m), ptr(self.v), rg.ref, lay.n_items,
                                    H0, ptr(self.g_small), lay.small_offset, lay.n_small, st), "adam_flat")
            return
        # the clip's last block also writes the step's Adam scalars into the step table
        check(L_.hvae_clip_grad_norm_step_adam(*clip, C.byref(cfg), ptr(self.adam_tab), ws, wsn, st),
              "clip_grad_norm_step_adam")
        # W1t (row-sparse gradient, offset 0 of the flat buffer) and the dense segment in one launch
        lazy = (C.byref(cfg), ptr(self.adam_tab), self.tab_len, ptr(self.flat), ptr(self.m), ptr(self.v),
                ptr(self.last_step), rg.ref, H0, ptr(self.g_small), lay.small_offset, lay.n_small)
        if self._defers(bf.B):  # W1t's rows recorded, moved by the next step (or a flush)
            check(L_.hvae_adam_lazy_defer(*lazy, C.byref(self._pend), st), "adam_lazy_defer")
            self._pend_open = True
        else:
            check(L_.hvae_adam_lazy(*lazy, st), "adam_lazy")

    def _adam_cfg(self, step: torch.Tensor, coef: torch.Tensor | None = None) -> _lib.Adam:
        """The optimizer's constants with the device step counter (and clip coefficient) a launch reads."""
        return ops.adam_config(self.lr, self.betas, self.eps, self.wd, step, coef)

    def _lazy_w1(self) -> tuple:
        """The leading arguments of the lazy-Adam catch-up calls: the constants at the current step, the step
        table, and W1t's parameters, moments and per-row step stamps."""
        return (C.byref(self._adam_cfg(self.step_dev)), ptr(self.adam_tab), ptr(self.flat), ptr(self.m),
                ptr(self.v), ptr(self.last_step))

    def _catchup_csr(self, csr_ref, st, pending: bool):
        """The batch's W1t rows, found from its CSR entries, replay the steps they sat out; pending: after taking
        the last step's recorded update (hvae_adam_lazy_defer), which hvae_adam_lazy_pending moves for the rest."""
        H0 = self.layout.hidden[0]
        if pending:
            check(lib().hvae_adam_lazy_catchup_csr_pending(*self._lazy_w1(), csr_ref, H0, C.byref(self._pend), st),
                  "adam_lazy_catchup_csr_pending")
        else:
            check(lib().hvae_adam_lazy_catchup_csr(*self._lazy_w1(), csr_ref, H0, st), "adam_lazy_catchup_csr")

    def _catchup_rows(self, rg_ref, st):
        """The same for the rows of a finished row-gradient plan (rg_ref None: every row)."""
        check(lib().hvae_adam_lazy_catchup(*self._lazy_w1(), rg_ref, self.layout.n_items, self.layout.hidden[0],
                                           st), "adam_lazy_catchup")

    def _apply_pending(self, sweep_rows: int, st, guest: bool = False):
        fn = lib().hvae_adam_lazy_pending_guest if guest else lib().hvae_adam_lazy_pending
        check(fn(*self._lazy_w1(), self.layout.n_items, self.layout.hidden[0], sweep_rows, C.byref(self._pend), st),
              "adam_lazy_pending_guest" if guest else "adam_lazy_pending")

    def flush(self):
        """Bring every W1t row (and its m, v) up to the completed step count (lazy Adam). Called at the end of every
        epoch and eager step, so that whatever reads the parameters or the optimizer state next sees torch's values."""
        if not self.lazy_adam:
            return
        self._resolve_pending()
        self._catchup_rows(None, torch.cuda.current_stream(self.device).cuda_stream)

    def _resolve_pending(self):
        """Apply a recorded W1t update still pending, on the current stream (eager; a no-op on the device when
        the next step's catch-up and hvae_adam_lazy_pending already did)."""
        if not self._pend_open:
            return
        self._apply_pending(self.layout.n_items, torch.cuda.current_stream(self.device).cuda_stream)
        self._pend_open = False

    def _hyper(self) -> tuple:
        """The optimizer constants a captured step bakes in (part of its graph key)."""
        return (self.lr, self.betas, self.eps, self.wd, self.max_norm)

    def mark_all_current(self):
        """Every row has had every step applied (after an external dense update of W1t)."""
        self._resolve_pending()
        if self.adam_defer:
            # step_dev may have moved (a loaded optimizer state): the resolved record must not look live to a later
            # hvae_adam_lazy_pending that runs before the next hvae_adam_lazy_defer writes a new one
            self.pend_hdr.zero_()
        self.last_step.copy_(self.step_dev.to(torch.int32).expand_as(self.last_step))

    def _check_steps(self, more: int):
        if self.lazy_adam and self.host_step + more + 2 >= self.tab_len:
            raise RuntimeError("lazy Adam step table exhausted; run with HVAE_DENSE_ADAM=1")

    def _advance(self, B: int):
        check(lib().hvae_counter_add(ptr(self.boff), B, torch.cuda.current_stream(self.device).cuda_stream),
              "counter_add")

    # -------------------------------------------------------- public API ---
    def step_batch(self, data: DeviceData, rows: torch.Tensor | None, B: int, beta: float, p_drop: float,
                   train: bool = True, ext: dict | None = None, weight: float | None = None) -> torch.Tensor:
        """One eager step over `rows` (int32 device user ids, or None: rows 0..B-1). Returns loss3.

        Data parallel (train): every rank calls it together with its own rows; weight = this rank's share of
        the union batch (default 1 / world: equal batches)."""
        self.sync_embeddings()
        cap = int(data.row_ptr[-1].item()) if rows is None else data.max_batch_nnz(B)
        dp = self.dp if train else None
        if dp is not None:
            cap = int(dp.all_reduce([cap], op=torch.distributed.ReduceOp.MAX)[0])
            dp.plan(B, cap)
            cap *= dp.world
        bf = self._buffers(B, cap, train)
        csr = self._csr(data, B, rows, None)
        if train:
            self._check_steps(1)
        else:
            self.flush()
        self._launch(bf, csr, train, beta, p_drop, ext,
                     weight=(1.0 / dp.world if weight is None else weight) if dp is not None else 1.0)
        if train:
            self.host_step += 1
            self.flush()
            if dp is not None:
                dp.check()
        return bf.loss3

    def run_epoch(self, data: DeviceData, batch_size: int, shuffle: bool, beta_fn, p_drop: float,
                  train: bool = True, drop_last: bool = False, generator: torch.Generator | None = None,
                  max_batches: int | None = None) -> dict:
        """Iterate the dataset in batches (DataLoader semantics: shuffle, drop_last=False).

        beta_fn(step_index) -> beta; a constant beta (ConstBeta) or the annealed schedule evaluated on the device
        (AnnealedBeta) lets every full batch replay one graph.
        Returns the mean of the per-batch losses (VAETrainer.train_epoch's metric).
        """
        n = int(data.users.numel())
        if n == 0:
            nan = {"total_loss": float("nan"), "recon_loss": float("nan"), "kl_loss": float("nan")}
            if not train and self.dp is not None and not data.dp_global:
                # an empty shard still joins the other ranks' batch-weighted validation sum
                tot = self.dp.all_reduce([0.0, 0.0, 0.0, 0.0]).tolist()
                if tot[3] > 0:
                    return {"total_loss": tot[0] / tot[3], "recon_loss": tot[1] / tot[3], "kl_loss": tot[2] / tot[3]}
            return nan
        self.sync_embeddings()
        anneal = getattr(beta_fn, "anneal", None) if train else None
        if anneal is not None:
            self.anneal_dev.fill_(int(beta_fn.model.current_step))
        self._anneal = anneal
        try:
            if train and self.dp is not None:
                out, steps = self._run_epoch_dp(data, batch_size, shuffle, beta_fn, p_drop, drop_last, generator,
                                                max_batches)
            else:
                out, steps = self._run_epoch_local(data, batch_size, shuffle, beta_fn, p_drop, train, drop_last,
                                                   generator, max_batches)
        finally:
            self._anneal = None
        if anneal is not None:  # the host mirror of the device schedule counter (AnnealedVAE.step_annealing)
            beta_fn.model.current_step += steps
        return out

    @staticmethod
    def _step_beta(beta_fn, const_beta, anneal, i: int):
        """The beta argument of step i: the constant, a placeholder when the device schedule supplies it, or
        beta_fn(i) (a host schedule: eager steps)."""
        if const_beta is not None:
            return const_beta
        return 0.0 if anneal is not None else beta_fn(i)

    def _run_epoch_local(self, data: DeviceData, batch_size: int, shuffle: bool, beta_fn, p_drop: float,
                         train: bool, drop_last: bool, generator, max_batches) -> tuple[dict, int]:
        n = int(data.users.numel())
        shard_reduce = False
        if not train and self.dp is not None and data.users_host is not None:
            if data.dp_global:  # every rank holds every user: deal the single-GPU batches over the ranks
                return self._run_eval_sharded(data, batch_size, shuffle, beta_fn, p_drop, drop_last, generator,
                                              max_batches)
            # per-rank shards: each rank validates its whole shard, then the batch losses are summed over ranks
            shard_reduce = True
        if shuffle:
            order = _sampler_order(n, generator, self.device)
            data.perm.copy_(data.users[order.to(self.device)])
        else:
            data.perm.copy_(data.users)
        accum = self.accum_train if train else self.accum_val
        accum.zero_()
        self.boff.zero_()
        if train:
            self._check_steps(n // batch_size + 1)
        else:
            self.flush()  # the forward reads W1t rows that no catch-up precedes
        n_full, tail = divmod(n, batch_size)
        if drop_last:
            tail = 0
        if max_batches is not None:  # bounded pass (benchmarks): full batches only
            n_full, tail = min(n_full, max_batches), 0
        n_batches = n_full + (1 if tail else 0)
        const_beta = getattr(beta_fn, "constant", None)
        anneal = self._anneal
        B = batch_size
        bi = 0
        while bi < n_full:
            beta = self._step_beta(beta_fn, const_beta, anneal, bi)
            bf = self._buffers(B, data.max_batch_nnz(B), train)
            if self.use_graphs and (const_beta is not None or anneal is not None):
                done = self._replay(bf, data, train, beta, p_drop, bi, (beta, anneal, p_drop) + self._hyper(),
                                    n_full - bi)
            else:
                self._launch(bf, self._csr(data, B, data.perm, self.boff), train, beta, p_drop, advance=B)
                done = 1
            if train:
                self.host_step += done
            bi += done
        if tail:
            beta = self._step_beta(beta_fn, const_beta, anneal, n_full)
            bf = self._buffers(tail, data.max_batch_nnz(tail), train)
            self._launch(bf, self._csr(data, tail, data.perm, self.boff), train, beta, p_drop, advance=tail)
            if train:
                self.host_step += 1
        self.flush()
        sums = accum.cpu().tolist()  # the one host sync of the epoch
        if shard_reduce:  # batch-weighted: the mean over every rank's batches, as one GPU over all shards
            tot = self.dp.all_reduce(np.array(sums + [float(n_batches)], dtype=np.float64)).tolist()
            sums, n_batches = tot[:3], int(round(tot[3]))
        return ({"total_loss": sums[0] / n_batches, "recon_loss": sums[1] / n_batches,
                 "kl_loss": sums[2] / n_batches}, n_batches if train else 0)

    def _run_eval_sharded(self, data: DeviceData, B: int, shuffle: bool, beta_fn, p_drop: float, drop_last: bool,
                          generator, max_batches) -> tuple[dict, int]:
        """Data-parallel validation (VAETrainer.validate under torchrun): the epoch's batches -- the ones a single
        GPU would form, in its order -- are dealt round-robin over the ranks (batch i to rank i mod W), each rank
        runs its own through the same captured eval step, and the per-batch loss sums are all-reduced. Every
        batch is the single-GPU batch, so the result is the single-GPU validation loss up to the order of the
        fp64 sum over batches."""
        dp, W, r = self.dp, self.dp.world, self.dp.rank
        users = data.users_host
        n = len(users)
        if shuffle:  # one order on every rank
            if generator is not None:
                # the caller's generator decides it, as in a single-GPU run: every rank draws the permutation
                # exactly as _sampler_order does (so each generator ends in the state a single-GPU validation
                # leaves it in) and rank 0's permutation is broadcast (so the ranks agree even if their generators
                # do not): the batches are the single-GPU batches
                grp = dp.group
                on_dev = torch.distributed.get_backend(grp) == "nccl"
                perm = _sampler_order(n, generator, self.device).to(torch.int64)
                perm = perm.to(self.device if on_dev else "cpu")
                torch.distributed.broadcast(perm, torch.distributed.get_global_rank(grp, 0), group=grp)
                order = users[perm.cpu().numpy()]
            else:  # the shared data-parallel seed
                rng = np.random.default_rng([self.dp_seed, 0x5EA1, self.dp_val_epoch])
                self.dp_val_epoch += 1
                order = users[rng.permutation(n)]
        else:
            order = users
        n_full, tail = divmod(n, B)
        if drop_last:
            tail = 0
        if max_batches is not None:
            n_full, tail = min(n_full, max_batches), 0
        n_batches = n_full + (1 if tail else 0)
        mine_full = list(range(r, n_full, W))
        mine_tail = bool(tail) and n_full % W == r
        parts = [order[i * B:(i + 1) * B] for i in mine_full] + ([order[n_full * B:n_full * B + tail]] if mine_tail
                                                                   else [])
        if parts:
            mine = np.concatenate(parts).astype(np.int32)
            data.perm[:len(mine)].copy_(torch.as_tensor(mine).to(self.device))
        self.accum_val.zero_()
        self.boff.zero_()
        self.flush()  # the forward reads W1t rows that no catch-up precedes
        const_beta = getattr(beta_fn, "constant", None)
        for k, bi in enumerate(mine_full):
            beta = const_beta if const_beta is not None else beta_fn(bi)
            bf = self._buffers(B, data.max_batch_nnz(B), False)
            if self.use_graphs and const_beta is not None:
                self._replay(bf, data, False, beta, p_drop, k, (beta, None, p_drop) + self._hyper())
            else:
                self._launch(bf, self._csr(data, B, data.perm, self.boff), False, beta, p_drop, advance=B)
        if mine_tail:
            beta = const_beta if const_beta is not None else beta_fn(n_full)
            bf = self._buffers(tail, data.max_batch_nnz(tail), False)
            self._launch(bf, self._csr(data, tail, data.perm, self.boff), False, beta, p_drop, advance=tail)
        tot = dp.all_reduce(self.accum_val.cpu().numpy()).tolist()  # the batches' losses summed over the ranks
        if n_batches == 0:
            return {"total_loss": float("nan"), "recon_loss": float("nan"), "kl_loss": float("nan")}, 0
        return {"total_loss": tot[0] / n_batches, "recon_loss": tot[1] / n_batches,
                "kl_loss": tot[2] / n_batches}, 0

    def _replay(self, bf: _StepBuffers, data: DeviceData, train: bool, beta: float, p_drop: float, bi: int,
                key, left: int = 1) -> int:
        """Run full batches through their captured graph(s), capturing them first if needed; returns the steps
        run. The first use of a buffer set runs one step eagerly instead (loads kernels, sets attributes). A graph
        holds the DeviceData it reads (compared by identity, so a freed dataset's address reused by a new one
        never replays a stale graph). Single GPU: where `left` allows, one replay of the K-step graph runs K
        consecutive steps (the batch offset advances on the device), so the host pays one replay per K steps."""
        if bf.graph is None or bf.graph_key != key or bf.graph_data is not data:
            if bi == 0 and bf.graph is None:
                self._launch(bf, self._csr(data, bf.B, data.perm, self.boff), train, beta, p_drop, advance=bf.B,
                             weight=key[-1] if self.dp is not None and train else 1.0)
                return 1
            self._capture(bf, data, train, beta, p_drop, key)
        defer = train and self._defers(bf.B)
        if train and not defer:
            self._resolve_pending()  # the graph's forward reads rows without the recorded update's catch-up
        if bf.graph_k is not None and left >= bf.graph_k_steps:
            bf.graph_k.replay()
            self._pend_open = self._pend_open or defer
            return bf.graph_k_steps
        if bf.graph_pre is not None:  # data parallel: the CSR packet, then its exchange
            bf.graph_pre.replay()
            self.dp.communicate_csr()
        bf.graph.replay()
        if bf.graph_up is not None:  # data parallel: the gradients' exchange between the step's graphs
            self.dp.communicate_grads()
            bf.graph_up.replay()
        self._pend_open = self._pend_open or defer
        return 1

    # ------------------------------------------------------ data parallel ---
    def _dp_cap(self, data: DeviceData, B: int) -> int:
        """Entries of the largest batch of B users any rank can draw (agreed once per dataset and B)."""
        key = (id(data), B)
        hit = self._dp_caps.get(key)
        if hit is None or hit[0] is not data:
            cap = int(self.dp.all_reduce([data.max_batch_nnz(B)], op=torch.distributed.ReduceOp.MAX)[0])
            self._dp_caps[key] = hit = (data, max(cap, 1))
        return hit[1]

    def _run_epoch_dp(self, data: DeviceData, B: int, shuffle: bool, beta_fn, p_drop: float, drop_last: bool,
                      generator, max_batches) -> tuple[dict, int]:
        """A data-parallel training epoch (hvae/dist.py). data.dp_global: every rank holds every user and takes
        its slice of each global batch of a permutation drawn from the shared seed; otherwise the ranks'
        datasets are their own shards, which must have equal sizes."""
        from .dist import dp_shard
        dp, W, r = self.dp, self.dp.world, self.dp.rank
        users = data.users_host
        n = len(users)
        if data.dp_global:
            rng = np.random.default_rng([self.dp_seed, self.dp_epoch])
            order = users[rng.permutation(n)] if shuffle else users
            mine, n_full, counts = dp_shard(order, B, W, r)
        else:
            sizes = dp.all_reduce([n, -n], op=torch.distributed.ReduceOp.MAX)
            if int(sizes[0]) != n or int(-sizes[1]) != n:
                raise ValueError("data-parallel shards of unequal sizes: give every rank the whole dataset "
                                 "(DeviceData.dp_global) or equal shards")
            # the rank's own shard in the sampler's order, gathered on the device (a host round trip of the
            # order and the users cost ~10-45 ms per epoch at 1.25 M users: scripts/bench_dp_emul.py)
            order = _sampler_order(n, generator, self.device) if shuffle else None
            mine = data.users[order.to(self.device)] if order is not None else data.users
            n_full, t = divmod(n, B)
            counts = [t] * W
        self.dp_epoch += 1
        if drop_last:
            counts = [0] * W
        if max_batches is not None:
            n_full, counts = min(n_full, max_batches), [0] * W
        if isinstance(mine, torch.Tensor):
            data.perm[:len(mine)].copy_(mine)
        else:
            data.perm[:len(mine)].copy_(torch.as_tensor(np.asarray(mine, dtype=np.int32)).to(self.device))
        self.accum_train.zero_()
        self.boff.zero_()
        n_steps = n_full + (1 if sum(counts) else 0)
        self._check_steps(n_steps + 1)
        const_beta = getattr(beta_fn, "constant", None)
        anneal = self._anneal
        cap = self._dp_cap(data, B)
        if n_full:
            dp.plan(B, cap)
        for bi in range(n_full):
            beta = self._step_beta(beta_fn, const_beta, anneal, bi)
            bf = self._buffers(B, W * cap, True)
            if self.use_graphs and (const_beta is not None or anneal is not None):
                self._replay(bf, data, True, beta, p_drop, bi, (beta, anneal, p_drop) + self._hyper() + (cap, 1.0 / W))
            else:
                self._launch(bf, self._csr(data, B, data.perm, self.boff), True, beta, p_drop, advance=B,
                             weight=1.0 / W)
            self.host_step += 1
        sums = self.accum_train.cpu().numpy() / W  # the union batch's loss = mean of equal shares
        if sum(counts):  # the last, partial global batch: eager, every rank takes part (possibly with no users)
            T, c, Bt = sum(counts), counts[r], max(counts)
            beta = self._step_beta(beta_fn, const_beta, anneal, n_full)
            dp.plan(Bt, cap)
            bf = self._buffers(Bt, W * cap, True)
            if c:
                bfc = self._buffers(c, W * cap, True)
                csr = self._csr(data, c, data.perm, self.boff)
                self._launch_pack_csr(bfc, csr, c / T)
            else:
                self._launch_pack_csr(None, None, 0.0)
            dp.communicate_csr()
            if c:
                self.accum_train.zero_()
                self._launch_fwd_bwd(bfc, csr, True, beta, p_drop, None)
                self._launch_pack_grads(bfc, c / T)
                sums = sums + self.accum_train.cpu().numpy() * (c / T)
            else:  # no users here: the union batch's plan still runs (and the schedule counter advances)
                self._resolve_pending()  # (no forward here to carry it; the apply below rewrites the rows it reads)
                dp.merge_plan()
                self._launch_pack_grads(None, 0.0)
                if anneal is not None:
                    ops.counter_add(self.anneal_dev, 1)
            dp.communicate_grads()
            self._launch_dp_update(bf, c)
            self.host_step += 1
        self.flush()
        dp.check()
        tot = dp.all_reduce(sums).tolist()  # the union batches' losses summed over the steps (Python floats:
        # the metrics go into checkpoints, which load with weights_only=True)
        return ({"total_loss": tot[0] / n_steps, "recon_loss": tot[1] / n_steps, "kl_loss": tot[2] / n_steps},
                n_steps)

    def _capture(self, bf: _StepBuffers, data: DeviceData, train: bool, beta: float, p_drop: float, key):
        """One graph per step (single GPU); data-parallel: the CSR packet | forward/backward (the union plan
        beside it) + the gradient packet | union apply + clip + Adam, with the collectives launched eagerly in
        between (they stay out of the graphs)."""
        csr = self._csr(data, bf.B, data.perm, self.boff)
        bf.csr_keepalive = csr
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        if self.dp is None or not train:
            with torch.cuda.graph(g):
                self._launch(bf, csr, train, beta, p_drop, advance=bf.B)
            bf.graph_pre = bf.graph_up = None
            k = self._steps_per_graph(bf.B) if self.dp is None else 1
            bf.graph_k, bf.graph_k_steps = None, 0
            if k > 1:  # the same step K times: each one reads the batch offset the previous one advanced
                gk = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gk):
                    for _ in range(k):
                        self._launch(bf, csr, train, beta, p_drop, advance=bf.B)
                bf.graph_k, bf.graph_k_steps = gk, k
        else:
            g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g0):
                self._launch_pack_csr(bf, csr, key[-1])
            with torch.cuda.graph(g):
                self._launch_fwd_bwd(bf, csr, train, beta, p_drop, None)
                self._launch_pack_grads(bf, key[-1])
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                self._launch_dp_update(bf, bf.B)
            bf.graph_pre, bf.graph_up = g0, g2
        bf.graph = g
        bf.graph_key = key
        bf.graph_data = data

    def _steps_per_graph(self, B: int) -> int:
        """Steps per replay for batch size B: a step of a few hundred microseconds is host-bound on one replay
        per step (HVAE_STEPS_PER_GRAPH overrides)."""
        env = os.environ.get("HVAE_STEPS_PER_GRAPH")
        if env:
            return max(1, int(env))
        return 8 if B <= 1024 else 1

    def sync_state_to_model(self):
        """Parameters are views of the flat buffer already; nothing to copy."""
        return None


class ConstBeta:
    def __init__(self, beta: float):
        self.constant = float(beta)

    def __call__(self, _i):
        return self.constant


class AnnealedBeta:
    """AnnealedVAE's linear KL-weight schedule (reference src/ml/model.py:312-334) for a fused epoch.

    run_epoch evaluates it on the device (hvae_anneal_beta: one launch per train step that reads and advances a
    device copy of model.current_step), so annealed epochs replay one captured step like constant-beta ones, and
    then advances model.current_step by the steps it ran. Called directly (eager steps over other iterables) it is
    the reference's _compute_loss order: the current beta, then step_annealing()."""

    def __init__(self, model):
        self.model = model
        self.anneal = (float(model.beta_min), float(model.beta_max), int(model.anneal_steps))

    def __call__(self, _i):
        b = self.model.get_current_beta()
        self.model.step_annealing()
        return b
