"""Mult-VAE baseline on MI355X -- the reference's MultVAE / MultVAERecommender (src/ml/baseline.py:126-231), trained
and evaluated on the device (`make baseline-multvae`).

The reference densifies the interaction matrix and runs a dense torch loop. Here the rows stay sparse: a step is
launches of libhvae only. New kernels (csrc/hvae_mvae.hip) where the library had none -- the first layer over sparse
rows with its normalisation, dropouts and tanh (hvae_mvae_encoder_fwd), the elementwise tanh + dropout and its
backward (hvae_mvae_tanh_drop_*), and the multinomial loss with its gradient against the sparse target, in place over
the stored logits (hvae_mvae_nll) -- and the existing entry points for everything else: hvae_gemm_f32 for every dense
product (bias through its epilogue), hvae_colsum for the bias gradients, hvae_w1_rowgrad for the row-sparse gradient
of the first weight, hvae_reparam_kl_* for the latent, hvae_adam_rows / hvae_adam_dense, hvae_loss_finalize. The
step loop never synchronises with the host: an epoch's order goes to the device once, and the summed loss is read
only at the epochs the reference logs.

Draws. The initial parameters come from torch's CPU generator, the nn.Linear modules of MultVAE.__init__ in its
order (init_params). Each epoch's order is torch's own DataLoader(shuffle=True) iterated on the host (epoch_order),
which consumes the global generator as the reference's loader does. The dropout masks and eps are not drawn on the
host: they are the device Philox streams keyed by (seed, step) -- the reference draws them from whatever device it
runs on, so there is no canonical stream to follow. TrainSteps.run also takes injected masks and eps, which is how the
tests follow the reference. Scoring, ranking, ties and negatives are src/ml/baseline.py's (evaluate_model),
unchanged; main() sets the "Mult-VAE" entry of models/figures/baseline_results.json beside the existing entries.
"""
from __future__ import annotations

import logging

import numpy as np
import torch
from scipy.sparse import csr_matrix

from hvae import _lib, ops

from .baseline import BaseRecommender, _resolve_device, parse_args, run_baseline

logger = logging.getLogger(__name__)

NAME = "Mult-VAE"
BATCH_SIZE = 512      # the reference's loader (baseline.py:203)
DROPOUT = 0.5         # MultVAE's default, which the recommender never overrides (baseline.py:130, 198)
SERVED_HIDDEN = (4, ops.MVAE_MAX_HIDDEN)
SERVED_LATENT = (4, ops.MVAE_MAX_LATENT)
# the reference module's state_dict, in the order MultVAE.__init__ constructs (and draws) its nn.Linear modules
LINEARS = ("encoder.0", "encoder.3", "mu_layer", "logvar_layer", "decoder.0", "decoder.2")


def linear_shapes(n_items: int, hidden_dim: int, latent_dim: int) -> dict[str, tuple[int, int]]:
    """name -> (out_features, in_features) of every nn.Linear of MultVAE (baseline.py:133-147)."""
    N, H, L = n_items, hidden_dim, latent_dim
    return {"encoder.0": (H, N), "encoder.3": (H, H), "mu_layer": (L, H), "logvar_layer": (L, H),
            "decoder.0": (H, L), "decoder.2": (N, H)}


def init_params(n_items: int, hidden_dim: int, latent_dim: int) -> dict[str, torch.Tensor]:
    """The initial parameters from torch's CPU generator, draw for draw MultVAE.__init__: one nn.Linear per layer in
    the reference's order (the Tanh and Dropout modules between them draw nothing). Keys and shapes are the
    reference module's state_dict."""
    out = {}
    for name, (o, i) in linear_shapes(n_items, hidden_dim, latent_dim).items():
        lin = torch.nn.Linear(i, o)
        out[f"{name}.weight"] = lin.weight.detach().clone()
        out[f"{name}.bias"] = lin.bias.detach().clone()
    return out


def epoch_order(n_users: int, batch_size: int = BATCH_SIZE) -> np.ndarray:
    """One epoch's user order (int32 [n_users]) from torch's own DataLoader(shuffle=True) over arange(n_users),
    iterated on the host: it consumes the global generator exactly as the reference's loader does (baseline.py:203,
    208). Batch k is order[k * batch_size : (k + 1) * batch_size]; the last one is ragged."""
    from torch.utils.data import DataLoader, TensorDataset
    loader = DataLoader(TensorDataset(torch.arange(n_users)), batch_size=batch_size, shuffle=True)
    parts = [b for (b,) in loader]
    order = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64)
    return order.numpy().astype(np.int32)


def batch_capacity(matrix: csr_matrix, batch_size: int = BATCH_SIZE) -> int:
    """The most stored entries any batch of batch_size distinct rows can hold."""
    lens = np.sort(np.diff(matrix.tocsr().indptr))[::-1]
    return max(int(lens[:batch_size].sum()), 1)


class TrainSteps:
    """The device state of a Mult-VAE training run and its step. Nothing in run() waits for the device.

    W1t [N, H] (the item-major image of encoder.0.weight) has its own Adam state and a row-sparse gradient; every
    other parameter lives in one flat arena (`flat`, with `grad`, `m`, `v` of the same layout) so that one
    hvae_adam_dense updates them all. The two heads are one [2L, H] weight: mu's rows, then logvar's."""

    def __init__(self, matrix: csr_matrix, params: dict[str, torch.Tensor], device, lr: float = 1e-3,
                 beta: float = 0.2, seed: int = 0, dropout: float = DROPOUT, batch_size: int = BATCH_SIZE):
        matrix = matrix.tocsr()
        self.n_users, self.N = matrix.shape
        self.H, self.L = (int(s) for s in params["decoder.0.weight"].shape)
        self.beta, self.seed, self.p, self.batch_size = float(beta), int(seed), float(dropout), int(batch_size)
        self.device = dev = device
        N, H, L, B = self.N, self.H, self.L, self.batch_size
        f32 = dict(dtype=torch.float32, device=dev)

        self.x = ops.csr_from_scipy(matrix, dev)
        self.xs = torch.zeros_like(self.x.vals)          # the encoder's scaled entries, indexed like x.vals
        self.W1t = params["encoder.0.weight"].t().contiguous().to(dev)
        self.m1, self.v1 = torch.zeros_like(self.W1t), torch.zeros_like(self.W1t)
        self.rg = ops.RowGradBuffers(N, H, batch_capacity(matrix, B), dev)

        sizes = [("b1", (H,)), ("W2", (H, H)), ("b2", (H,)), ("Wh", (2 * L, H)), ("bh", (2 * L,)), ("Wd1", (H, L)),
                 ("bd1", (H,)), ("Wd2", (N, H)), ("bd2", (N,))]
        total = sum(int(np.prod(s)) for _, s in sizes)
        self.flat, self.grad = torch.zeros(total, **f32), torch.zeros(total, **f32)
        self.m, self.v = torch.zeros(total, **f32), torch.zeros(total, **f32)
        self.P, self.G, off = {}, {}, 0
        for name, shape in sizes:  # every segment but the last holds a multiple of 4 floats: all 16-B aligned
            n = int(np.prod(shape))
            self.P[name], self.G[name] = self.flat[off:off + n].view(shape), self.grad[off:off + n].view(shape)
            off += n
        P = self.P
        P["b1"].copy_(params["encoder.0.bias"])
        P["W2"].copy_(params["encoder.3.weight"])
        P["b2"].copy_(params["encoder.3.bias"])
        P["Wh"].copy_(torch.cat([params["mu_layer.weight"], params["logvar_layer.weight"]], dim=0))
        P["bh"].copy_(torch.cat([params["mu_layer.bias"], params["logvar_layer.bias"]], dim=0))
        P["Wd1"].copy_(params["decoder.0.weight"])
        P["bd1"].copy_(params["decoder.0.bias"])
        P["Wd2"].copy_(params["decoder.2.weight"])
        P["bd2"].copy_(params["decoder.2.bias"])

        self.lds = (N + 3) // 4 * 4                        # the logits' leading dimension
        self.S = torch.empty(B, self.lds, **f32)
        self.t1, self.h1, self.t2, self.h2, self.td, self.dH = (torch.empty(B, H, **f32) for _ in range(6))
        self.heads, self.dheads = torch.empty(B, 2 * L, **f32), torch.empty(B, 2 * L, **f32)
        self.dz = torch.empty(B, L, **f32)
        self.lse, self.recon = torch.empty(B, **f32), torch.empty(B, **f32)
        self.loss3 = torch.zeros(3, **f32)                 # the last step's (total, recon, kl)
        self.total = torch.zeros(3, dtype=torch.float64, device=dev)  # the epoch's summed (total, recon, kl)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.adam = ops.adam_config(lr, (0.9, 0.999), 1e-8, 0.0, self.step)  # torch.optim.Adam's defaults (:199)
        self.n_batches = 0

    # ------------------------------------------------------------------------------------------------ epochs --
    def load_epoch(self, order: np.ndarray) -> None:
        """One epoch's user order to the device; clears the summed loss."""
        self.order = torch.as_tensor(np.ascontiguousarray(order, dtype=np.int32), device=self.device)
        self.n = len(order)
        self.n_batches = (self.n + self.batch_size - 1) // self.batch_size
        self.total.zero_()

    def _batch(self, rows: torch.Tensor, vals: torch.Tensor) -> ops.Csr:
        return ops.Csr(self.x.row_ptr, self.x.col_idx, vals, self.N, rows=rows)

    @staticmethod
    def _bias(b: torch.Tensor):
        return ops.epilogue(_lib.EPI_BIAS, bias=b)

    # -------------------------------------------------------------------------------------------------- step --
    def run(self, k: int, inject: dict | None = None) -> None:
        """Train step k of the loaded epoch. inject (parity mode): {"in_mult": float32 indexed like the matrix's
        stored values, "m1", "m2": [nb, H] multipliers, "eps": [nb, L]}, all on the device; absent entries are
        drawn from the Philox streams."""
        inj = inject or {}
        s, e = k * self.batch_size, min((k + 1) * self.batch_size, self.n)
        nb, N, L, P, G, p = e - s, self.N, self.L, self.P, self.G, self.p
        rows = self.order[s:e]
        x = self._batch(rows, self.x.vals)
        t1, h1, t2, h2, td, dH = (b[:nb] for b in (self.t1, self.h1, self.t2, self.h2, self.td, self.dH))
        heads, dheads, dz, S = self.heads[:nb], self.dheads[:nb], self.dz[:nb], self.S[:nb]
        seed, step = self.seed, self.step

        # forward
        ops.mvae_encoder_fwd(x, self.W1t, P["b1"], p, p, True, seed, step, in_mult=inj.get("in_mult"),
                             drop_mult=inj.get("m1"), xs_out=self.xs, t_out=t1, h_out=h1)
        ops.gemm(h1, P["W2"].t(), out=t2, epi=self._bias(P["b2"]))
        ops.mvae_tanh_drop_fwd(t2, p, True, _lib.TAG_MVAE_HID2, seed, step, drop_mult=inj.get("m2"), t_out=t2,
                               h_out=h2)
        ops.gemm(h2, P["Wh"].t(), out=heads, epi=self._bias(P["bh"]))
        mu, lv = heads[:, :L], heads[:, L:]
        z, eps, kl_rows = ops.reparam_kl_fwd(mu, lv, True, seed, step, eps_in=inj.get("eps"))
        ops.gemm(z, P["Wd1"].t(), out=td, epi=self._bias(P["bd1"]))
        ops.mvae_tanh_drop_fwd(td, 0.0, False, 0, t_out=td, h_out=td)
        ops.gemm(td, P["Wd2"].t(), out=S[:, :N], epi=self._bias(P["bd2"]))
        ops.mvae_nll(x, S, 1.0 / nb, self.lse[:nb], self.recon[:nb])
        ops.loss_finalize(self.recon[:nb], kl_rows, self.beta, self.loss3, self.total)

        # backward: S now holds d loss / d logits
        dS = S[:, :N]
        ops.gemm(dS.t(), td, out=G["Wd2"])
        ops.colsum(dS, out=G["bd2"])
        ops.gemm(dS, P["Wd2"], out=dH)
        ops.mvae_tanh_drop_bwd(dH, td, 0.0, False, 0, da=dH)
        ops.gemm(dH.t(), z, out=G["Wd1"])
        ops.colsum(dH, out=G["bd1"])
        ops.gemm(dH, P["Wd1"], out=dz)
        ops.reparam_kl_bwd(dz, mu, lv, eps, self.beta / nb, True, dmu=dheads[:, :L], dlv=dheads[:, L:])
        ops.gemm(dheads.t(), h2, out=G["Wh"])
        ops.colsum(dheads, out=G["bh"])
        ops.gemm(dheads, P["Wh"], out=dH)
        ops.mvae_tanh_drop_bwd(dH, t2, p, True, _lib.TAG_MVAE_HID2, seed, step, drop_mult=inj.get("m2"), da=dH)
        ops.gemm(dH.t(), h1, out=G["W2"])
        ops.colsum(dH, out=G["b2"])
        ops.gemm(dH, P["W2"], out=h2)                      # h2 is free now: d loss / d h1
        ops.mvae_tanh_drop_bwd(h2, t1, p, True, _lib.TAG_MVAE_HID1, seed, step, drop_mult=inj.get("m1"), da=h2)
        ops.colsum(h2, out=G["b1"])
        ops.w1_rowgrad(self._batch(rows, self.xs), h2, self.rg)

        # torch.optim.Adam: dense moments, so W1t's rows outside the batch decay too (hvae_adam_rows)
        ops.adam_rows(self.adam, self.W1t, self.m1, self.v1, self.rg)
        ops.adam_dense(self.adam, self.flat, self.m, self.v, self.grad)
        ops.counter_add(self.step)

    # ------------------------------------------------------------------------------------------------- eval ---
    def hidden(self, users: np.ndarray) -> torch.Tensor:
        """The eval-mode chain up to the last hidden layer, [B, H]: no dropout, z = mu."""
        rows = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=self.device)
        P, L = self.P, self.L
        h, _, _ = ops.mvae_encoder_fwd(self._batch(rows, self.x.vals), self.W1t, P["b1"], 0.0, 0.0, False,
                                       save=False)
        a = ops.gemm(h, P["W2"].t(), epi=self._bias(P["b2"]))
        ops.mvae_tanh_drop_fwd(a, 0.0, False, 0, t_out=a, h_out=a)
        mu = ops.gemm(a, P["Wh"][:L].t(), epi=self._bias(P["bh"][:L]))
        d = ops.gemm(mu, P["Wd1"].t(), epi=self._bias(P["bd1"]))
        ops.mvae_tanh_drop_fwd(d, 0.0, False, 0, t_out=d, h_out=d)
        return d

    def state_dict(self) -> dict[str, torch.Tensor]:
        """The parameters under the reference module's key names and shapes (host tensors)."""
        P, L = self.P, self.L
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        return {"encoder.0.weight": c(self.W1t.t()).contiguous(), "encoder.0.bias": c(P["b1"]),
                "encoder.3.weight": c(P["W2"]), "encoder.3.bias": c(P["b2"]),
                "mu_layer.weight": c(P["Wh"][:L]), "mu_layer.bias": c(P["bh"][:L]),
                "logvar_layer.weight": c(P["Wh"][L:]), "logvar_layer.bias": c(P["bh"][L:]),
                "decoder.0.weight": c(P["Wd1"]), "decoder.0.bias": c(P["bd1"]),
                "decoder.2.weight": c(P["Wd2"]), "decoder.2.bias": c(P["bd2"])}


def _check_dim(name: str, value: int, served: tuple[int, int]) -> None:
    if not (served[0] <= int(value) <= served[1] and int(value) % 4 == 0):
        raise ValueError(f"Mult-VAE: {name} {value} is not served; served: multiples of 4 from {served[0]} to "
                         f"{served[1]}")


class MultVAERecommender(BaseRecommender):
    """The reference's MultVAERecommender (baseline.py:166-231) with its attributes (fit, predict) plus the batched
    device scoring that baseline.evaluate_model uses. `seed` keys the device's dropout and eps streams."""

    def __init__(self, hidden_dim: int = 600, latent_dim: int = 200, epochs: int = 50, lr: float = 1e-3,
                 beta: float = 0.2, device=None, seed: int = 0):
        _check_dim("hidden_dim", hidden_dim, SERVED_HIDDEN)
        _check_dim("latent_dim", latent_dim, SERVED_LATENT)
        self.hidden_dim = hidden_dim
        self.latent_dim = latent_dim
        self.epochs = epochs
        self.lr = lr
        self.beta = beta
        self.seed = seed
        self._device_arg = device
        self.matrix: csr_matrix | None = None
        self.steps: TrainSteps | None = None
        self.epoch_losses: list[float] = []  # the mean batch loss of every 10th epoch, as the reference logs it

    def fit(self, interaction_matrix: csr_matrix) -> None:
        logger.info(f"Fitting Mult-VAE (latent={self.latent_dim}, epochs={self.epochs})...")
        self.matrix = interaction_matrix
        n_users, n_items = interaction_matrix.shape
        params = init_params(n_items, self.hidden_dim, self.latent_dim)
        self.device = dev = _resolve_device(self._device_arg)
        self.steps = steps = TrainSteps(interaction_matrix, params, dev, self.lr, self.beta, self.seed)
        self.epoch_losses = []
        for epoch in range(self.epochs):
            steps.load_epoch(epoch_order(n_users))
            for k in range(steps.n_batches):
                steps.run(k)
            if (epoch + 1) % 10 == 0:
                self.epoch_losses.append(float(steps.total[0].item()) / max(steps.n_batches, 1))
                logger.info(f"  Epoch {epoch + 1}/{self.epochs}, Loss: {self.epoch_losses[-1]:.4f}")

    def state_dict(self) -> dict[str, torch.Tensor]:
        assert self.steps is not None, "Model not fitted"
        return self.steps.state_dict()

    def predict(self, user_idx: int) -> np.ndarray:
        return self.score_all(np.array([user_idx]))[0].cpu().numpy()

    def score_candidates(self, users: np.ndarray, cand: torch.Tensor) -> torch.Tensor:
        P = self.steps.P
        d = self.steps.hidden(users)
        local = torch.arange(len(users), dtype=torch.int32, device=self.device)
        cand = cand.contiguous()
        return ops.score_candidates(d, local, P["Wd2"], cand) + P["bd2"][cand.long()]

    def score_all(self, users: np.ndarray) -> torch.Tensor:
        P = self.steps.P
        return ops.gemm(self.steps.hidden(users), P["Wd2"].t(), epi=TrainSteps._bias(P["bd2"]))


def run_multvae(data_dir: str, k_values: list[int] | None = None, n_negatives: int | None = 99, epochs: int = 50,
                seed: int = 0, hidden_dim: int = 600, latent_dim: int = 200) -> dict:
    """Fit and evaluate Mult-VAE as the reference's run_all_baselines does for one model (baseline.py:474-533)."""
    model = MultVAERecommender(hidden_dim, latent_dim, epochs=epochs, seed=seed)
    return run_baseline(model, NAME, data_dir, k_values, n_negatives)


def _add_flags(parser) -> None:
    parser.add_argument("--epochs", type=int, default=50)
    parser.add_argument("--seed", type=int, default=0, help="keys the device's dropout and eps streams")


def main() -> None:
    args = parse_args("Train and evaluate the Mult-VAE baseline (MI355X)", _add_flags)
    run_multvae(args.data, args.k_values, args.n_negatives, epochs=args.epochs, seed=args.seed)


if __name__ == "__main__":
    main()
