"""The Mult-VAE tests' graphs and a restatement of the model's train step in torch (not collected: no test_ prefix).

The restatement is written from the model's definition, dense and with autograd, in any
dtype: float64 is the tests' reference and the distance between its float32 and float64 runs from the same draws
is the noise that sets their bars. It takes the dropout multipliers and eps as inputs, so it follows whatever stream
the caller hands it.

  xs   = x / max(||x||_2, 1e-12) * in_mult                     (rows of the dense batch)
  h1   = tanh(xs W1^T + b1) * m1;   h2 = tanh(h1 W2^T + b2) * m2
  mu   = h2 Wmu^T + bmu;  lv = h2 Wlv^T + blv;  z = mu + exp(lv / 2) eps   (z = mu in eval mode)
  S    = tanh(z Wd1^T + bd1) Wd2^T + bd2
  loss = -mean_b sum_j log_softmax(S)_bj x_bj + beta * (-1/2 mean_b sum_l (1 + lv - mu^2 - e^lv))
"""
from __future__ import annotations

import hashlib
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import torch
from scipy.sparse import csr_matrix

GOLDEN = Path(__file__).resolve().parent / "golden"
U = 2.0 ** -24  # float32 unit roundoff
KEYS = ("encoder.0", "encoder.3", "mu_layer", "logvar_layer", "decoder.0", "decoder.2")
BATCH = 512
P_DROP = 0.5


def _canonical(rows, cols, vals, shape) -> csr_matrix:
    m = csr_matrix((np.asarray(vals, np.float64), (np.asarray(rows), np.asarray(cols))), shape=shape)
    m.sum_duplicates()
    m.sort_indices()
    return m


@lru_cache(maxsize=None)
def g_small() -> csr_matrix:
    """600 users x 97 items (an epoch is 512 + 88): user 0 is empty, user 1 has one item, user 2 has 85, a few
    entries are 2.0, item 96 belongs to nobody."""
    rng = np.random.Generator(np.random.PCG64(20))
    n_users, n_items = 600, 97
    rows, cols, vals = [], [], []
    for u in range(n_users):
        k = 0 if u == 0 else 1 if u == 1 else 85 if u == 2 else int(rng.integers(2, 12))
        # users sit in one of three taste groups so that there is something to learn
        lo = (u % 3) * 32
        pool = np.arange(96) if u == 2 else np.concatenate([np.arange(lo, lo + 32)] * 3 + [np.arange(96)])
        items = rng.choice(np.unique(pool) if u == 2 else pool, size=k, replace=(u != 2))
        for j in np.unique(items):
            rows.append(u), cols.append(int(j)), vals.append(2.0 if rng.random() < 0.03 else 1.0)
    m = _canonical(rows, cols, vals, (n_users, n_items))
    lens = np.diff(m.indptr)
    assert lens[0] == 0 and lens[1] == 1 and lens[2] >= 80 and (m.data == 2.0).sum() >= 3
    assert m.getnnz(axis=0)[96] == 0
    return m


@lru_cache(maxsize=None)
def g_wide() -> csr_matrix:
    """37 users x 4,101 items; user 5 has 300 entries."""
    rng = np.random.Generator(np.random.PCG64(21))
    n_users, n_items = 37, 4101
    rows, cols, vals = [], [], []
    for u in range(n_users):
        k = 300 if u == 5 else int(rng.integers(1, 40))
        for j in rng.choice(n_items, size=k, replace=False):
            rows.append(u), cols.append(int(j)), vals.append(2.0 if rng.random() < 0.05 else 1.0)
    m = _canonical(rows, cols, vals, (n_users, n_items))
    assert np.diff(m.indptr)[5] == 300
    return m


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def entry_mult(matrix: csr_matrix, rows, dense_mult: np.ndarray) -> np.ndarray:
    """The input multipliers of a batch (dense_mult [nb, N], batch row b = matrix row rows[b]) in entry order:
    float32 indexed like matrix.data; entries of rows outside the batch are 1."""
    out = np.ones(matrix.nnz, np.float32)
    for b, r in enumerate(np.asarray(rows)):
        s, e = matrix.indptr[r], matrix.indptr[r + 1]
        out[s:e] = dense_mult[b, matrix.indices[s:e]]
    return out


def random_params(n_items: int, H: int, L: int, seed: int, scale: float = 1.0) -> dict[str, torch.Tensor]:
    """float32 parameters under the reference module's keys, nn.Linear-like magnitudes, from a private generator."""
    g = torch.Generator().manual_seed(seed)
    shapes = {"encoder.0": (H, n_items), "encoder.3": (H, H), "mu_layer": (L, H), "logvar_layer": (L, H),
              "decoder.0": (H, L), "decoder.2": (n_items, H)}
    out = {}
    for k, (o, i) in shapes.items():
        bound = scale / np.sqrt(i)
        out[f"{k}.weight"] = (torch.rand(o, i, generator=g) * 2 - 1) * bound
        out[f"{k}.bias"] = (torch.rand(o, generator=g) * 2 - 1) * bound
    return out


def forward(p: dict[str, torch.Tensor], x: torch.Tensor, in_mult=None, m1=None, m2=None, eps=None):
    """-> (S, mu, lv) in p's dtype; every multiplier None means eval mode (no dropout, z = mu)."""
    one = lambda m: 1.0 if m is None else m  # noqa: E731
    den = x.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    xs = x / den * one(in_mult)
    h1 = torch.tanh(xs @ p["encoder.0.weight"].t() + p["encoder.0.bias"]) * one(m1)
    h2 = torch.tanh(h1 @ p["encoder.3.weight"].t() + p["encoder.3.bias"]) * one(m2)
    mu = h2 @ p["mu_layer.weight"].t() + p["mu_layer.bias"]
    lv = h2 @ p["logvar_layer.weight"].t() + p["logvar_layer.bias"]
    z = mu if eps is None else mu + torch.exp(0.5 * lv) * eps
    d = torch.tanh(z @ p["decoder.0.weight"].t() + p["decoder.0.bias"])
    return d @ p["decoder.2.weight"].t() + p["decoder.2.bias"], mu, lv


def loss_terms(S, mu, lv, x, beta: float):
    recon = -(torch.log_softmax(S, dim=1) * x).sum(dim=1).mean()
    kl = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(dim=1).mean()
    return recon + beta * kl, recon, kl


class Model:
    """The parameters in one dtype with torch.optim.Adam(lr) over them; step() is one train step from given draws."""

    def __init__(self, params: dict[str, torch.Tensor], dtype, lr: float = 1e-3, beta: float = 0.2):
        self.p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
        self.dtype, self.beta = dtype, beta
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr)

    def _t(self, a):
        return None if a is None else torch.as_tensor(a).to(self.dtype)

    def step(self, x, in_mult, m1, m2, eps):
        """-> ((total, recon, kl) floats, {key: gradient clone}); the parameters are updated."""
        self.opt.zero_grad()
        x = self._t(x)
        S, mu, lv = forward(self.p, x, self._t(in_mult), self._t(m1), self._t(m2), self._t(eps))
        total, recon, kl = loss_terms(S, mu, lv, x, self.beta)
        total.backward()
        grads = {k: v.grad.detach().clone() for k, v in self.p.items()}
        self.opt.step()
        return tuple(float(v.detach()) for v in (total, recon, kl)), grads

    @torch.no_grad()
    def scores(self, x) -> np.ndarray:
        return forward(self.p, self._t(x))[0].numpy()

    def state(self) -> dict[str, torch.Tensor]:
        return {k: v.detach().clone() for k, v in self.p.items()}


def encoder64(matrix: csr_matrix, rows, w1t: np.ndarray, b1: np.ndarray, in_mult=None, m1=None):
    """float64 first layer of the batch `rows` -> (xs in entry order [nnz of the matrix, NaN outside the batch],
    a, t, h, A) with A = |b1| + sum_e |xs_e w_e| (the magnitude the rounding bound scales with) and cnt [nb]."""
    w = w1t.astype(np.float64)
    nb, H = len(rows), w.shape[1]
    xs = np.full(matrix.nnz, np.nan)
    a, A = np.tile(b1.astype(np.float64), (nb, 1)), np.tile(np.abs(b1.astype(np.float64)), (nb, 1))
    cnt = np.zeros(nb, np.int64)
    for b, r in enumerate(np.asarray(rows)):
        s, e = matrix.indptr[r], matrix.indptr[r + 1]
        v = matrix.data[s:e].astype(np.float64)
        den = max(np.sqrt((v * v).sum()), 1e-12)
        x = v / den * (1.0 if in_mult is None else in_mult[s:e].astype(np.float64))
        xs[s:e] = x
        a[b] += x @ w[matrix.indices[s:e]]
        A[b] += np.abs(x) @ np.abs(w[matrix.indices[s:e]])
        cnt[b] = e - s
    t = np.tanh(a)
    h = t if m1 is None else t * m1.astype(np.float64)
    return xs, a, t, h, A, cnt


def fixture():
    return np.load(GOLDEN / "multvae.npz")


def fixture_meta() -> dict:
    return json.loads((GOLDEN / "multvae_meta.json").read_text())


# ------------------------------------------------------------------------------- the reference's trajectory ----
# tests/golden/make_multvae_fixture.py observes the reference's own MultVAERecommender on g_small() with these seeds.
# Its dropout multipliers and eps are handed to it (the reference draws them from whatever device it runs on, so
# it has no canonical stream): they are tests/philox_ref.py's, a pure function of (SEED_DEV, step, tag, element),
# so no mask is stored and the device's own Philox masks follow the same run. eps is philox_ref.normal32 (numpy's
# float32 evaluation); the device's logf / cospif differ from numpy's in the last bits, so the tests inject it.
SEED_TORCH = 1234        # torch.manual_seed before the fit: the initial parameters and every epoch's order
SEED_DEV = 2024          # the dropout and eps streams
HIDDEN, LATENT = 600, 200
FIX_EPOCHS = (1, 3)
BAR_FACTOR = 16
TAG_IN, TAG_H1, TAG_H2 = 0x400, 0x401, 0x402


def draws(step: int, nb: int, n_items: int, H: int = HIDDEN, L: int = LATENT, seed: int = SEED_DEV):
    """(in_mult [nb, N], m1 [nb, H], m2 [nb, H], eps [nb, L]) float32 of train step `step` (0-based, counted over
    the whole fit)."""
    import philox_ref as PR
    return (PR.mult(seed, step, TAG_IN, nb, n_items, P_DROP), PR.mult(seed, step, TAG_H1, nb, H, P_DROP),
            PR.mult(seed, step, TAG_H2, nb, H, P_DROP), PR.normal32(seed, step, nb, L))


def fixture_tests(matrix: csr_matrix):
    """(users, test items) of the fixture's evaluation: every user, one seeded item outside the user's row."""
    rng = np.random.Generator(np.random.PCG64(78))
    users = np.arange(matrix.shape[0], dtype=np.int64)
    tests = np.array([rng.choice(np.setdiff1d(np.arange(matrix.shape[1]),
                                              matrix.indices[matrix.indptr[u]:matrix.indptr[u + 1]])) for u in users])
    return users, tests.astype(np.int64)


def graph_digest(matrix: csr_matrix) -> str:
    return digest(matrix.indptr.astype(np.int64), matrix.indices.astype(np.int32), matrix.data.astype(np.float64))


def params_digest(params: dict[str, torch.Tensor]) -> str:
    return digest(*[params[f"{k}.{w}"].detach().numpy() for k in KEYS for w in ("weight", "bias")])


def trajectory(params: dict[str, torch.Tensor], matrix: csr_matrix, orders, dtype, snapshots=FIX_EPOCHS):
    """The restatement run over the given epoch orders with draws(): -> (per-step total losses, {epochs: scores of
    every user [n_users, N]})."""
    model = Model(params, dtype)
    X = np.asarray(matrix.todense(), dtype=np.float32)
    losses, scores, step = [], {}, 0
    for ep, order in enumerate(orders):
        for s in range(0, len(order), BATCH):
            rows = np.asarray(order[s:s + BATCH])
            (total, _, _), _ = model.step(X[rows], *draws(step, len(rows), matrix.shape[1]))
            losses.append(total)
            step += 1
        if ep + 1 in snapshots:
            scores[ep + 1] = model.scores(X)
    return np.array(losses), scores


def bracket(scores: np.ndarray, cand_mask: np.ndarray, tests: np.ndarray, bar: float):
    """Per row the smallest and the largest 0-based rank the test item can take among the row's candidates when
    every score is known to within bar: [#certainly greater, #possibly greater or equal]."""
    st = scores[np.arange(len(tests)), tests][:, None]
    others = cand_mask.copy()
    others[np.arange(len(tests)), tests] = False
    return ((scores > st + 2 * bar) & others).sum(1), ((scores >= st - 2 * bar) & others).sum(1)
