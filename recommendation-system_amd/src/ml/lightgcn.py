"""LightGCN baseline on MI355X -- the reference's LightGCNRecommender (src/ml/baseline.py:239-385), trained and
evaluated on the device (`make baseline-lightgcn`).

The reference repeats the full 3-layer propagation, forward and backward, for every batch of 1024 interactions:
six torch.sparse.mm products per step. Here a step is launches of libhvae only (csrc/hvae_lgcn.hip): the forward
Horner chain F = 1/4 (E + A(E + A(E + A E))) (hvae_lgcn_propagate, three launches), the BPR loss and its gradient
with respect to F (hvae_lgcn_bpr), the same chain over the gradient (the adjacency is symmetric), and one
hvae_adam_dense over the whole [n_users + n_items, d] table. The step loop never synchronises with the host: an
epoch's indices and summation plans go to the device once, and the summed loss is read only at the epochs the
reference logs.

fit() reproduces the reference's run draw for draw: the initial embeddings from torch's CPU generator in the
reference's order (the two nn.Embedding constructors, then the two normal_(std=0.1) calls), one
np.random.permutation per epoch and one np.random.randint per batch from numpy's global stream, which is left
where the reference leaves it. Scoring, ranking, ties and negatives are src/ml/baseline.py's (evaluate_model),
unchanged; main() sets the "LightGCN" entry of models/figures/baseline_results.json beside the entries
`make baseline` wrote.
"""
from __future__ import annotations

import logging

import numpy as np
import torch
from scipy.sparse import csr_matrix

from hvae import ops

from .baseline import BaseRecommender, _resolve_device, parse_args, run_baseline

logger = logging.getLogger(__name__)

NAME = "LightGCN"
SERVED_DIMS = ops.LGCN_DIMS
SERVED_LAYERS = (1, 8)
BATCH_SIZE = 1024  # the reference's (baseline.py:341); hvae_lgcn_bpr's largest batch


def init_table(n_users: int, n_items: int, embedding_dim: int) -> torch.Tensor:
    """The initial [n_users + n_items, d] table from torch's CPU generator, draw for draw LightGCNModel.__init__
    (baseline.py:248-251): both nn.Embedding constructors draw N(0, 1) weights, then both are redrawn with
    std = 0.1."""
    user = torch.nn.Embedding(n_users, embedding_dim)
    item = torch.nn.Embedding(n_items, embedding_dim)
    torch.nn.init.normal_(user.weight, std=0.1)
    torch.nn.init.normal_(item.weight, std=0.1)
    return torch.cat([user.weight.detach(), item.weight.detach()], dim=0).contiguous()


def epoch_batches(pos_users: np.ndarray, pos_items: np.ndarray, n_items: int, batch_size: int = BATCH_SIZE):
    """One epoch's (users, pos, neg) int32 [n_interactions] from numpy's global stream, as the reference draws
    them (baseline.py:336-349): one permutation, then one randint(0, n_items, size) per batch. Batch k is
    [k * batch_size, (k + 1) * batch_size) of each."""
    n = len(pos_users)
    perm = np.random.permutation(n)
    neg = np.empty(n, np.int64)
    for start in range(0, n, batch_size):
        end = min(start + batch_size, n)
        neg[start:end] = np.random.randint(0, n_items, end - start)
    return pos_users[perm].astype(np.int32), pos_items[perm].astype(np.int32), neg.astype(np.int32)


def epoch_plan(users: np.ndarray, pos: np.ndarray, neg: np.ndarray, n_users: int, n_items: int,
               batch_size: int = BATCH_SIZE):
    """ops.lgcn_bpr_plan of every batch of an epoch in one sort: (slots int32 [3 n], seg_off int32, seg_base,
    n_seg). Batch k's slots are slots[3 k batch_size : ...] and its group bounds seg_off[seg_base[k] :
    seg_base[k] + n_seg[k] + 1]."""
    n = len(users)
    n_nodes = n_users + n_items
    i = np.arange(n, dtype=np.int64)
    bat = i // batch_size
    b = i - bat * batch_size
    nb = np.minimum(batch_size, n - bat * batch_size)
    node = np.concatenate([users.astype(np.int64), pos.astype(np.int64) + n_users, neg.astype(np.int64) + n_users])
    bat3 = np.concatenate([bat, bat, bat])
    slot = np.concatenate([b, nb + b, 2 * nb + b])
    key = bat3 * n_nodes + node
    order = np.lexsort((slot, key))
    key, bat3 = key[order], bat3[order]
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    n_batches = (n + batch_size - 1) // batch_size
    n_seg = np.bincount(bat3[starts], minlength=n_batches).astype(np.int64)
    seg_base = np.concatenate([[0], np.cumsum(n_seg + 1)[:-1]]).astype(np.int64)
    seg_off = np.empty(int((n_seg + 1).sum()), np.int64)
    first = np.concatenate([[0], np.cumsum(n_seg)[:-1]])  # index into starts of each batch's first group
    sb = bat3[starts]
    seg_off[seg_base[sb] + np.arange(len(starts)) - first[sb]] = starts - 3 * batch_size * sb
    k = np.arange(n_batches)
    seg_off[seg_base + n_seg] = 3 * np.minimum(batch_size, n - k * batch_size)
    return slot[order].astype(np.int32), seg_off.astype(np.int32), seg_base, n_seg


class TrainSteps:
    """The device state of a LightGCN training run and its step: forward chain, BPR, backward chain, Adam. Nothing
    in run() waits for the device."""

    def __init__(self, graph: "ops.LgcnGraph", table: torch.Tensor, n_layers: int, lr: float, reg: float):
        self.graph, self.n_layers, self.reg = graph, n_layers, reg
        self.E = E = table.contiguous()
        self.m, self.v = torch.zeros_like(E), torch.zeros_like(E)
        self.F, self.g, self.dE, self.ta, self.tb = (torch.empty_like(E) for _ in range(5))
        self.step = torch.zeros(1, dtype=torch.int64, device=E.device)
        self.adam = ops.adam_config(lr, (0.9, 0.999), 1e-8, 0.0, self.step)  # torch.optim.Adam's defaults (:326)
        self.total = torch.zeros(1, dtype=torch.float64, device=E.device)    # the epoch's summed loss
        self.n_batches = 0

    def load_epoch(self, users: np.ndarray, pos: np.ndarray, neg: np.ndarray) -> None:
        """One epoch's triples and their summation plans to the device; clears the summed loss."""
        g = self.graph
        self.n, self.n_batches = len(users), (len(users) + BATCH_SIZE - 1) // BATCH_SIZE
        self.total.zero_()
        if self.n == 0:
            return
        slots, seg_off, self.seg_base, self.n_seg = epoch_plan(users, pos, neg, g.n_users, g.n_items)
        self.users, self.pos, self.neg, self.slots, self.seg_off = (
            torch.as_tensor(a, device=self.E.device) for a in (users, pos, neg, slots, seg_off))

    def forward(self) -> torch.Tensor:
        return ops.lgcn_chain(self.graph, self.E, self.n_layers, self.F, self.ta, self.tb)

    def run(self, k: int) -> None:
        s, e = k * BATCH_SIZE, min((k + 1) * BATCH_SIZE, self.n)
        self.forward()
        ops.lgcn_bpr(self.F, self.graph.n_users, self.users[s:e], self.pos[s:e], self.neg[s:e], self.reg, g=self.g,
                     loss_accum=self.total, plan=(self.slots[3 * s:3 * e], self.seg_off[int(self.seg_base[k]):]),
                     n_seg=int(self.n_seg[k]))
        ops.lgcn_chain(self.graph, self.g, self.n_layers, self.dE, self.ta, self.tb)
        ops.adam_dense(self.adam, self.E, self.m, self.v, self.dE)
        ops.counter_add(self.step)


class LightGCNRecommender(BaseRecommender):
    """The reference's LightGCNRecommender (baseline.py:269-385) with its attributes (user_final_emb,
    item_final_emb, fit, predict) plus the batched device scoring that baseline.evaluate_model uses."""

    def __init__(self, embedding_dim: int = 64, n_layers: int = 3, epochs: int = 50, lr: float = 1e-3,
                 reg: float = 1e-4, device=None):
        if embedding_dim not in SERVED_DIMS:
            raise ValueError(f"LightGCN: embedding_dim {embedding_dim} is not served; served: {SERVED_DIMS[0]} and "
                             f"{SERVED_DIMS[1]}")
        if not SERVED_LAYERS[0] <= n_layers <= SERVED_LAYERS[1]:
            raise ValueError(f"LightGCN: n_layers {n_layers} is not served; served: {SERVED_LAYERS[0]} to "
                             f"{SERVED_LAYERS[1]}")
        self.embedding_dim = embedding_dim
        self.n_layers = n_layers
        self.epochs = epochs
        self.lr = lr
        self.reg = reg
        self._device_arg = device
        self.user_final_emb: torch.Tensor | None = None
        self.item_final_emb: torch.Tensor | None = None
        self.ego: torch.Tensor | None = None     # the trained [n_users + n_items, d] table
        self.epoch_losses: list[float] = []      # the summed loss of every 10th epoch, as the reference logs it

    def fit(self, interaction_matrix: csr_matrix) -> None:
        logger.info(f"Fitting LightGCN (dim={self.embedding_dim}, layers={self.n_layers})...")
        n_users, n_items = interaction_matrix.shape
        self.n_users, self.n_items = n_users, n_items
        table = init_table(n_users, n_items, self.embedding_dim)
        self.device = dev = _resolve_device(self._device_arg)
        graph = ops.lgcn_graph_from_scipy(interaction_matrix, dev)
        pos_users, pos_items = interaction_matrix.nonzero()
        steps = TrainSteps(graph, table.to(dev), self.n_layers, self.lr, self.reg)
        self.epoch_losses = []
        for epoch in range(self.epochs):
            steps.load_epoch(*epoch_batches(pos_users, pos_items, n_items))
            for k in range(steps.n_batches):
                steps.run(k)
            if (epoch + 1) % 10 == 0:
                self.epoch_losses.append(float(steps.total.item()))
                logger.info(f"  Epoch {epoch + 1}/{self.epochs}, Loss: {self.epoch_losses[-1]:.4f}")
        F = steps.forward()
        self.ego = steps.E
        self.user_final_emb = F[:n_users]
        self.item_final_emb = F[n_users:]

    def predict(self, user_idx: int) -> np.ndarray:
        return self.score_all(np.array([user_idx]))[0].cpu().numpy()

    def score_candidates(self, users: np.ndarray, cand: torch.Tensor) -> torch.Tensor:
        rows = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=self.device)
        return ops.score_candidates(self.user_final_emb, rows, self.item_final_emb, cand.contiguous())

    def score_all(self, users: np.ndarray) -> torch.Tensor:
        rows = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int64), device=self.device)
        return ops.gemm(self.user_final_emb.index_select(0, rows), self.item_final_emb.t())


def run_lightgcn(data_dir: str, k_values: list[int] | None = None, n_negatives: int | None = 99,
                 embedding_dim: int = 64, n_layers: int = 3, epochs: int = 50, lr: float = 1e-3,
                 reg: float = 1e-4) -> dict:
    """Fit and evaluate LightGCN as the reference's run_all_baselines does for one model (baseline.py:474-533)."""
    model = LightGCNRecommender(embedding_dim, n_layers, epochs, lr, reg)
    return run_baseline(model, NAME, data_dir, k_values, n_negatives)


def _add_flags(parser) -> None:
    parser.add_argument("--epochs", type=int, default=50)
    parser.add_argument("--embedding-dim", type=int, default=64, help="served: 64, 128")
    parser.add_argument("--n-layers", type=int, default=3, help="served: 1 to 8")
    parser.add_argument("--lr", type=float, default=1e-3)
    parser.add_argument("--reg", type=float, default=1e-4)


def main() -> None:
    args = parse_args("Train and evaluate the LightGCN baseline (MI355X)", _add_flags)
    run_lightgcn(args.data, args.k_values, args.n_negatives, embedding_dim=args.embedding_dim, n_layers=args.n_layers,
                 epochs=args.epochs, lr=args.lr, reg=args.reg)


if __name__ == "__main__":
    main()
