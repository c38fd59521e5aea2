"""LightGCN train-step time on MI355X: the libhvae step (src/ml/lightgcn.py TrainSteps: forward Horner chain, BPR,
backward chain, dense Adam) against a torch restatement of the reference's step (torch.sparse.mm + autograd +
torch.optim.Adam, src/ml/baseline.py:343-370 of the reference) on the same GPU, on the All_Beauty-shaped planted
set (tests/golden/gen.py PLANTED_CONFIG: 22,363 users x 12,101 items).

    python scripts/bench_lightgcn.py [--steps 200] [--warmup 20] [--embedding-dim 64] [--n-layers 3]

Both run the same first batches of one epoch from the same initial table; one JSON line with ms per step and
steps/s of each and the ratio. The torch side's index tensors are on the device before the clock starts, so it is
spared the reference's three host-to-device copies per step.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "recommendation-system_amd"), str(ROOT / "tests" / "golden")]

import torch  # noqa: E402


def timed(fn, steps: int, warmup: int) -> float:
    """ms per call of fn(k), k = 0, 1, ..., after `warmup` calls."""
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k in range(warmup, warmup + steps):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--embedding-dim", type=int, default=64)
    ap.add_argument("--n-layers", type=int, default=3)
    args = ap.parse_args()
    import pandas as pd
    from scipy.sparse import csr_matrix
    from gen import PLANTED_CONFIG, synth_planted
    from hvae import ops
    import src.ml.lightgcn as lg

    dev = torch.device("cuda", 0)
    tr, va, _, _, uid, iid = synth_planted(**PLANTED_CONFIG)
    both = pd.concat([tr, va])
    matrix = csr_matrix((np.ones(len(both)), (both["user_id"].str[1:].astype(np.int64).values,
                                              both["asin"].str[1:].astype(np.int64).values)),
                        shape=(len(uid), len(iid)))
    n_users, n_items = matrix.shape
    d, L, lr, reg = args.embedding_dim, args.n_layers, 1e-3, 1e-4
    torch.manual_seed(0)
    np.random.seed(0)
    table = lg.init_table(n_users, n_items, d)
    pu, pi = matrix.nonzero()
    users, pos, neg = lg.epoch_batches(pu, pi, n_items)
    n_batches = (len(users) + lg.BATCH_SIZE - 1) // lg.BATCH_SIZE - 1  # full batches only

    graph = ops.lgcn_graph_from_scipy(matrix, dev)
    steps = lg.TrainSteps(graph, table.to(dev), L, lr, reg)
    steps.load_epoch(users, pos, neg)
    hip_ms = timed(lambda k: steps.run(k % n_batches), args.steps, args.warmup)

    # the reference's step, restated on the device
    s = matrix.tocoo()
    deg = np.concatenate([np.asarray((matrix != 0).sum(axis=1)).ravel(), np.asarray((matrix != 0).sum(axis=0)).ravel()])
    scale = np.where(deg > 0, np.power(np.maximum(deg, 1), -0.5), 0.0)
    r = np.concatenate([s.row, s.col + n_users])
    c = np.concatenate([s.col + n_users, s.row])
    adj = torch.sparse_coo_tensor(torch.tensor(np.stack([r, c])), torch.tensor(scale[r] * scale[c], dtype=torch.float32),
                                  (n_users + n_items,) * 2).coalesce().to(dev)
    p = torch.nn.Parameter(table.to(dev).clone())
    opt = torch.optim.Adam([p], lr=lr)
    ud, pd_, nd = (torch.as_tensor(a.astype(np.int64), device=dev) for a in (users, pos, neg))

    def torch_step(k):
        b = (k % n_batches) * lg.BATCH_SIZE
        bu, bp, bn = ud[b:b + lg.BATCH_SIZE], pd_[b:b + lg.BATCH_SIZE], nd[b:b + lg.BATCH_SIZE]
        opt.zero_grad()
        layers = [p]
        for _ in range(L):
            layers.append(torch.sparse.mm(adj, layers[-1]))
        f = torch.stack(layers, dim=1).mean(dim=1)
        u_, p_, n_ = f[bu], f[n_users + bp], f[n_users + bn]
        loss = -torch.nn.functional.logsigmoid((u_ * p_).sum(1) - (u_ * n_).sum(1)).mean() \
            + reg * (u_.norm(2).pow(2) + p_.norm(2).pow(2) + n_.norm(2).pow(2)) / len(bu)
        loss.backward()
        opt.step()

    torch_ms = timed(torch_step, args.steps, args.warmup)
    drift = float((steps.E - p.detach()).abs().max())
    print(json.dumps({"bench": "lightgcn_step", "shape": [n_users, n_items], "nnz": int(graph.nnz), "d": d,
                      "n_layers": L, "batch": lg.BATCH_SIZE, "steps": args.steps, "warmup": args.warmup,
                      "hip_ms_per_step": round(hip_ms, 4), "hip_steps_per_s": round(1e3 / hip_ms, 1),
                      "torch_ms_per_step": round(torch_ms, 4), "torch_steps_per_s": round(1e3 / torch_ms, 1),
                      "torch_over_hip": round(torch_ms / hip_ms, 2), "max_table_diff_after": drift}), flush=True)


if __name__ == "__main__":
    main()
