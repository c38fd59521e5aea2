"""Mult-VAE train-step time on MI355X: the libhvae step (src/ml/multvae.py TrainSteps) against a torch restatement of
the reference's step (dense input rows, autograd, torch.optim.Adam, src/ml/baseline.py:208-218 of the reference) on
the same GPU, on the All_Beauty-shaped planted set (tests/golden/gen.py PLANTED_CONFIG: 22,363 users x 12,101 items,
batches of 512, hidden 600, latent 200).

    python scripts/bench_multvae.py [--steps 1000] [--warmup 50] [--probe-steps 10]

Both run the same full batches of one epoch from the same initial parameters, each with its own device-side dropout
and eps streams. The torch side's dense matrix is on the device before the clock starts, so it is spared the
reference's host-to-device copy of every batch. One JSON line: ms per step of each, the ratio, and per kernel the
mean time per launch and the launches per step (hvae_probe_*, one kernel name armed per pass of --probe-steps steps,
in passes of their own after the timed run).
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "recommendation-system_amd"), str(ROOT / "tests" / "golden")]

import torch  # noqa: E402

PROBES = ("mvae_encoder_fwd", "mvae_tanh_drop_fwd", "mvae_tanh_drop_bwd", "mvae_nll", "gemm", "rowgrad_apply",
          "adam_rows", "adam_dense")


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


def probe(name: str, fn, steps: int):
    """(mean us per launch, launches per step) of the kernel `name` over `steps` calls of fn."""
    from hvae import _lib
    L = _lib.lib()
    _lib.check(L.hvae_probe_arm(name.encode(), 64 * steps), "hvae_probe_arm")
    for k in range(steps):
        fn(k)
    torch.cuda.synchronize()
    us, n = C.c_double(), C.c_int()
    _lib.check(L.hvae_probe_collect(C.byref(us), C.byref(n)), "hvae_probe_collect")
    L.hvae_probe_arm(None, 0)
    return round(us.value, 2), round(n.value / steps, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--probe-steps", type=int, default=10)
    args = ap.parse_args()
    import pandas as pd
    import torch.nn.functional as F
    from scipy.sparse import csr_matrix
    from gen import PLANTED_CONFIG, synth_planted
    import src.ml.multvae as mv

    dev = torch.device("cuda", 0)
    tr, va, _, _, uid, iid = synth_planted(**PLANTED_CONFIG)
    both = pd.concat([tr, va])
    matrix = csr_matrix((np.ones(len(both)), (both["user_id"].str[1:].astype(np.int64).values,
                                              both["asin"].str[1:].astype(np.int64).values)),
                        shape=(len(uid), len(iid)))
    matrix.sum_duplicates()
    n_users, n_items = matrix.shape
    H, L, lr, beta, p = 600, 200, 1e-3, 0.2, mv.DROPOUT
    torch.manual_seed(0)
    params = mv.init_params(n_items, H, L)
    order = mv.epoch_order(n_users)
    n_batches = n_users // mv.BATCH_SIZE  # full batches only

    steps = mv.TrainSteps(matrix, params, dev, lr, beta, seed=0)
    steps.load_epoch(order)
    hip_ms = timed(lambda k: steps.run(k % n_batches), args.steps, args.warmup)
    hip_loss = float(steps.loss3[0])
    kernels = {name: dict(zip(("us_per_launch", "launches_per_step"),
                              probe(name, lambda k: steps.run(k % n_batches), args.probe_steps))) for name in PROBES}

    # the reference's step, restated on the device
    P = {k: torch.nn.Parameter(v.to(dev).clone()) for k, v in params.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr)
    Xd = torch.as_tensor(matrix.toarray(), dtype=torch.float32).to(dev)
    od = torch.as_tensor(order.astype(np.int64), device=dev)
    last = {}

    def lin(x, k):
        return F.linear(x, P[f"{k}.weight"], P[f"{k}.bias"])

    def torch_step(k):
        b = (k % n_batches) * mv.BATCH_SIZE
        x = Xd[od[b:b + mv.BATCH_SIZE]]
        opt.zero_grad()
        h = F.dropout(F.normalize(x, p=2, dim=1), p)
        h = F.dropout(torch.tanh(lin(h, "encoder.0")), p)
        h = F.dropout(torch.tanh(lin(h, "encoder.3")), p)
        mu, lv = lin(h, "mu_layer"), lin(h, "logvar_layer")
        std = torch.exp(0.5 * lv)
        z = mu + std * torch.randn_like(std)
        s = lin(torch.tanh(lin(z, "decoder.0")), "decoder.2")
        loss = -torch.mean(torch.sum(F.log_softmax(s, dim=1) * x, dim=1)) \
            + beta * (-0.5 * torch.mean(torch.sum(1 + lv - mu.pow(2) - lv.exp(), dim=1)))
        loss.backward()
        opt.step()
        last["loss"] = loss.detach()

    torch_ms = timed(torch_step, args.steps, args.warmup)
    new = sum(kernels[k]["us_per_launch"] * kernels[k]["launches_per_step"] for k in PROBES if k.startswith("mvae_"))
    print(json.dumps({"bench": "multvae_step", "shape": [n_users, n_items], "nnz": int(matrix.nnz), "hidden": H,
                      "latent": L, "batch": mv.BATCH_SIZE, "steps": args.steps, "warmup": args.warmup,
                      "hip_ms_per_step": round(hip_ms, 4), "hip_steps_per_s": round(1e3 / hip_ms, 1),
                      "torch_ms_per_step": round(torch_ms, 4), "torch_steps_per_s": round(1e3 / torch_ms, 1),
                      "torch_over_hip": round(torch_ms / hip_ms, 2), "hip_last_loss": round(hip_loss, 4),
                      "torch_last_loss": round(float(last["loss"]), 4), "kernels": kernels,
                      "new_kernels_us_per_step": round(new, 1)}), flush=True)


if __name__ == "__main__":
    main()
