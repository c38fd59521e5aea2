"""Baseline evaluation throughput on MI355X (users/s): Popularity and Item-KNN (src/ml/baseline.py) under the
99-negative and the full-ranking protocol, on the All_Beauty-shaped planted set (tests/golden/gen.py
PLANTED_CONFIG: 22,363 users x 12,101 items, so Item-KNN takes the reference's on-the-fly path above 10,000 items).

    python scripts/bench_baselines.py [--users N] [--reps 3]

One JSON line per model and protocol: the whole evaluate_model work for the test rows (host-side negative sampling
included, as in the reference's loop), best of --reps, plus the fit time and, for the 99-negative protocol, the
share of the host sampler. The reference's own loop is timed on the CPU by tests/golden/time_reference_baseline.py.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=0, help="test rows to evaluate (0 = all)")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import pandas as pd
    from scipy.sparse import csr_matrix
    from gen import PLANTED_CONFIG, synth_planted
    from hvae import ops
    import src.ml.baseline as b

    dev = torch.device("cuda", 0)
    tr, va, te, _, uid, iid = synth_planted(**PLANTED_CONFIG)
    both = pd.concat([tr, va])
    matrix = csr_matrix((np.ones(len(both)), (both["user_id"].str[1:].astype(np.int64).values,
                                              both["asin"].str[1:].astype(np.int64).values)),
                        shape=(len(uid), len(iid)))
    users = te["user_id"].str[1:].astype(np.int64).values
    tests = te["asin"].str[1:].astype(np.int64).values
    if args.users:
        users, tests = users[:args.users], tests[:args.users]
    ks = [5, 10, 20]
    for name in b.SERVED_MODELS:
        model = b.BASELINES[name]()
        model.fit(matrix)  # warm-up: library load, allocator
        torch.cuda.synchronize()
        t = time.perf_counter()
        model.fit(matrix)
        torch.cuda.synchronize()
        fit_s = time.perf_counter() - t
        for n_neg in (99, None):
            np.random.seed(0)
            b.evaluate_ranks(model, matrix, users[:256], tests[:256], ks, n_neg)  # warm-up
            torch.cuda.synchronize()
            best, neg_s = float("inf"), None
            for _ in range(args.reps):
                np.random.seed(0)
                t = time.perf_counter()
                rank = b.evaluate_ranks(model, matrix, users, tests, ks, n_neg)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t)
            if n_neg:
                np.random.seed(0)
                t = time.perf_counter()
                ops.negatives_legacy(matrix.indptr, matrix.indices, matrix.shape[1], users, tests, n_neg, arrays=True)
                neg_s = round(time.perf_counter() - t, 4)
            print(json.dumps({"model": name, "protocol": "neg99" if n_neg else "full", "users": len(users),
                              "shape": list(matrix.shape), "batch": model.max_batch, "fit_s": round(fit_s, 4),
                              "s": round(best, 4), "users_per_s": round(len(users) / best, 1),
                              "host_sampler_s": neg_s, "hit_ratio@10": round(float((rank < 10).mean()), 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
