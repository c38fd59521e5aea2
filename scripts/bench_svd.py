"""SVD baseline fit time on MI355X: SVDRecommender.fit (src/ml/svd.py: libhvae's fp64 spmm / Gram / Cholesky / apply
kernels, one host eigendecomposition) against a torch restatement of the same randomized SVD on the same GPU
(torch.sparse.mm in fp64 for the sparse products, torch.linalg.qr for every normaliser, torch.linalg.svd of B), on
the All_Beauty-shaped planted set (tests/golden/gen.py PLANTED_CONFIG: 22,363 users x 12,101 items).

    python scripts/bench_svd.py [--fits 20] [--warmup 3] [--n-components 50]

Both start from the same host sketch and include its draw, its upload and the upload of the matrix; one JSON line
with ms per fit of each and the ratio, the host sketch's own time and the ratio without it, and the largest difference
between the two runs' scores on a sample of users.
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


def timed(fn, fits: int, warmup: int) -> float:
    """ms per call of fn() after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(fits):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / fits


def torch_fit(matrix, k: int, dev):
    """The reference's randomized SVD restated with torch ops on the device: (user_factors, components)."""
    import src.ml.svd as svd
    n_users, n_items = matrix.shape
    W = k + svd.N_OVERSAMPLES
    coo = matrix.tocoo()
    A = torch.sparse_coo_tensor(torch.tensor(np.stack([coo.row, coo.col])), torch.tensor(coo.data, dtype=torch.float64),
                                coo.shape).coalesce().to(dev)
    At = A.t().coalesce()
    transposed = n_users < n_items
    M, Mt = (At, A) if transposed else (A, At)
    Q = torch.as_tensor(svd.sketch(M.shape[1], W)).to(dev)
    for _ in range(svd.N_ITER):
        Q, _ = torch.linalg.qr(torch.sparse.mm(M, Q))
        Q, _ = torch.linalg.qr(torch.sparse.mm(Mt, Q))
    Q, _ = torch.linalg.qr(torch.sparse.mm(M, Q))
    B = torch.sparse.mm(Mt, Q).t()
    Uh, s, Vt = torch.linalg.svd(B, full_matrices=False)
    comps = ((Q @ Uh).t() if transposed else Vt)[:k]
    big = comps.abs().argmax(dim=1, keepdim=True)
    comps = comps * torch.sign(comps.gather(1, big))
    return torch.sparse.mm(A, comps.t().contiguous()), comps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fits", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-components", type=int, default=50)
    args = ap.parse_args()
    import pandas as pd
    from scipy.sparse import csr_matrix
    from gen import PLANTED_CONFIG, synth_planted
    import src.ml.svd as svd

    dev = torch.device("cuda", 0)
    tr, va, _, _, uid, iid = synth_planted(**PLANTED_CONFIG)
    both = pd.concat([tr, va])
    matrix = csr_matrix((np.ones(len(both)), (both["user_id"].str[1:].astype(np.int64).values,
                                              both["asin"].str[1:].astype(np.int64).values)),
                        shape=(len(uid), len(iid)))
    matrix.sum_duplicates()
    k = args.n_components
    model = svd.SVDRecommender(n_components=k, device=dev)
    hip_ms = timed(lambda: model.fit(matrix), args.fits, args.warmup)
    ref = {}

    def run_torch():
        ref["uf"], ref["comps"] = torch_fit(matrix, k, dev)

    torch_ms = timed(run_torch, args.fits, args.warmup)
    t = time.perf_counter()
    for _ in range(args.fits):   # both sides draw the same host sketch inside the clock; its share, alone
        svd.sketch(min(matrix.shape), k + svd.N_OVERSAMPLES)
    sketch_ms = (time.perf_counter() - t) * 1e3 / args.fits
    rows = torch.arange(0, matrix.shape[0], max(1, matrix.shape[0] // 512), device=dev)
    diff = float((model.user_factors[rows] @ model.item_factors - ref["uf"][rows] @ ref["comps"]).abs().max())
    print(json.dumps({"bench": "svd_fit", "shape": list(matrix.shape), "nnz": int(matrix.nnz), "n_components": k,
                      "fits": args.fits, "warmup": args.warmup, "hip_ms_per_fit": round(hip_ms, 3),
                      "torch_ms_per_fit": round(torch_ms, 3), "torch_over_hip": round(torch_ms / hip_ms, 2),
                      "host_sketch_ms": round(sketch_ms, 3),
                      "torch_over_hip_without_sketch": round((torch_ms - sketch_ms) / (hip_ms - sketch_ms), 2),
                      "explained_variance_sum": round(float(model.explained_variance_ratio_.sum()), 6),
                      "max_score_diff_sampled": diff}), flush=True)


if __name__ == "__main__":
    main()
