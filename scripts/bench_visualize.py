"""Latent-space projection time on MI355X: src/ml/visualize.py's latent_projections (the sparse encoder, exact PCA,
libhvae's fp64 t-SNE kernels) stage by stage at n = 2000 sampled users and L = 128 on a planted model, and, where
scikit-learn is importable, the reference's PCA + TSNE calls (src/ml/visualize.py:226-234 of the reference) on the same
mu on the host cores this process is given.

    python scripts/bench_visualize.py [--n 2000] [--latent 128] [--fits 3] [--warmup 1] [--no-sklearn]

One JSON line: ms per stage (encode, kNN + P with its host symmetrisation, PCA, the 1000 iterations), their sum, the
KL divergence reached, and scikit-learn's times and KL divergence. The model is untrained (planted data, seeded
weights): the timings do not depend on what the latents mean.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "recommendation-system_amd"), str(ROOT / "tests" / "golden")]

import torch  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--fits", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    import pandas as pd
    from scipy.sparse import csr_matrix
    from gen import PLANTED_CONFIG, synth_planted
    import src.ml.visualize as v
    from src.ml.model import HybridVAE

    dev = torch.device("cuda", 0)
    tr, va, _, E, uid, iid = synth_planted(**PLANTED_CONFIG)
    both = pd.concat([tr, va])
    matrix = csr_matrix((np.ones(len(both)), (both["user_id"].str[1:].astype(np.int64).values,
                                              both["asin"].str[1:].astype(np.int64).values)),
                        shape=(len(uid), len(iid)))
    matrix.sum_duplicates()
    torch.manual_seed(0)
    model = HybridVAE(len(iid), E, latent_dim=args.latent, hidden_dims=[512], dropout=0.3, beta=0.2).to(dev).eval()
    indices = v.sample_users(matrix.shape[0], args.n, seed=0)
    stages = {"encode": [], "pca": [], "knn_p": [], "iterations": []}
    kl = it = mu = None
    for rep in range(args.warmup + args.fits):
        mu, t_enc = clock(lambda: v.encode_users(model, matrix, indices))
        (proj, evr), t_pca = clock(lambda: v.pca_2d(mu))
        P, t_p = clock(lambda: v.tsne_joint_p(mu, 30.0))
        init = v.tsne_init(proj.cpu().numpy())
        (Y, kl, it), t_it = clock(lambda: v.tsne_embed(P, init, 1000))
        if rep >= args.warmup:
            for name, t in zip(stages, (t_enc, t_pca, t_p, t_it)):
                stages[name].append(t)
    row = {"bench": "tsne_fit", "n": int(len(indices)), "latent": args.latent, "n_items": int(matrix.shape[1]),
           "perplexity": 30.0, "max_iter": 1000, "fits": args.fits, "warmup": args.warmup,
           "hip_ms": {k: round(float(np.median(t)), 3) for k, t in stages.items()}, "n_iter": it,
           "kl_divergence": round(kl, 6), "p_nnz": int(P.val.numel())}
    row["hip_ms_total"] = round(sum(row["hip_ms"].values()), 3)
    if not args.no_sklearn:
        try:
            from sklearn.decomposition import PCA
            from sklearn.manifold import TSNE
        except ImportError:
            PCA = None
        if PCA is not None:
            import sklearn
            x = mu.cpu().numpy()
            t = time.perf_counter()
            PCA(n_components=2).fit_transform(x)
            t_pca = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            ts = TSNE(n_components=2, perplexity=30, max_iter=1000, random_state=42).fit(x)
            t_tsne = (time.perf_counter() - t) * 1e3
            row["sklearn"] = {"version": sklearn.__version__, "host_threads": len(os.sched_getaffinity(0)),
                              "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "pca_ms": round(t_pca, 1),
                              "tsne_ms": round(t_tsne, 1), "kl_divergence": round(float(ts.kl_divergence_), 6),
                              "n_iter": int(ts.n_iter_)}
            hip = row["hip_ms"]["pca"] + row["hip_ms"]["knn_p"] + row["hip_ms"]["iterations"]
            row["sklearn_over_hip_pca_tsne"] = round((t_pca + t_tsne) / hip, 2)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
