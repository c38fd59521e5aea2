"""G12: t-SNE / PCA fixture from scikit-learn, the library the reference's plot_latent_space calls
(src/ml/visualize.py:226-234).

Run in the build container (where scikit-learn exists; about a minute):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tsne_fixture.py

Three small clustered float32 inputs (tests/tsne_ref.py CASES): 300 x 16, 120 x 5 at perplexity 10, and 193 x 33 with
three exactly duplicated rows. Per case <c>, scikit-learn is observed, outputs only:
  _X                     the input (float32)
  _P_ptr, _P_col, _P_val sklearn.manifold._t_sne._joint_probabilities_nn on its own kNN graph (squared distances)
  _Y                     a recorded non-trivial embedding (float32): the PCA init after 60 restated iterations
  _grad, _error          sklearn.manifold._barnes_hut_tsne.gradient(..., angle=0.0, compute_error=True) at _Y with P,
                         times 4 (the routine leaves the factor to its caller)
  _pca, _evr             PCA(n_components=2).fit_transform(X) and explained_variance_ratio_
  _kl                    kl_divergence_ of TSNE(n_components=2, perplexity=p, max_iter=1000, random_state=42) at
                         angle = 0.5 and angle = 0.0, and of the float64 restatement's full run
meta: versions, seeds, and
  noise[<c>_<what>]  = |restatement - scikit-learn| (P, grad, error, pca, evr): fp32 storage on scikit-learn's side;
  bar                = 16 * noise, the bar of the CPU test and of the GPU test's comparison with these arrays;
  trajectory_noise   = the restatement's 30 iterations against the same with every sum reversed (relative to max |Y|),
  trajectory_bar     = 16 * that;
  kl_spread[<c>]     = max - min of the three recorded KL values: the GPU full run must land within twice that of
                       scikit-learn's angle = 0.5 value.
The generator asserts, drawing another seed if one fails: in every row the relative gap between the k-th and the
(k + 1)-th neighbour distance is at least 1e-5 (two orders above fp32 distance rounding: the neighbour set is the
same from fp32 and from fp64 distances); no duplicate sits at that boundary; no step of the restatement's perplexity
search has |H - log perplexity| within 1e-9 of the 1e-5 threshold (the stopping step is the same in numpy and on the
device).
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent)]
import tsne_ref as TR  # noqa: E402

TRAJECTORY_CASE, TRAJECTORY_ITERS, RECORD_ITERS = "c300", 30, 60


def conditions(X, perplexity) -> str | None:
    n = len(X)
    k = TR.neighbour_count(n, perplexity)
    D = TR.sq_distances(X)
    srt = np.sort(D, axis=1)
    if k < n - 1:
        gap = (srt[:, k] - srt[:, k - 1]) / srt[:, k]
        if gap.min() < 1e-5:
            return f"neighbour gap {gap.min():.2e}"
        if (srt[:, k] == srt[:, k - 1]).any():
            return "a duplicate at the k / k + 1 boundary"
    trace = []
    TR.conditional_p(TR.neighbours(X, k, D)[1], perplexity, trace=trace)
    if np.abs(np.array(trace) - TR.PERPLEXITY_TOL).min() < 1e-9:
        return "a perplexity step on the threshold"
    return None


def sklearn_p(X, perplexity):
    from sklearn.manifold._t_sne import _joint_probabilities_nn
    from sklearn.neighbors import NearestNeighbors
    k = TR.neighbour_count(len(X), perplexity)
    knn = NearestNeighbors(algorithm="auto", n_neighbors=k, metric="euclidean").fit(X)
    g = knn.kneighbors_graph(mode="distance")
    g.data **= 2
    P = _joint_probabilities_nn(g, perplexity, 0)
    P.sort_indices()
    return P


def sklearn_gradient(P, Y32):
    from sklearn.manifold import _barnes_hut_tsne
    grad = np.zeros(Y32.shape, np.float32)
    err = _barnes_hut_tsne.gradient(P.data.astype(np.float32), Y32, P.indices.astype(np.int64),
                                    P.indptr.astype(np.int64), grad, 0.0, 2, 0, dof=1, compute_error=True,
                                    num_threads=1)
    return 4.0 * grad.astype(np.float64), float(err)


def main():
    import sklearn
    from sklearn.decomposition import PCA
    from sklearn.manifold import TSNE
    out = {}
    meta = {"sklearn": sklearn.__version__, "numpy": np.__version__, "bar_factor": TR.BAR_FACTOR, "seed": {},
            "noise": {}, "bar": {}, "kl": {}, "kl_spread": {}, "n_iter": {}}
    for case, (n, L, perplexity) in TR.CASES.items():
        seed = 100
        while True:
            X = TR.clustered(n, L, seed, dup=int(case == "dup"))
            why = conditions(X, perplexity)
            if why is None:
                break
            print(f"{case}: seed {seed} refused ({why})")
            seed += 1
        meta["seed"][case] = seed
        out[f"{case}_X"] = X
        mine = TR.fit(X, perplexity)
        # P
        P = sklearn_p(X, perplexity)
        out[f"{case}_P_ptr"], out[f"{case}_P_col"] = P.indptr.astype(np.int64), P.indices.astype(np.int32)
        out[f"{case}_P_val"] = P.data.astype(np.float64)
        noise = {"P": float(np.abs(P.toarray() - mine["P"]).max())}
        assert (P.toarray() != 0).sum() == (mine["P"] != 0).sum() or case == "dup"
        # one gradient and error at a recorded embedding
        state = TR.new_state(mine["init"])
        TR.descend(state, mine["P"], 0, RECORD_ITERS, 0.5, TR.EARLY_EXAGGERATION, 250, TR.learning_rate(n))
        Y32 = state["Y"].astype(np.float32)
        grad, err = sklearn_gradient(P, Y32)
        out[f"{case}_Y"], out[f"{case}_grad"], out[f"{case}_error"] = Y32, grad, np.array(err)
        s = TR.step(Y32.astype(np.float64), np.ones((n, 2)), np.zeros((n, 2)), P.toarray().astype(np.float64), 1.0,
                    0.5, 1.0)
        noise["grad"] = float(np.abs(s["grad"] - grad).max())
        noise["error"] = abs(s["error"] - err)
        # PCA
        pca = PCA(n_components=2)
        proj = pca.fit_transform(X)
        out[f"{case}_pca"] = proj.astype(np.float64)
        out[f"{case}_evr"] = pca.explained_variance_ratio_.astype(np.float64)
        noise["pca"] = float(np.abs(proj - mine["pca"]).max())
        noise["evr"] = float(np.abs(pca.explained_variance_ratio_ - mine["explained_variance_ratio"]).max())
        for what, v in noise.items():
            assert v > 0, (case, what)
            meta["noise"][f"{case}_{what}"] = v
            meta["bar"][f"{case}_{what}"] = TR.BAR_FACTOR * v
        # the full runs
        kl = {}
        for angle in (0.5, 0.0):
            t = TSNE(n_components=2, perplexity=perplexity, max_iter=1000, random_state=42, angle=angle).fit(X)
            kl[f"sklearn_{angle}"] = float(t.kl_divergence_)
            meta["n_iter"][f"{case}_sklearn_{angle}"] = int(t.n_iter_)
        kl["restatement"] = float(mine["kl_divergence"])
        meta["n_iter"][f"{case}_restatement"] = int(mine["n_iter"])
        out[f"{case}_kl"] = np.array([kl["sklearn_0.5"], kl["sklearn_0.0"], kl["restatement"]])
        meta["kl"][case] = kl
        meta["kl_spread"][case] = max(kl.values()) - min(kl.values())
        print(case, "seed", seed, "noise", noise, "kl", kl)
        if case == TRAJECTORY_CASE:
            runs = []
            for reverse in (False, True):
                P_r = TR.joint_p(mine["idx"], TR.conditional_p(mine["d2"], perplexity, reverse), reverse)
                st = TR.new_state(TR.tsne_init(TR.pca2(X, reverse)[0]))
                TR.descend(st, P_r, 0, TRAJECTORY_ITERS, 0.5, TR.EARLY_EXAGGERATION, 250, TR.learning_rate(n), reverse)
                runs.append(st["Y"])
            tn = float(np.abs(runs[0] - runs[1]).max() / np.abs(runs[0]).max())
            assert tn > 0
            meta["trajectory_case"], meta["trajectory_iters"] = case, TRAJECTORY_ITERS
            meta["trajectory_noise"], meta["trajectory_bar"] = tn, TR.BAR_FACTOR * tn
            print("trajectory noise", tn)
    np.savez_compressed(HERE / "tsne.npz", **out)
    (HERE / "tsne_meta.json").write_text(json.dumps(meta, indent=1))
    size = (HERE / "tsne.npz").stat().st_size
    print("tsne.npz", size, "bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
