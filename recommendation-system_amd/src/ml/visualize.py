"""`make visualize` on MI355X: the figures of the reference's src/ml/visualize.py from the files this project writes.

Reference: src/ml/visualize.py (subcommands training / baseline / tuning / all, the same arguments, function names,
signatures, output file names and dataset prefix; a missing input is logged and the function returns). Three of the
four figure families are matplotlib over JSON (training_history.json, figures/baseline_results.json,
grid_search_results.json). The fourth, plot_latent_space (:163-289), computes: it encodes a sample of users and
projects their latent means with scikit-learn's PCA and TSNE. Here that compute is `latent_projections`:

  encode   the sampled users' CSR rows, in place, through the sparse encoder (no dense [n, n_items] vectors);
  PCA      exact: centre in fp64, the L x L covariance on the device (the K19 Gram kernel up to 64 columns, a torch
           fp64 product above), numpy's eigh of that small matrix on the host, svd_flip's sign rule, the projection
           on the device. scikit-learn's "auto" solver turns randomized (an unseeded stream) when n < 10 L; this
           path never does;
  t-SNE    scikit-learn 1.7's TSNE(method="barnes_hut", init="pca", learning_rate="auto") in the K21 kernels
           (csrc/hvae_tsne.hip), with two deliberate differences: the exact O(n^2) repulsion instead of the
           Barnes-Hut tree (its angle = 0 limit), and fp64 where scikit-learn keeps the embedding, gradient, gains and
           update in fp32. The init is exact PCA (scikit-learn: randomized PCA with seed 42, the same subspace), so no
           random stream is involved and two fits are bitwise equal. The symmetrisation of P is the fit's one host
           step; the loop reads the error and the gradient norm back every 50th iteration and on the last one, and
           nothing else waits for the device.

matplotlib is imported inside the plotting functions only (Agg backend); nothing here imports scikit-learn.
Additive options: --n-samples (default 2000) and --seed (default none: the reference's np.random.choice on the global
stream; with a seed the sample comes from np.random.RandomState(seed) and the global stream is left alone).
"""
from __future__ import annotations

import argparse
import json
import logging
import pickle
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from hvae import ops

from ..config import config

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger(__name__)

COLORS = ["#2ecc71", "#3498db", "#9b59b6", "#e74c3c", "#f39c12"]
STYLE = "seaborn-v0_8-whitegrid"
MODEL_NAME = "HybridVAE"

# scikit-learn's TSNE constants (sklearn/manifold/_t_sne.py)
EXPLORATION_ITER = 250        # _EXPLORATION_MAX_ITER: the early-exaggeration stage, and its n_iter_without_progress
N_ITER_CHECK = 50             # _N_ITER_CHECK
EARLY_EXAGGERATION = 12.0
N_ITER_WITHOUT_PROGRESS = 300
MIN_GRAD_NORM = 1e-7
ENCODE_CHUNK = 4096           # users per encoder batch


# =============================================================================
# The latent-space compute (no matplotlib)
# =============================================================================
@dataclass
class LatentProjections:
    mu: np.ndarray                        # [n, L] float32, model.get_user_embedding of the sampled rows
    pca: np.ndarray                       # [n, 2] float64
    explained_variance_ratio: np.ndarray  # [2]
    tsne: np.ndarray                      # [n, 2] float64
    kl_divergence: float
    n_iter: int                           # the last iteration's index, as scikit-learn's n_iter_


def pca_2d(mu: torch.Tensor, return_components: bool = False):
    """Exact two-component PCA of mu [n, L] (device) -> (projection [n, 2] float64 on the device,
    explained_variance_ratio [2] numpy[, components [2, L] numpy]). Each component's largest-magnitude entry is
    positive."""
    n, L = mu.shape
    X = mu.double()
    Xc = X - X.mean(dim=0, keepdim=True)
    tall = None
    if L <= ops.SVD_LD:
        tall = torch.zeros(n, ops.SVD_LD, dtype=torch.float64, device=mu.device)
        tall[:, :L] = Xc
        cov = ops.svd_gram(tall, L)[:L, :L] / (n - 1)
    else:
        cov = Xc.t() @ Xc / (n - 1)
    w, v = np.linalg.eigh(cov.cpu().numpy())  # the one tiny eigenproblem on the host
    comps = v[:, ::-1][:, :2].T.copy()
    big = np.abs(comps).argmax(axis=1)
    comps *= np.sign(comps[np.arange(2), big])[:, None]
    if tall is not None:
        T = torch.zeros(ops.SVD_LD, ops.SVD_LD, dtype=torch.float64)
        T[:L, :2] = torch.as_tensor(comps.T)
        proj = ops.svd_apply(tall, L, T.to(mu.device), 2)[:, :2].contiguous()
    else:
        proj = (Xc @ torch.as_tensor(comps.T.copy(), device=mu.device)).contiguous()
    evr = w[::-1][:2] / w.sum()
    return (proj, evr, comps) if return_components else (proj, evr)


def tsne_init(proj: np.ndarray) -> np.ndarray:
    """scikit-learn's init="pca": the projection in float32 storage, PC1 scaled to a standard deviation of 1e-4."""
    y = np.asarray(proj).astype(np.float32).astype(np.float64)
    return y / np.std(y[:, 0]) * 1e-4


class TsneState:
    """The device buffers of one descent: the embedding (double-buffered), gains, update, forces, statistics."""

    def __init__(self, init: np.ndarray, device):
        y = torch.as_tensor(np.ascontiguousarray(init, dtype=np.float64), device=device)
        self.y, self.y_next = y, torch.empty_like(y)
        self.gains, self.upd = torch.ones_like(y), torch.zeros_like(y)
        self.attr, self.rep = torch.empty_like(y), torch.empty_like(y)
        self.z = torch.empty(y.shape[0], dtype=torch.float64, device=device)
        self.stats = torch.zeros(2, dtype=torch.float64, device=device)

    def step(self, P: "ops.TsneP", exaggeration: float, momentum: float, lr: float, want_stats: bool, **out):
        ops.tsne_forces(self.y, P, self.attr, self.rep, self.z)
        ops.tsne_update(self.attr, self.rep, self.z, self.gains, self.upd, self.y, self.y_next, exaggeration, momentum,
                        lr, P=P if want_stats else None, stats=self.stats if want_stats else None, **out)
        self.y, self.y_next = self.y_next, self.y


def tsne_descend(state: TsneState, P: "ops.TsneP", it: int, max_iter: int, momentum: float, exaggeration: float,
                 n_iter_without_progress: int, lr: float):
    """scikit-learn's _gradient_descent from iteration `it` up to max_iter -> (error, last iteration). Two launches an
    iteration; the error and the gradient norm come back every N_ITER_CHECK-th iteration and on the last one."""
    error = best_error = float(np.finfo(float).max)
    best_iter = i = it
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        want = check or i == max_iter - 1
        state.step(P, exaggeration, momentum, lr, want)
        if want:
            error, grad_norm = state.stats.cpu().tolist()
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= MIN_GRAD_NORM:
                break
    return error, i


def tsne_learning_rate(n: int) -> float:
    return max(n / EARLY_EXAGGERATION / 4.0, 50.0)


def tsne_joint_p(mu: torch.Tensor, perplexity: float) -> "ops.TsneP":
    """Neighbours, the perplexity search and the symmetrisation (the host step) -> the joint P on the device."""
    idx, d2 = ops.tsne_knn(mu, perplexity)
    return ops.tsne_joint(idx, ops.tsne_perplexity(d2, perplexity))


def tsne_embed(P: "ops.TsneP", init: np.ndarray, max_iter: int = 1000, on_stage=None):
    """The two-stage descent from init [n, 2] -> (embedding [n, 2] numpy, kl_divergence, n_iter). on_stage(name, it)
    is called as each stage starts."""
    if max_iter < EXPLORATION_ITER:
        raise ValueError(f"max_iter = {max_iter} is not served: at least {EXPLORATION_ITER}, as scikit-learn's TSNE")
    n = P.n
    lr, state = tsne_learning_rate(n), TsneState(init, P.ptr.device)
    if on_stage:
        on_stage("exaggeration", 0)
    kl, it = tsne_descend(state, P, 0, EXPLORATION_ITER, 0.5, EARLY_EXAGGERATION, EXPLORATION_ITER, lr)
    if it < EXPLORATION_ITER or max_iter - EXPLORATION_ITER > 0:
        if on_stage:
            on_stage("final", it + 1)
        kl, it = tsne_descend(state, P, it + 1, max_iter, 0.8, 1.0, N_ITER_WITHOUT_PROGRESS, lr)
    return state.y.cpu().numpy(), float(kl), int(it)


def encode_users(model, interaction_matrix, indices) -> torch.Tensor:
    """mu [n, L] of the matrix rows `indices` (in that order) as CSR-row batches through the sparse encoder."""
    dev = next(model.parameters()).device
    csr = ops.csr_from_scipy(interaction_matrix, dev)
    rows = torch.as_tensor(np.asarray(indices, np.int32).reshape(-1), device=dev)
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            chunks = [model.get_user_embedding(ops.Csr(csr.row_ptr, csr.col_idx, csr.vals, csr.n_items,
                                                       rows=rows[a:a + ENCODE_CHUNK]))
                      for a in range(0, rows.numel(), ENCODE_CHUNK)]
    finally:
        model.train(was)
    return torch.cat(chunks).float().contiguous()


def latent_projections(model, interaction_matrix, indices, *, perplexity: float = 30.0,
                       max_iter: int = 1000) -> LatentProjections:
    """Encode the users `indices` of the scipy interaction matrix and project their latent means: exact PCA and
    exact t-SNE on the device. A shape outside the served range is a ValueError before any device work."""
    indices = np.asarray(indices).reshape(-1)
    ops.tsne_neighbours(len(indices), int(model.latent_dim), perplexity, "latent_projections")
    if max_iter < EXPLORATION_ITER:
        raise ValueError(f"max_iter = {max_iter} is not served: at least {EXPLORATION_ITER}, as scikit-learn's TSNE")
    mu = encode_users(model, interaction_matrix, indices)
    proj, evr = pca_2d(mu)
    proj_h = proj.cpu().numpy()
    P = tsne_joint_p(mu, perplexity)
    Y, kl, it = tsne_embed(P, tsne_init(proj_h), max_iter)
    return LatentProjections(mu=mu.cpu().numpy(), pca=proj_h, explained_variance_ratio=evr, tsne=Y, kl_divergence=kl,
                             n_iter=it)


def sample_users(n_users: int, n_samples: int, seed: int | None = None) -> np.ndarray:
    """The reference's draw: np.random.choice(n_users, n_samples, replace=False) when there are more users than
    samples, else every user in order. With a seed the draw comes from its own RandomState."""
    if n_users <= n_samples:
        return np.arange(n_users)
    rng = np.random if seed is None else np.random.RandomState(seed)
    return rng.choice(n_users, min(n_samples, n_users), replace=False)


# =============================================================================
# Plot helpers
# =============================================================================
def _pyplot():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def _get_dataset_name() -> str:
    """RAW_DATA_FILE's stem with spaces ("All_Beauty.jsonl" -> "All Beauty"), or ""."""
    raw = getattr(config, "RAW_DATA_FILE", "")
    return Path(raw).stem.replace("_", " ") if raw else ""


def _get_dataset_prefix() -> str:
    """RAW_DATA_FILE's stem in lower case plus "_" ("All_Beauty.jsonl" -> "all_beauty_"), or ""."""
    raw = getattr(config, "RAW_DATA_FILE", "")
    return f"{Path(raw).stem.lower()}_" if raw else ""


def _save_figure(fig, path: Path, name: str, prefix: str = "") -> None:
    plt = _pyplot()
    filename = f"{prefix}{name}" if prefix else name
    fig.savefig(Path(path) / filename, dpi=150, bbox_inches="tight")
    plt.close(fig)
    logger.info(f"Saved {filename} to {path}")


def _get_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the latent-space figures need the HIP device; there is no CPU path")
    return torch.device("cuda")


def _title_prefix(*parts: str) -> str:
    joined = " - ".join(p for p in parts if p)
    return f"{joined}: " if joined else ""


def _line_axes(ax, epochs, series, xlabel, ylabel, title, legend=True):
    for values, fmt, label in series:
        ax.plot(epochs, values, fmt, label=label, linewidth=2)
    ax.set(xlabel=xlabel, ylabel=ylabel, title=title)
    if legend:
        ax.legend(fontsize=11)
    ax.grid(True, alpha=0.3)


# =============================================================================
# Training figures
# =============================================================================
def plot_training_curves(
    train_losses: list[float],
    val_losses: list[float],
    train_recon_losses: list[float],
    train_kl_losses: list[float],
    output_path: Path,
    dataset_name: str = "",
    model_name: str = "HybridVAE",
    file_prefix: str = "",
) -> None:
    """loss_curves.png, loss_components.png and training_summary.png."""
    plt = _pyplot()
    plt.style.use(STYLE)
    epochs = list(range(1, len(train_losses) + 1))
    best = int(np.argmin(val_losses)) + 1
    head = _title_prefix(dataset_name, model_name)
    total = [(train_losses, "b-", "Training Loss"), (val_losses, "r-", "Validation Loss")]
    parts = [(train_recon_losses, "b-", "Reconstruction Loss"), (train_kl_losses, "orange", "KL Divergence")]

    fig, ax = plt.subplots(figsize=(10, 6))
    _line_axes(ax, epochs, total, "Epoch", "Loss", f"{head}Training vs Validation Loss", legend=False)
    ax.axvline(x=best, color="green", linestyle="--", alpha=0.7, label=f"Best (epoch {best})")
    ax.legend(fontsize=11)
    fig.tight_layout()
    _save_figure(fig, output_path, "loss_curves.png", file_prefix)

    fig, ax = plt.subplots(figsize=(10, 6))
    _line_axes(ax, epochs, parts, "Epoch", "Loss Component", f"{head}Loss Components (Reconstruction vs KL)")
    fig.tight_layout()
    _save_figure(fig, output_path, "loss_components.png", file_prefix)

    fig, axes = plt.subplots(2, 2, figsize=(14, 10))
    _line_axes(axes[0, 0], epochs, [(train_losses, "b-", "Train"), (val_losses, "r-", "Val")], "Epoch", "Total Loss",
               "Training vs Validation Loss")
    axes[0, 0].axvline(x=best, color="green", linestyle="--", alpha=0.7)
    _line_axes(axes[0, 1], epochs, [(train_recon_losses, "b-", None)], "Epoch", "Reconstruction Loss",
               "Reconstruction Loss (Multinomial NLL)", legend=False)
    _line_axes(axes[1, 0], epochs, [(train_kl_losses, "orange", None)], "Epoch", "KL Divergence",
               "KL Divergence (Regularization)", legend=False)
    share = [r / (r + k) if (r + k) > 0 else 0.5 for r, k in zip(train_recon_losses, train_kl_losses)]
    _line_axes(axes[1, 1], epochs, [(share, "purple", None)], "Epoch", "Reconstruction / Total",
               "Reconstruction Loss Ratio", legend=False)
    axes[1, 1].set_ylim(0, 1)
    fig.suptitle(f"{head}Training Summary", fontsize=16, fontweight="bold", y=1.02)
    fig.tight_layout()
    _save_figure(fig, output_path, "training_summary.png", file_prefix)


def _scatter_axes(fig, ax, xy, colour, labels):
    sc = ax.scatter(xy[:, 0], xy[:, 1], c=colour, cmap="viridis", alpha=0.6, s=20)
    fig.colorbar(sc, ax=ax, label="Log(1 + #Interactions)")
    ax.set(xlabel=labels[0], ylabel=labels[1], title=labels[2])


def plot_latent_space(
    model_path: Path,
    data_dir: Path,
    embeddings_path: Path,
    output_path: Path,
    n_samples: int = 2000,
    dataset_name: str = "",
    model_name: str = "HybridVAE",
    file_prefix: str = "",
    seed: int | None = None,
) -> None:
    """latent_space_pca.png, latent_space_tsne.png and latent_space_combined.png of a sample of users."""
    from ..preprocessing.embeddings import load_embeddings
    from .evaluate import load_model_from_checkpoint

    device = _get_device()
    logger.info(f"Using device: {device}")
    embeddings, _, _ = load_embeddings(str(embeddings_path))
    model = load_model_from_checkpoint(str(model_path), embeddings, device)
    model.to(device).eval()
    with open(Path(data_dir) / "interaction_matrix.pkl", "rb") as f:
        interaction_matrix = pickle.load(f).tocsr()  # the project's own artifact

    indices = sample_users(interaction_matrix.shape[0], n_samples, seed)
    logger.info("Computing user embeddings, PCA and t-SNE projections...")
    res = latent_projections(model, interaction_matrix, indices)
    logger.info(f"t-SNE: KL divergence {res.kl_divergence:.6f} after {res.n_iter + 1} iterations")
    log_activity = np.log1p(np.diff(interaction_matrix.indptr)[indices])

    plt = _pyplot()
    head = _title_prefix(dataset_name, model_name)
    evr = res.explained_variance_ratio
    pca_axes = (f"PC1 ({evr[0]:.1%} var)", f"PC2 ({evr[1]:.1%} var)")
    for name, xy, labels in (
        ("latent_space_pca.png", res.pca, pca_axes + (f"{head}User Latent Space (PCA)",)),
        ("latent_space_tsne.png", res.tsne, ("t-SNE 1", "t-SNE 2", f"{head}User Latent Space (t-SNE)")),
    ):
        fig, ax = plt.subplots(figsize=(10, 8))
        _scatter_axes(fig, ax, xy, log_activity, labels)
        fig.tight_layout()
        _save_figure(fig, output_path, name, file_prefix)

    fig, axes = plt.subplots(1, 2, figsize=(16, 6))
    _scatter_axes(fig, axes[0], res.pca, log_activity, pca_axes + ("PCA Projection",))
    _scatter_axes(fig, axes[1], res.tsne, log_activity, ("t-SNE 1", "t-SNE 2", "t-SNE Projection"))
    fig.suptitle(f"{head}User Latent Space Visualization", fontsize=14, fontweight="bold")
    fig.tight_layout()
    _save_figure(fig, output_path, "latent_space_combined.png", file_prefix)


# =============================================================================
# Baseline figures
# =============================================================================
def plot_baseline_comparison(
    all_results: dict[str, dict],
    k_values: list[int],
    output_path: Path,
    n_negatives: int | None = 99,
    dataset_name: str = "",
    file_prefix: str = "",
) -> None:
    """baseline_{recall,ndcg,hitrate}_comparison.png and baseline_summary.png."""
    plt = _pyplot()
    plt.style.use(STYLE)
    head = f"{dataset_name}: " if dataset_name else ""
    models = list(all_results)
    protocol = f"Negative Sampling ({n_negatives})" if n_negatives else "Full Ranking"
    pos, width = np.arange(len(k_values)), 0.25
    colour = [COLORS[i % len(COLORS)] for i in range(len(models))]

    def nice(metric):
        return metric.replace("_", " ").title()

    for metric, filename in (("recall", "baseline_recall_comparison.png"), ("ndcg", "baseline_ndcg_comparison.png"),
                             ("hit_ratio", "baseline_hitrate_comparison.png")):
        fig, ax = plt.subplots(figsize=(10, 6))
        for i, m in enumerate(models):
            ax.bar(pos + width * i, [all_results[m][k][metric] for k in k_values], width, label=m, color=colour[i])
        ax.set(xlabel="K", ylabel=f"{nice(metric)}@K", title=f"{head}{nice(metric)}@K Comparison ({protocol})")
        ax.set_xticks(pos + width)
        ax.set_xticklabels([f"@{k}" for k in k_values])
        ax.legend(fontsize=11)
        ax.grid(True, alpha=0.3, axis="y")
        fig.tight_layout()
        _save_figure(fig, output_path, filename, file_prefix)

    fig, axes = plt.subplots(2, 2, figsize=(14, 10))
    k_main = 10
    for ax, metric, title in ((axes[0, 0], "recall", "Recall@10"), (axes[0, 1], "ndcg", "NDCG@10"),
                              (axes[1, 0], "hit_ratio", "Hit Ratio@10")):
        values = [all_results[m][k_main][metric] for m in models]
        for bar, v in zip(ax.bar(models, values, color=colour), values):
            ax.text(bar.get_x() + bar.get_width() / 2, bar.get_height() + 0.005, f"{v:.3f}", ha="center", va="bottom",
                    fontsize=10)
        ax.set(ylabel=title, title=f"{title} by Model")
        ax.grid(True, alpha=0.3, axis="y")
    for i, m in enumerate(models):
        axes[1, 1].plot(k_values, [all_results[m][k]["recall"] for k in k_values], "o-", label=m, color=colour[i],
                        linewidth=2, markersize=8)
    axes[1, 1].set(xlabel="K", ylabel="Recall@K", title="Recall@K Trend")
    axes[1, 1].legend()
    axes[1, 1].grid(True, alpha=0.3)
    fig.suptitle(f"{head}Baseline Models Comparison ({protocol})", fontsize=16, fontweight="bold", y=1.02)
    fig.tight_layout()
    _save_figure(fig, output_path, "baseline_summary.png", file_prefix)


# =============================================================================
# Grid-search figures
# =============================================================================
def _config_label(cfg: dict) -> str:
    hidden = cfg.get("hidden_dims", [])
    return (f"L{cfg.get('latent_dim', '?')}\nH{'x'.join(map(str, hidden)) if hidden else '?'}\n"
            f"d{cfg.get('dropout', '?')}\nβ{cfg.get('beta', '?')}")


def plot_grid_search_results(
    results_path: Path,
    output_path: Path,
    dataset_name: str = "",
    model_name: str = "HybridVAE",
    file_prefix: str = "",
) -> None:
    """grid_search_top_configs.png, _param_impact.png, _heatmap.png (latent_dim x beta, when both were searched) and
    _scatter.png."""
    plt = _pyplot()
    plt.style.use(STYLE)
    head = _title_prefix(dataset_name, model_name)
    with open(results_path) as f:
        data = json.load(f)
    runs = [r for r in data["all_results"] if "error" not in r]
    if not runs:
        logger.error("No valid results found in grid search")
        return
    configs = [r["config"] for r in runs]
    ndcg = [r["ndcg@10"] for r in runs]
    recall = [r["recall@10"] for r in runs]

    top = sorted(runs, key=lambda r: r["ndcg@10"], reverse=True)[:10]
    pos, width = np.arange(len(top)), 0.35
    fig, ax = plt.subplots(figsize=(14, 6))
    bars = ax.bar(pos - width / 2, [r["ndcg@10"] for r in top], width, label="NDCG@10", color="#3498db")
    ax.bar(pos + width / 2, [r["recall@10"] for r in top], width, label="Recall@10", color="#2ecc71")
    for bar in bars:
        ax.text(bar.get_x() + bar.get_width() / 2, bar.get_height(), f"{bar.get_height():.3f}", ha="center",
                va="bottom", fontsize=8)
    ax.set(xlabel="Configuration (L=latent, H=hidden, d=dropout, β=beta)", ylabel="Score",
           title=f"{head}Top 10 Hyperparameter Configurations")
    ax.set_xticks(pos)
    ax.set_xticklabels([_config_label(r["config"]) for r in top], fontsize=8)
    ax.legend()
    ax.grid(True, alpha=0.3, axis="y")
    fig.tight_layout()
    _save_figure(fig, output_path, "grid_search_top_configs.png", file_prefix)

    params = list(configs[0])
    fig, axes = plt.subplots(2, 3, figsize=(15, 10))
    axes = axes.flatten()
    for slot, ax in enumerate(axes):
        if slot >= min(len(params), 6):
            ax.set_visible(False)
            continue
        groups: dict[str, list[float]] = {}
        for cfg, score in zip(configs, ndcg):
            groups.setdefault(str(cfg[params[slot]]), []).append(score)
        boxes = ax.boxplot(list(groups.values()), tick_labels=list(groups), patch_artist=True)
        for patch in boxes["boxes"]:
            patch.set_facecolor("#3498db")
            patch.set_alpha(0.7)
        ax.set(title=params[slot], ylabel="NDCG@10")
        ax.grid(True, alpha=0.3, axis="y")
        ax.tick_params(axis="x", rotation=45)
    fig.suptitle(f"{head}Hyperparameter Impact on NDCG@10", fontsize=16, fontweight="bold", y=1.02)
    fig.tight_layout()
    _save_figure(fig, output_path, "grid_search_param_impact.png", file_prefix)

    if "latent_dim" in params and "beta" in params:
        latents = sorted({c["latent_dim"] for c in configs})
        betas = sorted({c["beta"] for c in configs})
        total, count = np.zeros((len(latents), len(betas))), np.zeros((len(latents), len(betas)))
        for cfg, score in zip(configs, ndcg):
            cell = latents.index(cfg["latent_dim"]), betas.index(cfg["beta"])
            total[cell] += score
            count[cell] += 1
        mean = total / np.maximum(count, 1)
        fig, ax = plt.subplots(figsize=(10, 8))
        im = ax.imshow(mean, cmap="YlGnBu", aspect="auto")
        ax.set_xticks(np.arange(len(betas)))
        ax.set_yticks(np.arange(len(latents)))
        ax.set_xticklabels([str(b) for b in betas])
        ax.set_yticklabels([str(v) for v in latents])
        ax.set(xlabel="Beta (KL Weight)", ylabel="Latent Dimension",
               title=f"{head}Average NDCG@10 (Latent Dim vs Beta)")
        for (i, j), v in np.ndenumerate(mean):
            ax.text(j, i, f"{v:.3f}", ha="center", va="center", fontsize=10)
        fig.colorbar(im, ax=ax, label="NDCG@10")
        fig.tight_layout()
        _save_figure(fig, output_path, "grid_search_heatmap.png", file_prefix)

    best = int(np.argmax(ndcg))
    fig, ax = plt.subplots(figsize=(10, 6))
    ax.scatter(recall, ndcg, alpha=0.6, s=50, c="#3498db")
    ax.scatter([recall[best]], [ndcg[best]], s=200, c="#e74c3c", marker="*", label="Best Config", zorder=5)
    ax.set(xlabel="Recall@10", ylabel="NDCG@10", title=f"{head}Grid Search Results (Recall vs NDCG)")
    ax.legend()
    ax.grid(True, alpha=0.3)
    note = "\n".join(f"{k}: {v}" for k, v in data["best_config"].items())
    ax.annotate(f"Best:\n{note}", xy=(recall[best], ndcg[best]), xytext=(10, -10), textcoords="offset points",
                fontsize=8, bbox=dict(boxstyle="round", fc="yellow", alpha=0.5))
    fig.tight_layout()
    _save_figure(fig, output_path, "grid_search_scatter.png", file_prefix)


# =============================================================================
# Entry points
# =============================================================================
def _figures_dir(model_dir: str) -> Path:
    figures = Path(model_dir) / "figures"
    figures.mkdir(parents=True, exist_ok=True)
    return figures


def visualize_training(model_dir: str, data_dir: str, embeddings_path: str, n_samples: int = 2000,
                       seed: int | None = None) -> None:
    """Training curves from training_history.json, and the latent-space figures when best_model.pth exists."""
    figures = _figures_dir(model_dir)
    name, prefix = _get_dataset_name(), _get_dataset_prefix()
    history_path = Path(model_dir) / "training_history.json"
    if not history_path.exists():
        logger.error(f"Training history not found: {history_path}. Run `make train` first.")
        return
    history = json.loads(history_path.read_text())
    logger.info("Generating training curve visualizations...")
    plot_training_curves(history["train_losses"], history["val_losses"], history["train_recon_losses"],
                         history["train_kl_losses"], figures, dataset_name=name, model_name=MODEL_NAME,
                         file_prefix=prefix)
    best_model = Path(model_dir) / "best_model.pth"
    if best_model.exists():
        logger.info("Generating latent space visualizations...")
        plot_latent_space(best_model, Path(data_dir), Path(embeddings_path), figures, n_samples=n_samples,
                          dataset_name=name, model_name=MODEL_NAME, file_prefix=prefix, seed=seed)
    else:
        logger.warning(f"Model not found: {best_model}, skipping latent space plots")
    logger.info(f"All visualizations saved to {figures}")


def visualize_baselines(model_dir: str) -> None:
    """Baseline comparison figures from figures/baseline_results.json."""
    figures = _figures_dir(model_dir)
    name, prefix = _get_dataset_name(), _get_dataset_prefix()
    results_path = figures / "baseline_results.json"
    if not results_path.exists():
        logger.error(f"Baseline results not found: {results_path}. Run `make baseline` first.")
        return
    raw = json.loads(results_path.read_text())
    # this project's results files carry a "training_time_seconds" entry beside the K entries
    results = {m: {int(k): v for k, v in entry.items() if str(k).lstrip("-").isdigit()} for m, entry in raw.items()}
    k_values = sorted(next(iter(results.values())))
    logger.info("Generating baseline comparison visualizations...")
    plot_baseline_comparison(results, k_values, figures, dataset_name=name, file_prefix=prefix)
    logger.info(f"All visualizations saved to {figures}")


def visualize_grid_search(model_dir: str) -> None:
    """Grid-search figures from grid_search_results.json."""
    figures = _figures_dir(model_dir)
    name, prefix = _get_dataset_name(), _get_dataset_prefix()
    results_path = Path(model_dir) / "grid_search_results.json"
    if not results_path.exists():
        logger.error(f"Grid search results not found: {results_path}. Run `make tune` first.")
        return
    logger.info("Generating grid search visualizations...")
    plot_grid_search_results(results_path, figures, dataset_name=name, model_name=MODEL_NAME, file_prefix=prefix)
    logger.info(f"All visualizations saved to {figures}")


def main() -> None:
    parser = argparse.ArgumentParser(description="Generate visualizations for recommendation system (MI355X)")
    sub = parser.add_subparsers(dest="command", help="Visualization type")
    for command, text, full in (("training", "Generate training visualizations", True),
                                ("baseline", "Generate baseline visualizations", False),
                                ("tuning", "Generate grid search visualizations", False),
                                ("all", "Generate all visualizations", True)):
        p = sub.add_parser(command, help=text)
        p.add_argument("--model-dir", default=str(config.MODEL_DIR))
        if full:
            p.add_argument("--data-dir", default=str(config.DATA_DIR))
            p.add_argument("--embeddings", default=str(config.EMBEDDINGS_FILE))
            p.add_argument("--n-samples", type=int, default=2000, help="users in the latent-space figures")
            p.add_argument("--seed", type=int, default=None,
                           help="draw the sample from np.random.RandomState(seed) (default: the global stream)")
    args = parser.parse_args()
    if args.command in ("training", "all"):
        visualize_training(args.model_dir, args.data_dir, args.embeddings, n_samples=args.n_samples, seed=args.seed)
    if args.command in ("baseline", "all"):
        visualize_baselines(args.model_dir)
    if args.command in ("tuning", "all"):
        visualize_grid_search(args.model_dir)
    if args.command is None:
        parser.print_help()


if __name__ == "__main__":
    main()
