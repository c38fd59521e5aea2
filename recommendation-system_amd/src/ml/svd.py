"""SVD baseline on MI355X -- the reference's SVDRecommender (src/ml/baseline.py:102-118), fitted and evaluated on
the device (`make baseline-svd`).

The reference calls scikit-learn's TruncatedSVD(n_components=50, random_state=42): a randomized SVD that draws a
Gaussian sketch Omega of W = n_components + 10 columns, runs five rounds of Q <- lu(M Q), Q <- lu(M^T Q) over
M = A (or A^T when there are fewer users than items), then Q <- qr(M Q), B = Q^T M and a dense SVD of B. The scores
user_factors @ item_factors = A V V^T depend on the span of V only, and in exact arithmetic any orthonormalisation
gives the same span. Here every normaliser is CholeskyQR2 (ops.svd_orthonormalize: Gram matrix, Cholesky, product with
R^-1, twice) and the SVD of B is the eigendecomposition of the W x W Gram matrix of B^T; all of it is fp64 in
libhvae (csrc/hvae_svd.hip), the sparse products gathered from the device CSR and CSC of A. The result follows
scikit-learn's own run to about 1e-13 (tests/golden/make_svd_fixture.py).

fit() draws the sketch on the host from np.random.RandomState(42), draw for draw the reference's; numpy's global
stream is not touched. The W x W symmetric eigenproblem is solved on the host (numpy.linalg.eigh): reading that
Gram matrix is the only synchronisation before the end of fit, where the rank flag is read. CholeskyQR2 needs the
sketch's columns to stay linearly independent (cond(Y^T Y) far below 2^53; a few thousand on real interaction
data); a matrix of rank below W breaks the Cholesky factorisation, sets the flag, and fit raises.

Scoring, ranking, ties and negatives are src/ml/baseline.py's (evaluate_model), unchanged; main() sets the "SVD"
entry of models/figures/baseline_results.json beside the entries `make baseline` wrote.
"""
from __future__ import annotations

import logging

import numpy as np
import torch
from scipy.sparse import csr_matrix

from hvae import ops

from .baseline import BaseRecommender, _resolve_device, parse_args, run_baseline

logger = logging.getLogger(__name__)

NAME = "SVD"
RANDOM_STATE = 42       # the reference's (baseline.py:107)
N_OVERSAMPLES = 10      # TruncatedSVD's defaults
N_ITER = 5
SERVED_COMPONENTS = (1, ops.SVD_LD - N_OVERSAMPLES)


def check_components(n_components: int, shape: tuple[int, int] | None = None) -> None:
    lo, hi = SERVED_COMPONENTS
    served = (f"served: {lo} <= n_components <= {hi} with n_components + {N_OVERSAMPLES} <= min(n_users, n_items)")
    if not lo <= n_components <= hi:
        raise ValueError(f"SVD: n_components {n_components} is not served; {served}")
    if shape is not None and n_components + N_OVERSAMPLES > min(shape):
        raise ValueError(f"SVD: n_components {n_components} is not served for a {shape[0]} x {shape[1]} matrix; "
                         f"{served}")


def sketch(n: int, W: int) -> np.ndarray:
    """The reference's starting matrix [n, W] (randomized_svd's random_state.normal(size=(n, W))), from a
    RandomState of its own."""
    return np.random.RandomState(RANDOM_STATE).normal(size=(n, W))


def eig_transform(G: np.ndarray, W: int, k: int, transposed: bool):
    """The host step. From G = B B^T [W, W] (the Gram matrix of B^T): (s [k], T [64, 64]) with the eigenpairs
    ordered by descending eigenvalue, s = sqrt(w) the singular values of B, and T the matrix whose product gives
    the item-space components: E diag(1 / s) applied to B^T when M = A, E applied to Q when M = A^T."""
    w, E = np.linalg.eigh(G[:W, :W])
    order = np.argsort(w)[::-1]
    w, E = w[order], E[:, order]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(w)
        T = np.zeros((ops.SVD_LD, ops.SVD_LD))
        T[:W, :k] = (E if transposed else E / s)[:, :k]
    return s[:k], T


class SVDRecommender(BaseRecommender):
    """The reference's SVDRecommender with its attributes (n_components, user_factors [n_users, k], item_factors
    [k, n_items], fit, predict), both fp64 on the device, plus singular_values_ and explained_variance_ratio_
    (TruncatedSVD's) and the batched device scoring that baseline.evaluate_model uses (fp32)."""

    def __init__(self, n_components: int = 50, device=None):
        check_components(n_components)
        self.n_components = n_components
        self._device_arg = device
        self.user_factors: torch.Tensor | None = None
        self.item_factors: torch.Tensor | None = None
        self.singular_values_: torch.Tensor | None = None
        self.explained_variance_ratio_: torch.Tensor | None = None

    def fit(self, interaction_matrix: csr_matrix) -> None:
        """The subspace iteration on the device. The host waits for the device once, for the W x W Gram matrix
        whose eigenproblem it solves, and once more at the end, for the rank flag."""
        logger.info(f"Fitting SVD ({self.n_components} components)...")
        n_users, n_items = interaction_matrix.shape
        check_components(self.n_components, (n_users, n_items))
        k, W = self.n_components, self.n_components + N_OVERSAMPLES
        self.n_users, self.n_items = n_users, n_items
        self.transposed = transposed = n_users < n_items   # randomized_svd's transpose="auto"
        omega = sketch(n_users if transposed else n_items, W)
        full_var = self._full_variance(interaction_matrix)
        self.device = dev = _resolve_device(self._device_arg)
        csr = ops.csr_from_scipy(interaction_matrix, dev)
        csc = ops.csc_from_scipy(interaction_matrix, dev)
        M, Mt = (csc, csr) if transposed else (csr, csc)   # M X and M^T X
        m, n = (n_items, n_users) if transposed else (n_users, n_items)
        Q = ops.svd_tall(n, dev, omega)
        Y = torch.empty(m, ops.SVD_LD, dtype=torch.float64, device=dev)
        G, Rinv = (torch.empty(ops.SVD_LD, ops.SVD_LD, dtype=torch.float64, device=dev) for _ in range(2))
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(N_ITER):
            ops.svd_orthonormalize(ops.svd_spmm(M, Q, W, out=Y), W, flag, G, Rinv)
            ops.svd_orthonormalize(ops.svd_spmm(Mt, Y, W, out=Q), W, flag, G, Rinv)
        ops.svd_orthonormalize(ops.svd_spmm(M, Q, W, out=Y), W, flag, G, Rinv)   # Y: the orthonormal basis [m, W]
        Bt = ops.svd_spmm(Mt, Y, W, out=Q)                                       # B^T = M^T Q [n, W]
        g_host = ops.svd_gram(Bt, W, G).cpu().numpy()                            # the one wait inside the iteration
        if not np.isfinite(g_host).all():
            self._raise_if_flagged(flag, force=True)
        s, T = eig_transform(g_host, W, k, transposed)
        comps = ops.svd_apply(Y if transposed else Bt, W, torch.as_tensor(T, device=dev), k)   # [n_items, 64]
        # svd_flip(u_based_decision=False): each component's largest-magnitude entry (the first of equals) positive
        big = comps.abs().argmax(dim=0, keepdim=True)
        sign = torch.sign(comps.gather(0, big))
        sign[:, k:] = 1.0
        comps = (comps * sign).contiguous()
        users = ops.svd_spmm(csr, comps, k)                                      # A V [n_users, 64]
        self.user_factors = users[:, :k]
        self.item_factors = comps[:, :k].t()
        self.singular_values_ = torch.as_tensor(s, device=dev)
        self.explained_variance_ratio_ = torch.var(self.user_factors, dim=0, unbiased=False) / full_var
        self._users32, self._items32 = users.float().contiguous(), comps.float().contiguous()
        self._raise_if_flagged(flag)
        logger.info(f"Explained variance: {float(self.explained_variance_ratio_.sum()):.4f}")

    @staticmethod
    def _raise_if_flagged(flag: torch.Tensor, force: bool = False) -> None:
        if int(flag.item()) or force:
            raise RuntimeError("SVD: the interaction matrix's sketch is rank-deficient (a Cholesky pivot of its Gram "
                               "matrix is not positive): the matrix's rank is below n_components + "
                               f"{N_OVERSAMPLES}; ask for fewer components")

    @staticmethod
    def _full_variance(matrix: csr_matrix) -> float:
        """The summed per-column variance of A (scikit-learn's mean_variance_axis(X, axis=0)[1].sum()), float64 on
        the host: a property of the input alone."""
        a = matrix.tocsr().astype(np.float64)
        n = a.shape[0]
        mean = np.asarray(a.sum(axis=0)).ravel() / n
        return float((np.asarray(a.multiply(a).sum(axis=0)).ravel() / n - mean ** 2).sum())

    def predict(self, user_idx: int) -> np.ndarray:
        return self.score_all(np.array([user_idx]))[0].cpu().numpy()

    def score_candidates(self, users: np.ndarray, cand: torch.Tensor) -> torch.Tensor:
        rows = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=self.device)
        return ops.score_candidates(self._users32, rows, self._items32, cand.contiguous())

    def score_all(self, users: np.ndarray) -> torch.Tensor:
        rows = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int64), device=self.device)
        return ops.gemm(self._users32.index_select(0, rows), self._items32.t())


def run_svd(data_dir: str, k_values: list[int] | None = None, n_negatives: int | None = 99,
            n_components: int = 50) -> dict:
    """Fit and evaluate SVD as the reference's run_all_baselines does for one model (baseline.py:474-533)."""
    return run_baseline(SVDRecommender(n_components), NAME, data_dir, k_values, n_negatives)


def main() -> None:
    args = parse_args("Fit and evaluate the SVD baseline (MI355X)", lambda p: p.add_argument(
        "--n-components", type=int, default=50, help="served: 1 to 54"))
    run_svd(args.data, args.k_values, args.n_negatives, n_components=args.n_components)


if __name__ == "__main__":
    main()
