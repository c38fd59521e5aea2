"""k_svd_spmm and k_lgcn_propagate as instantiations of csrc/hvae_rowgather.h return the bits they returned as two
hand-written kernels.

The scipy comparisons in tests/test_gpu_svd.py and tests/test_gpu_lightgcn.py hold for any summation order; the
header's contract is one order (its first comment), so these cases compare with tests/golden/rowgather_parent.json
and .npz, recorded by tests/golden/make_rowgather_fixture.py on the commit before the header existed: the SHA-256 of
every output's bytes on the three graphs of lightgcn_ref.KERNEL_GRAPHS (short rows, a 120-entry row, split rows of
290 and 1500 entries, empty rows), and the arrays themselves on 37x23, where a mismatch can then be located.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import lightgcn_ref as LR
import make_rowgather_fixture as MF

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES = list(LR.KERNEL_GRAPHS)


@pytest.fixture(scope="module")
def digests():
    return json.loads((GOLDEN / "rowgather_parent.json").read_text())["sha256"]


@pytest.fixture(scope="module")
def arrays():
    return dict(np.load(GOLDEN / "rowgather_parent.npz", allow_pickle=False))


def test_fixture_holds_the_cases(digests, arrays):
    assert MF.graphs() == ["37x23", "300x257", "2100x130"] and MF.ARRAY_GRAPH == "37x23"
    assert set(digests) == set(MF.keys()) and len(digests) == 3 * (2 * 3 + 2 * 2 * 2)
    assert set(arrays) == set(MF.keys([MF.ARRAY_GRAPH]))
    for k, a in arrays.items():
        assert MF.digest(a) == digests[k]


def _check(key, got, digests, arrays):
    if key in arrays:
        want = arrays[key]
        assert got.dtype == want.dtype and got.shape == want.shape
        diff = np.flatnonzero((got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape[0], -1).any(axis=1))
        assert diff.size == 0, f"{key}: rows {diff.tolist()} differ from the parent's"
    assert MF.digest(got) == digests[key], f"{key}: not the parent's bits"


@pytest.mark.parametrize("W", MF.WIDTHS)
@pytest.mark.parametrize("image", ["csr", "csc"])
@pytest.mark.parametrize("name", NAMES)
def test_svd_spmm_returns_the_parents_bits(hip_device, digests, arrays, name, image, W):
    _check(MF.svd_key(name, image, W), MF.svd_case(name, image, W), digests, arrays)


@pytest.mark.parametrize("alpha", MF.ALPHAS)
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("d", MF.DIMS)
@pytest.mark.parametrize("name", NAMES)
def test_lgcn_propagate_returns_the_parents_bits(hip_device, digests, arrays, name, d, with_add, alpha):
    _check(MF.lgcn_key(name, d, with_add, alpha), MF.lgcn_case(name, d, with_add, alpha), digests, arrays)
