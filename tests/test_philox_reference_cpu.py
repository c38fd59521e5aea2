"""The numpy restatement of the random stream (tests/philox_ref.py), checked without a GPU.

tests/test_gpu_philox.py holds the kernels to philox_ref bit for bit. That means something only if philox_ref is
Philox4x32-10 (the published known-answer vectors of Random123), if its uniforms and normals have the distribution
the model needs, and if each way a kernel could get the stream wrong -- another tag, step, seed word or element
index -- gives a mask that differs nearly as much as an independent one (two independent masks at p = 0.3 differ in
2 p (1 - p) = 42 % of their elements).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import philox_ref as P  # noqa: E402

SEED = (5 << 40) + 1234
STEP = 5
N_STAT = 1 << 22

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = P.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want
    # vectorised: the same answer in every lane of an array call
    arr = P.philox4x32_10(*(np.full(5, c, dtype=np.uint64) for c in ctr), *key)
    assert all(np.all(a == np.uint64(w)) for a, w in zip(arr, want))


def test_words_layout():
    """words() places idx, step, tag and seed as the contract says (against philox4x32_10 called by hand)."""
    idx = np.array([0, 1, 0xFFFFFFFF, (3 << 32) + 7], dtype=np.uint64)
    got = P.words(SEED, STEP, 0x102, idx)
    want = P.philox4x32_10(idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), STEP, 0x102, SEED & 0xFFFFFFFF,
                           SEED >> 32)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert (SEED >> 32) != 0  # the seed of every test has a high word
    # the step enters with its low 32 bits (the kernels cast the int64 counter)
    assert all(np.array_equal(a, b) for a, b in zip(P.words(SEED, STEP + (1 << 32), 0x102, idx), got))


def test_u01_and_mult_edges():
    assert P.u01(np.uint64(0xFFFFFFFF)) == np.float32(1.0) - np.float32(2.0 ** -24)  # < 1
    assert P.u01(np.uint64(0xFF)) == 0.0
    assert P.mult(SEED, STEP, P.TAG_PROJ_DROP, 3, 8, 0.0).tolist() == [[1.0] * 8] * 3
    assert P.mult(SEED, STEP, P.TAG_PROJ_DROP, 3, 8, 1.0).tolist() == [[0.0] * 8] * 3
    m = P.mult(SEED, STEP, P.TAG_PROJ_DROP, 16, 64, 0.3)
    assert m.dtype == np.float32
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.3)))}
    assert np.array_equal(m != 0, P.keep(SEED, STEP, P.TAG_PROJ_DROP, 16, 64, 0.3))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_fraction(p):
    n = N_STAT
    frac = P.keep_idx(SEED, STEP, P.TAG_ENC_DROP, np.arange(n), p).mean()
    print(f"p = {p}: keep fraction off by {abs(frac - (1 - p)):.2e}")
    assert abs(frac - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n)


def test_normal_moments():
    n = N_STAT
    idx = np.arange(n)
    z = P.normal_idx(SEED, STEP, P.TAG_EPS, idx)
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    dev = np.abs(P.normal32_idx(SEED, STEP, P.TAG_EPS, idx).astype(np.float64) - z).max()
    print(f"normal: mean {mean:.2e}, variance {var:.5f}, kurtosis {kurt:.4f}; max |normal32 - normal| = {dev:.2e}")
    assert np.isfinite(z).all()
    assert abs(mean) < 4 / np.sqrt(n)
    assert abs(var - 1) < 1e-2
    assert abs(kurt - 3) < 0.05
    assert dev < 2e-6  # the float32 evaluation stays a float32 rounding away, so 8 x dev is a usable GPU bar


# ------------------------------------------------------------ mutation proofs --
NB, W, PD = 64, 64, 0.3
TAG = P.TAG_ENC_DROP + 1


def _true():
    return P.keep(SEED, STEP, TAG, NB, W, PD)


def _mutants():
    idx = P.index(NB, W)
    yield "tag + 1", P.keep(SEED, STEP, TAG + 1, NB, W, PD)
    yield "step + 1", P.keep(SEED, STEP + 1, TAG, NB, W, PD)
    yield "seed high word cleared", P.keep(SEED & 0xFFFFFFFF, STEP, TAG, NB, W, PD)
    yield "index + 1", P.keep_idx(SEED, STEP, TAG, idx + np.uint64(1), PD)
    yield "row * (width + 4) + col", P.keep_idx(SEED, STEP, TAG, P.index(NB, W, ld=W + 4), PD)
    yield "4-chunks reversed", _true().reshape(NB, W // 4, 4)[:, :, ::-1].reshape(NB, W)


def test_mutations_move_the_mask():
    true = _true()
    seen = []
    for name, mask in _mutants():
        diff = float((mask != true).mean())
        print(f"{name}: differs in {diff:.3f}")
        seen.append(name)
        assert mask.shape == true.shape
        assert diff >= 0.30, name
    assert len(seen) == 6


def test_mutations_move_the_noise():
    """The same for eps: a wrong step, seed word or index gives noise that is uncorrelated with the true one."""
    true = P.normal(SEED, STEP, NB, W)
    for name, other in (("step + 1", P.normal(SEED, STEP + 1, NB, W)),
                        ("seed high word cleared", P.normal(SEED & 0xFFFFFFFF, STEP, NB, W)),
                        ("index + 1", P.normal_idx(SEED, STEP, P.TAG_EPS, P.index(NB, W) + np.uint64(1)))):
        r = float(np.corrcoef(true.ravel(), other.ravel())[0, 1])
        assert abs(r) < 4 / np.sqrt(NB * W), name  # 4 sigma of the sample correlation of independent draws
