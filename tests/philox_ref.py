"""A numpy restatement of libhvae's random stream (not collected: no test_ prefix; numpy only).

Training never stores a dropout mask or the reparameterisation noise: every kernel that needs one draws it from the
counter-based Philox4x32-10 of csrc/hvae_common.h as a pure function of (seed, step, tag, element index), and each
backward kernel draws it again. tests/test_gpu_philox.py holds every drawing kernel, the executor and the module API
to this file bit for bit; tests/test_philox_reference_cpu.py pins this file itself, without a GPU, to the published
known-answer vectors of Philox4x32-10 and shows that each way of getting the stream wrong moves the mask.

The contract:

  counter  (idx & 0xffffffff, idx >> 32, step & 0xffffffff, tag)      key  (seed & 0xffffffff, seed >> 32)
  idx      row * width + col, with row the position in the batch (not the matrix row a `rows` list names)
  tag      TAG_ENC_DROP + hidden layer index | TAG_PROJ_DROP | TAG_EPS
  dropout  word 0 (x):  u = float32(x >> 8) * 2^-24;  keep = u >= float32(p);  mult = keep ? 1 / (1 - p) : 0
  noise    words 0 and 1:  a = ((x >> 8) + 1) 2^-24 in (0, 1],  b = (y >> 8) 2^-24;  sqrt(-2 ln a) cos(2 pi b)

All integer arithmetic is done in uint64 and masked to 32 bits, so nothing relies on wrap-around.
"""
from __future__ import annotations

import numpy as np

TAG_ENC_DROP = 0x100  # + hidden layer index
TAG_PROJ_DROP = 0x200
TAG_EPS = 0x300

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_KEY0, _KEY1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_2M24 = np.float32(2.0 ** -24)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 over broadcastable arrays of 32-bit words held in uint64 -> the four output words."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _KEY0) & _M32, (k1 + _KEY1) & _M32
    return c0, c1, c2, c3


def words(seed: int, step: int, tag: int, idx):
    """The four Philox words of element `idx` (array of non-negative integers) of stream (seed, step, tag)."""
    idx = _u64(idx)
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
    return philox4x32_10(idx & _M32, idx >> _S32, np.uint64(step), np.uint64(int(tag) & 0xFFFFFFFF),
                         np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))


def index(nb: int, width: int, ld: int | None = None):
    """[nb, width] element indices row * ld + col (ld = width: the contract; another ld only for mutation proofs)."""
    ld = width if ld is None else ld
    return (np.arange(nb, dtype=np.uint64)[:, None] * np.uint64(ld) + np.arange(width, dtype=np.uint64)[None, :])


def u01(x):
    """float32 uniform in [0, 1) from the top 24 bits of a word (exact: 24 bits fit a float32 mantissa)."""
    return (_u64(x) >> np.uint64(8)).astype(np.float32) * _2M24


def keep_idx(seed, step, tag, idx, p: float):
    p = float(p)
    idx = _u64(idx)
    if p <= 0.0:
        return np.ones(idx.shape, dtype=bool)
    if p >= 1.0:
        return np.zeros(idx.shape, dtype=bool)
    return u01(words(seed, step, tag, idx)[0]) >= np.float32(p)


def scale(p: float) -> np.float32:
    """The survivors' multiplier, computed in float32 as the launchers do (0 at p >= 1)."""
    p = np.float32(p)
    return np.float32(0.0) if p >= np.float32(1.0) else np.float32(1.0) / (np.float32(1.0) - p)


def keep(seed, step, tag, nb: int, width: int, p: float):
    """bool [nb, width]: the units that survive dropout."""
    return keep_idx(seed, step, tag, index(nb, width), p)


def mult(seed, step, tag, nb: int, width: int, p: float):
    """float32 [nb, width]: 0 or 1 / (1 - p)  (all 1 at p <= 0, all 0 at p >= 1)."""
    k = keep(seed, step, tag, nb, width, p)
    if float(p) <= 0.0:
        return np.ones(k.shape, dtype=np.float32)
    return np.where(k, scale(p), np.float32(0.0)).astype(np.float32)


def normal_idx(seed, step, tag, idx):
    """float64 Box-Muller normals of the given element indices."""
    x, y, _, _ = words(seed, step, tag, idx)
    a = ((x >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    b = (y >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(a)) * np.cos(2.0 * np.pi * b)


def normal32_idx(seed, step, tag, idx):
    """The same formula evaluated in float32 (the kernels' precision); its distance from normal_idx sets the bar of
    the GPU comparison."""
    x, y, _, _ = words(seed, step, tag, idx)
    one, two = np.float32(1.0), np.float32(2.0)
    a = ((x >> np.uint64(8)).astype(np.float32) + one) * _2M24
    b = (y >> np.uint64(8)).astype(np.float32) * _2M24
    # cos(pi t), t = 2 b, as a float32 cospi does it: the quarter-turn reduction is exact (t has 24 bits), so only
    # pi * r with |r| <= 1/4 is rounded
    t = two * b
    k = np.rint(two * t)
    x = np.float32(np.pi) * (t - np.float32(0.5) * k)
    c, s = np.cos(x), np.sin(x)
    cospi = np.choose(k.astype(np.int64) & 3, [c, -s, -c, s])
    return (np.sqrt(-two * np.log(a)) * cospi).astype(np.float32)


def normal(seed, step, nb: int, L: int, tag: int = TAG_EPS):
    """float64 [nb, L]: the reparameterisation noise."""
    return normal_idx(seed, step, tag, index(nb, L))


def normal32(seed, step, nb: int, L: int, tag: int = TAG_EPS):
    return normal32_idx(seed, step, tag, index(nb, L))


def normal_bar(seed, step, nb: int, L: int, factor: float = 8.0) -> float:
    """Absolute bar for a float32 kernel's noise against normal(): `factor` x the largest distance between the float32
    and the float64 evaluation of the formula over the same indices (numpy's float32 log, cos and sqrt are within
    1 ulp; a device's logf / cospif are allowed a few ulp more)."""
    return factor * float(np.abs(normal32(seed, step, nb, L).astype(np.float64) - normal(seed, step, nb, L)).max())
