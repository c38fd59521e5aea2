"""The guest update's fit beside the decoder sweep, without a device: hvae_adam_guest_fit_calc (the pure host
arithmetic of hvae_adam_pending_guest_fits) on hand-computed cases, and k_adam_pending_guest's footprint read from
the built library's gfx950 code object -- at most 32 VGPRs, no scratch, no LDS: the registers are the whole point
of that kernel (csrc/hvae_adam_guest.hip)."""
import struct
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "recommendation-system_amd" / "hvae" / "libhvae.so"
SWEEP_LDS = 3 * 49152 + 2 * 2 * 32 * 80 + 4 * 64 * 4  # k_dec5_bf16's (csrc/hvae_dec5_shared.h LDS_BYTES)


@pytest.fixture(scope="module")
def fit():
    # the library cross-compiles without a GPU: its absence is a failed build, not a missing device
    assert LIB.exists(), f"{LIB} is not built (run __graft_entry__.build())"
    from hvae import _lib
    return _lib.lib().hvae_adam_guest_fit_calc


def test_fit_registers(fit):
    # two sweep waves of 234 registers are allocated 240 each: 32 of 512 stay free
    assert SWEEP_LDS == 158720
    assert fit(2, 234, SWEEP_LDS, 32, 0) == 1        # 240 + 240 + 32 = 512
    assert fit(2, 234, SWEEP_LDS, 26, 0) == 1        # 26 is allocated as 32
    assert fit(2, 234, SWEEP_LDS, 33, 0) == 0        # 33 is allocated as 40
    assert fit(2, 250, SWEEP_LDS, 8, 0) == 0         # 250 -> 256 each: nothing left
    assert fit(2, 240, SWEEP_LDS, 16, 0) == 2        # two guest waves of 16 in the free 32
    assert fit(2, 232, SWEEP_LDS, 24, 0) == 2        # 512 - 464 = 48


def test_fit_lds_is_the_limit(fit):
    # registers and wave slots leave room for two guest waves a SIMD; 5,120 B of LDS are free on the CU
    assert fit(2, 232, SWEEP_LDS, 24, 0) == 2
    assert 160 * 1024 - SWEEP_LDS == 5120
    assert fit(2, 232, SWEEP_LDS, 24, 8192) == 0     # a guest block's LDS does not fit at all
    assert fit(2, 232, SWEEP_LDS, 24, 1024) == 1     # five blocks' worth: one wave on each of the four SIMDs
    assert fit(2, 232, 161 * 1024, 24, 0) == 0       # a sweep that cannot be resident itself


def test_fit_wave_slots_are_the_limit(fit):
    # small kernels: registers would allow 58 guest waves, the 32 wave slots of a CU (8 a SIMD) allow 8 - sweep's
    assert fit(6, 8, 0, 8, 0) == 2
    assert fit(8, 8, 0, 8, 0) == 0
    assert fit(0, 0, 0, 8, 0) == 8


def test_fit_rejects_nonsense(fit):
    assert fit(2, 234, SWEEP_LDS, 0, 0) == 0
    assert fit(-1, 234, SWEEP_LDS, 32, 0) == 0


# ---- the code object's metadata: clang offload bundle -> gfx950 ELF -> NT_AMDGPU_METADATA note (msgpack)
def _unpack(b, i):
    """One msgpack value at b[i]: (value, next index). The subset AMDGPU metadata uses."""
    t = b[i]
    if t <= 0x7f:
        return t, i + 1
    if 0x80 <= t <= 0x8f or t in (0xde, 0xdf):
        n, i = (t & 15, i + 1) if t <= 0x8f else \
            (struct.unpack_from(">H", b, i + 1)[0], i + 3) if t == 0xde else (struct.unpack_from(">I", b, i + 1)[0], i + 5)
        d = {}
        for _ in range(n):
            k, i = _unpack(b, i)
            d[k], i = _unpack(b, i)
        return d, i
    if 0x90 <= t <= 0x9f or t in (0xdc, 0xdd):
        n, i = (t & 15, i + 1) if t <= 0x9f else \
            (struct.unpack_from(">H", b, i + 1)[0], i + 3) if t == 0xdc else (struct.unpack_from(">I", b, i + 1)[0], i + 5)
        a = []
        for _ in range(n):
            x, i = _unpack(b, i)
            a.append(x)
        return a, i
    if 0xa0 <= t <= 0xbf:
        n = t & 31
        return b[i + 1:i + 1 + n].decode(), i + 1 + n
    if t in (0xd9, 0xda, 0xdb, 0xc4, 0xc5, 0xc6):
        w = {0xd9: 1, 0xda: 2, 0xdb: 4, 0xc4: 1, 0xc5: 2, 0xc6: 4}[t]
        n = int.from_bytes(b[i + 1:i + 1 + w], "big")
        raw = b[i + 1 + w:i + 1 + w + n]
        return (raw.decode() if t >= 0xd9 else bytes(raw)), i + 1 + w + n
    if t == 0xc0:
        return None, i + 1
    if t in (0xc2, 0xc3):
        return t == 0xc3, i + 1
    if t in (0xcc, 0xcd, 0xce, 0xcf):
        w = 1 << (t - 0xcc)
        return int.from_bytes(b[i + 1:i + 1 + w], "big"), i + 1 + w
    if t in (0xd0, 0xd1, 0xd2, 0xd3):
        w = 1 << (t - 0xd0)
        return int.from_bytes(b[i + 1:i + 1 + w], "big", signed=True), i + 1 + w
    if t == 0xca:
        return struct.unpack_from(">f", b, i + 1)[0], i + 5
    if t == 0xcb:
        return struct.unpack_from(">d", b, i + 1)[0], i + 9
    if t >= 0xe0:
        return t - 256, i + 1
    raise ValueError(f"msgpack type {t:#x}")


def _elf_kernels(elf):
    """The .amdhsa.kernels list of one AMDGPU code object."""
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        return []
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3a)
    out = []
    for k in range(shnum):
        sh = shoff + k * shentsize
        sh_type, = struct.unpack_from("<I", elf, sh + 4)
        off, size = struct.unpack_from("<QQ", elf, sh + 0x18)
        if sh_type != 7:  # SHT_NOTE
            continue
        i = off
        while i + 12 <= off + size:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, i)
            name = elf[i + 12:i + 12 + namesz]
            d0 = i + 12 + (namesz + 3) // 4 * 4
            if ntype == 32 and name.startswith(b"AMDGPU"):  # NT_AMDGPU_METADATA
                md, _ = _unpack(elf, d0)
                out += md.get("amdhsa.kernels", [])
            i = d0 + (descsz + 3) // 4 * 4
    return out


def _library_kernels(path):
    blob = path.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kernels, at = [], blob.find(magic)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(magic))
        i = at + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, i)
            triple = blob[i + 24:i + 24 + tlen].decode(errors="replace")
            i += 24 + tlen
            if "gfx950" in triple and size:
                kernels += _elf_kernels(blob[at + off:at + off + size])
        at = blob.find(magic, at + 1)
    return kernels


def test_guest_kernel_footprint_in_the_built_library():
    assert LIB.exists(), f"{LIB} is not built (run __graft_entry__.build())"
    ks = _library_kernels(LIB)
    assert len(ks) > 50, "the library's gfx950 code objects were not found"
    guest = [k for k in ks if "k_adam_pending_guest" in k[".name"]]
    assert len(guest) == 1, [k[".name"] for k in guest]
    g = guest[0]
    assert g[".vgpr_count"] <= 32, g[".vgpr_count"]
    assert g.get(".agpr_count", 0) == 0
    assert g[".private_segment_fixed_size"] == 0
    assert g[".group_segment_fixed_size"] == 0
    assert g[".max_flat_workgroup_size"] == 64
    # the sweep it is written to sit beside: two waves a SIMD whose allocation leaves the guest's 32 registers
    sweep = [k for k in ks if "k_dec5_bf16ILb1" in k[".name"]]
    assert len(sweep) == 1
    alloc = (sweep[0][".vgpr_count"] + sweep[0].get(".agpr_count", 0) + 7) // 8 * 8
    assert 2 * alloc + 32 <= 512, sweep[0][".vgpr_count"]
