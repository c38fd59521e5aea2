"""Which (precision, embedding width) pairs the streaming decoder serves, as libhvae's host code answers
(hvae_decoder_supported): 512- and 1024-wide item embeddings (distiluse / CLIP text towers; the "large"
sentence encoders) next to the widths served before. Needs only the built library, no GPU."""
import pytest

from hvae import _lib, ops

DTYPES = {"bf16": _lib.HVAE_BF16, "fp32": _lib.HVAE_F32, "fp8": _lib.HVAE_FP8}
BEFORE = {"bf16": (64, 128, 256, 384, 768), "fp32": (32, 64, 128, 256, 384), "fp8": (128, 256, 384, 768)}
NEW = {"bf16": (512, 1024), "fp32": (512,), "fp8": (512,)}
REFUSED = {"bf16": (96, 1000), "fp32": (768, 1024, 96, 1000), "fp8": (1024, 96, 1000)}


@pytest.mark.parametrize("precision", sorted(DTYPES))
def test_decoder_supported_widths(precision):
    dt = DTYPES[precision]
    for d in NEW[precision]:
        assert ops.decoder_supported(dt, d), (precision, d)
    for d in BEFORE[precision]:
        assert ops.decoder_supported(dt, d), (precision, d)
    for d in REFUSED[precision]:
        assert not ops.decoder_supported(dt, d), (precision, d)


@pytest.mark.parametrize("precision", sorted(DTYPES))
def test_no_other_width_appeared(precision):
    """The whole answer over 1 .. 1024 is the listed widths and nothing else."""
    got = [d for d in range(1, 1025) if ops.decoder_supported(DTYPES[precision], d)]
    assert got == sorted(BEFORE[precision] + NEW[precision])
