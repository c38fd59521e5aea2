"""The MPNet body of the SBERT item encoder on the device: attention with the relative-position bias
(hvae_sbert_attention_relbias) and the whole encoder against float64 truth, bitwise reproducibility, the zero table
against the unbiased kernel, the independence from the pass size, and compute_item_embeddings end to end.

Truth: tests/golden/mpnet.npz holds what transformers' MPNetModel and torch give in float64
(tests/golden/make_mpnet_fixture.py); the large arrays only at sampled rows, so every row is compared against
tests/mpnet_ref.py's float64 restatement, which test_mpnet_cpu.py pins to the fixture at 1e-12, and the sampled rows
against the fixture itself.

Bar: the maker also ran each computation with torch's CPU float32 operators and recorded their max |error| against
float64 (mpnet_meta.json fp32_ref_err_*). A device result may miss the truth by at most 8 x that, the margin of
tests/test_gpu_sbert.py.

Measured on an MI355X (max |device - float64| over every element, beside the bar):
  embeddings   h128 1.9e-7 (1.8e-6)   h384 2.6e-7 (1.2e-6)   h768 2.7e-7 (1.1e-6)
  hidden       h128 1.9e-5 (1.9e-4)   h384 2.8e-5 (2.1e-4)   h768 4.1e-5 (2.4e-4)
  attention    dh32 5.7e-6 (6.1e-5)   dh64 1.0e-5 (8.3e-5)
"""
import functools
import json

import numpy as np
import pytest
import torch

import mpnet_ref as M
import sbert_ref as R

pytestmark = pytest.mark.gpu
MARGIN = 8.0
SENTINEL = -12345.0


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.as_tensor(a, device=torch.device("cuda", 0))


def bar(key: str, case) -> float:
    return MARGIN * M.meta()[f"fp32_ref_err_{key}"][str(case)]


def check(name: str, got, want: np.ndarray, limit: float) -> None:
    got = got.cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name
    e = float(np.abs(got - want).max())
    print(f"{name}: max |device - float64| = {e:.3e}, bar {limit:.3e}")
    assert e <= limit, f"{name}: error {e:.3e} exceeds {limit:.3e}"


@functools.lru_cache(maxsize=None)
def model(name: str):
    """The config's synthetic model as the loader's record (no files)."""
    from src.preprocessing.sbert import SbertModel
    H, heads, _ = M.CONFIGS[name]
    return SbertModel(path=None, hidden_size=H, heads=heads, layers=M.LAYERS, intermediate_size=4 * H,
                      max_position=M.MAX_POS, layer_norm_eps=M.LN_EPS, max_seq_length=M.MAX_POS - M.POS_OFFSET,
                      do_lower_case=True, lower_text=False, vocab=M.vocab(), tensors=M.encoder_truth(name)[0],
                      model_type="mpnet")


@functools.lru_cache(maxsize=None)
def encoder(name: str):
    from src.preprocessing.sbert import SbertEncoder
    return SbertEncoder(model(name))


# --------------------------------------------------------------------------------------------------- kernel ----
@pytest.mark.parametrize("case", list(M.ATT_CASES))
def test_attention_relbias(case):
    """ctx has 16 rows more than T, pre-filled with a sentinel: rows from T on stay untouched and every row below T
    is written and checked. The table is drawn per delta, so an index that is off by one misses the bar."""
    from hvae import ops
    qkv, cu, heads, rel = M.attention_input(case)
    H, T = qkv.shape[1] // 3, int(cu[-1])
    pack = ops.SbertPack(np.zeros(T, np.int32), cu, torch.device("cuda", 0))
    ctx = torch.full((T + 16, H), SENTINEL, device="cuda")
    ops.sbert_attention(dev(qkv), pack, heads, ctx, dev(rel), M.REL_L)
    assert bool((ctx[T:] == SENTINEL).all()), "rows past T were written"
    assert not bool((ctx[:T] == SENTINEL).any()), "a row below T was left unwritten"
    check(f"attention_relbias {case}", ctx[:T], M.attention_truth(case), bar("attention", case))
    rows = R.sample_rows(cu)
    check(f"attention_relbias {case} fixture rows", ctx[dev(rows)], M.fixture()[f"att_{case}_rows"],
          bar("attention", case))
    again = torch.full((T + 16, H), SENTINEL, device="cuda")
    ops.sbert_attention(dev(qkv), pack, heads, again, dev(rel), M.REL_L)
    assert torch.equal(ctx, again)


@pytest.mark.parametrize("case", list(M.ATT_CASES))
def test_zero_table_equals_the_unbiased_kernel(case):
    """Adding 0 changes no score's value: with an all-zero table the result is bitwise hvae_sbert_attention's."""
    from hvae import ops
    qkv, cu, heads, rel = M.attention_input(case)
    H, T = qkv.shape[1] // 3, int(cu[-1])
    pack = ops.SbertPack(np.zeros(T, np.int32), cu, torch.device("cuda", 0))
    plain = torch.full((T + 16, H), SENTINEL, device="cuda")
    ops.sbert_attention(dev(qkv), pack, heads, plain)
    zero = torch.full((T + 16, H), SENTINEL, device="cuda")
    ops.sbert_attention(dev(qkv), pack, heads, zero, torch.zeros_like(dev(rel)), M.REL_L)
    assert torch.equal(plain, zero)


def test_wrapper_refuses_what_the_device_cannot_report():
    """Host side only: nothing is launched, ctx keeps its sentinel."""
    from hvae import ops
    device = torch.device("cuda", 0)
    pack = ops.SbertPack(np.zeros(70, np.int32), np.array([0, 5, 70]), device)
    qkv = torch.zeros(70, 3 * 64, device="cuda")
    ctx = torch.full((70, 64), SENTINEL, device="cuda")
    with pytest.raises(ValueError, match="longer than the relative-bias table"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(2, 2 * 64 - 1, device="cuda"), 64)
    with pytest.raises(ValueError, match=r"rel must be a contiguous float32 \[2, 255\]"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(2, 256, device="cuda"), 128)
    with pytest.raises(ValueError, match="rel must be a contiguous float32"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(255, 2, device="cuda").t(), 128)
    with pytest.raises(ValueError, match="rel must be a contiguous float32"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(2, 255, device="cuda", dtype=torch.float64), 128)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(2, 255), 128)
    with pytest.raises(ValueError, match="rel_len"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(2, 2 * 513 - 1, device="cuda"), 513)
    with pytest.raises(ValueError, match="together"):
        ops.sbert_attention(qkv, pack, 2, ctx, torch.zeros(2, 255, device="cuda"))
    assert bool((ctx == SENTINEL).all())


# --------------------------------------------------------------------------------------------------- encoder ----
@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_encoder(name):
    _, ids, cu, hidden, emb = M.encoder_truth(name)
    enc = encoder(name)
    h, e = enc.forward_packed(ids, cu)
    check(f"{name} embeddings", e, M.fixture()[f"{name}_emb"], bar("embedding", name))
    check(f"{name} embeddings (restatement)", e, emb, bar("embedding", name))
    check(f"{name} hidden", h, hidden, bar("hidden", name))
    check(f"{name} hidden fixture rows", h[dev(R.sample_rows(cu))], M.fixture()[f"{name}_hidden_rows"],
          bar("hidden", name))
    h2, e2 = enc.forward_packed(ids, cu)
    assert torch.equal(h, h2) and torch.equal(e, e2)


def test_pass_size_does_not_matter():
    """The same sequences in passes of 3, of 4 (in reversed order) and of 11: each result, put back in input order,
    is within the embedding bar of the one float64 truth."""
    name = "h384"
    _, ids, cu, _, _ = M.encoder_truth(name)
    seqs = [ids[cu[s]:cu[s + 1]].tolist() for s in range(len(cu) - 1)]
    enc = encoder(name)
    want = M.fixture()[f"{name}_emb"]
    for bs in (3, 11):
        check(f"passes of {bs}", enc.encode_ids(seqs, batch_size=bs), want, bar("embedding", name))
    order = list(reversed(range(len(seqs))))
    check("reversed order", enc.encode_ids([seqs[i] for i in order], batch_size=4), want[order],
          bar("embedding", name))


def test_compute_item_embeddings(tmp_path):
    from src.preprocessing import embeddings as E
    model_dir = M.write_model_dir(tmp_path / "models" / "tiny-mpnet", "h128", max_seq_length=64)
    g = np.random.default_rng(5)
    asins = [f"B{g.integers(0, 25):04d}" for _ in range(40)]  # duplicates, unsorted
    asins[3], asins[7] = "B9000", "A0001"                     # the empty and the over-long text: one row each
    words = "toy game play great kids fun puzzle train wooden set love super car box".split()
    rows = []
    for i, a in enumerate(asins):
        text = " ".join(g.choice(words, size=int(g.integers(1, 30))))
        if i == 3:
            text = ""
        if i == 7:
            text = "super toy " * 400  # over 2048 characters and over max_seq_length
        rows.append({"asin": a, "item_text": text, "n": i})
    src = tmp_path / "items.jsonl"
    src.write_text("".join(json.dumps(r) + "\n" for r in rows))
    out = tmp_path / "emb" / "item_embeddings.npy"
    E.compute_item_embeddings(src, out, model_name=str(model_dir), batch_size=7)

    emb = np.load(out)
    uniq = sorted(set(asins))
    assert emb.shape == (len(uniq), 128) and emb.dtype == np.float32
    assert np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1.0).max() <= 1e-6

    # the first text per asin wins, and each row is that text's float64 embedding
    from src.preprocessing.sbert import load_model_dir
    m = load_model_dir(model_dir)
    tok = m.tokenizer()
    gen = E.ItemEmbeddingGenerator.__new__(E.ItemEmbeddingGenerator)
    first = {}
    for r in rows:
        first.setdefault(r["asin"], r["item_text"])
    seqs = [tok.encode(t) for t in gen._preprocess_text([first[a] for a in uniq])]
    assert max(len(s) for s in seqs) == 64 and all(s[0] == 0 and s[-1] == 2 for s in seqs)
    cu = R.cu_of([len(s) for s in seqs])
    want = M.encode(m.tensors, m.heads, np.concatenate(seqs), cu)[1]
    check("compute_item_embeddings", emb, want, bar("embedding", "h128"))
