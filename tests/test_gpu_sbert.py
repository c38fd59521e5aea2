"""The SBERT item encoder on the device (K22): each kernel and the whole encoder against float64 truth, bitwise
reproducibility, the independence from the pass size, and compute_item_embeddings end to end.

Truth: tests/golden/sbert.npz holds what transformers' BertModel and torch give in float64
(tests/golden/make_sbert_fixture.py); the large arrays only at sampled rows, so every row is compared against
tests/sbert_ref.py's float64 restatement, which test_sbert_cpu.py pins to the fixture at 1e-12, and the sampled rows
against the fixture itself.

Bar: the maker also ran each computation with torch's CPU float32 operators and recorded their max |error| against
float64 (sbert_meta.json fp32_ref_err_*). A device result may miss the truth by at most 8 x that: the margin for
another summation order (MFMA k-chains against blocked BLAS sums) and the fast exponential of the softmax.

Measured on an MI355X (max |device - float64| over every element, beside the bar):
  embeddings   h384 2.1e-7 (1.0e-6)   h768 2.5e-7 (1.0e-6)   h128 1.4e-7 (1.4e-6)
  hidden       h384 2.1e-5 (1.3e-4)   h768 3.1e-5 (2.0e-4)   h128 1.9e-5 (1.6e-4)
  attention    dh32 7.4e-6 (7.4e-5)   dh64 8.5e-6 (7.8e-5)
  add + LN     at most 5.6e-7 (1.7e-6 .. 4.2e-6)   embed + LN 5.4e-7 (4.6e-6)   pooling at most 2.4e-8 (1.3e-7 .. 3.4e-7)
"""
import functools
import json
import pickle

import numpy as np
import pytest
import torch

import sbert_ref as R

pytestmark = pytest.mark.gpu
MARGIN = 8.0


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.as_tensor(a, device=torch.device("cuda", 0))


def bar(key: str, case) -> float:
    return MARGIN * R.meta()[f"fp32_ref_err_{key}"][str(case)]


def check(name: str, got, want: np.ndarray, limit: float) -> None:
    got = got.cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name
    e = float(np.abs(got - want).max())
    print(f"{name}: max |device - float64| = {e:.3e}, bar {limit:.3e}")
    assert e <= limit, f"{name}: error {e:.3e} exceeds {limit:.3e}"


@functools.lru_cache(maxsize=None)
def model_and_truth(name: str):
    """The config's synthetic model as the loader's record (no files), its ids and the restatement's float64 result."""
    from src.preprocessing.sbert import SbertModel
    H, heads, _ = R.CONFIGS[name]
    w = R.weights(name)
    vocab = (R.GOLDEN / "sbert_vocab.txt").read_text(encoding="utf-8").split("\n")[:-1]
    model = SbertModel(path=None, hidden_size=H, heads=heads, layers=R.LAYERS, intermediate_size=4 * H,
                       max_position=R.MAX_POS, layer_norm_eps=R.LN_EPS, max_seq_length=R.MAX_POS, do_lower_case=True,
                       lower_text=False, vocab=vocab, tensors=w)
    ids, cu = R.encoder_ids(name)
    hidden, emb = R.encode(w, heads, ids, cu)
    return model, ids, cu, hidden, emb


@functools.lru_cache(maxsize=None)
def encoder(name: str):
    from src.preprocessing.sbert import SbertEncoder
    return SbertEncoder(model_and_truth(name)[0])


# --------------------------------------------------------------------------------------------------- kernels ----
def test_embed_ln():
    from hvae import ops
    d = R.embed_input()
    pack = ops.SbertPack(d["ids"], d["cu"], torch.device("cuda", 0))
    got = ops.sbert_embed_ln(pack, dev(d["word"]), dev(d["pos"]), dev(d["type0"]), dev(d["w"]), dev(d["b"]), R.LN_EPS)
    want = R.embed_ln(d["ids"], d["cu"], d["word"], d["pos"], d["type0"], d["w"], d["b"])
    check("embed_ln", got, want, bar("embed_ln", R.EMB_H))
    rows = R.sample_rows(d["cu"])
    check("embed_ln fixture rows", got[dev(rows)], R.fixture()["embed_rows"], bar("embed_ln", R.EMB_H))


@pytest.mark.parametrize("H", R.LN_WIDTHS)
def test_add_ln(H):
    from hvae import ops
    d = R.ln_input(H)
    x, res = dev(d["x"]), dev(d["res"])
    got = ops.sbert_add_ln(x, res, dev(d["w"]), dev(d["b"]), R.LN_EPS)
    check(f"add_ln {H}", got, R.fixture()[f"ln_{H}"], bar("ln", H))
    inplace = ops.sbert_add_ln(x, res, dev(d["w"]), dev(d["b"]), R.LN_EPS, out=x)
    assert torch.equal(inplace, got)


@pytest.mark.parametrize("case", list(R.ATT_CASES))
def test_attention(case):
    """ctx has 16 rows more than T, pre-filled with a sentinel: rows from T on stay untouched (a tail chunk's queries
    past the sequence's end are the next sequence's rows, or past the buffer) and every row below T is checked."""
    from hvae import ops
    qkv, cu, heads = R.attention_input(case)
    H = qkv.shape[1] // 3
    T = int(cu[-1])
    pack = ops.SbertPack(np.zeros(T, np.int32), cu, torch.device("cuda", 0))
    sentinel = -12345.0
    ctx = torch.full((T + 16, H), sentinel, device="cuda")
    ops.sbert_attention(dev(qkv), pack, heads, ctx)
    assert bool((ctx[T:] == sentinel).all()), "rows past T were written"
    assert not bool((ctx[:T] == sentinel).any()), "a row below T was left unwritten"
    check(f"attention {case}", ctx[:T], R.attention(qkv, cu, heads), bar("attention", case))
    rows = R.sample_rows(cu)
    check(f"attention {case} fixture rows", ctx[dev(rows)], R.fixture()[f"att_{case}_rows"], bar("attention", case))
    again = torch.full((T + 16, H), sentinel, device="cuda")
    ops.sbert_attention(dev(qkv), pack, heads, again)
    assert torch.equal(ctx, again)


@pytest.mark.parametrize("H", R.LN_WIDTHS[1:])
def test_pool_norm(H):
    from hvae import ops
    x, cu = R.pool_input(H)
    pack = ops.SbertPack(np.zeros(int(cu[-1]), np.int32), cu, torch.device("cuda", 0))
    got = ops.sbert_pool_norm(dev(x), pack)
    check(f"pool_norm {H}", got, R.fixture()[f"pool_{H}"], bar("pool", H))


def test_wrappers_refuse_what_the_device_cannot_report():
    from hvae import ops
    d = R.embed_input()
    device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="increase strictly"):
        ops.SbertPack(np.zeros(4, np.int32), np.array([0, 3, 2, 4]), device)
    with pytest.raises(ValueError, match="513 tokens"):
        ops.SbertPack(np.zeros(513, np.int32), np.array([0, 513]), device)
    with pytest.raises(ValueError, match="outside"):
        ops.SbertPack(np.array([1, -1], np.int32), np.array([0, 2]), device)
    pack = ops.SbertPack(np.array([1, R.EMB_VOCAB], np.int32), np.array([0, 2]), device)
    args = (dev(d["type0"]), dev(d["w"]), dev(d["b"]), R.LN_EPS)
    with pytest.raises(ValueError, match="outside"):
        ops.sbert_embed_ln(pack, dev(d["word"]), dev(d["pos"]), *args)
    pack = ops.SbertPack(np.zeros(5, np.int32), np.array([0, 5]), device)
    with pytest.raises(ValueError, match="position table"):
        ops.sbert_embed_ln(pack, dev(d["word"]), dev(d["pos"][:4]), *args)
    with pytest.raises(ValueError, match="not served"):
        ops.sbert_attention(torch.zeros(5, 3 * 48, device="cuda"), pack, 1)


# --------------------------------------------------------------------------------------------------- encoder ----
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_encoder(name):
    _, ids, cu, hidden, emb = model_and_truth(name)
    enc = encoder(name)
    h, e = enc.forward_packed(ids, cu)
    check(f"{name} embeddings", e, R.fixture()[f"{name}_emb"], bar("embedding", name))
    check(f"{name} embeddings (restatement)", e, emb, bar("embedding", name))
    check(f"{name} hidden", h, hidden, bar("hidden", name))
    check(f"{name} hidden fixture rows", h[dev(R.sample_rows(cu))], R.fixture()[f"{name}_hidden_rows"],
          bar("hidden", name))
    h2, e2 = enc.forward_packed(ids, cu)
    assert torch.equal(h, h2) and torch.equal(e, e2)


def test_pass_size_does_not_matter():
    """The same sequences in passes of 3, of 4 (in reversed order) and of 11 (all at once): each result, put back in
    input order, is within the embedding bar of the one float64 truth. That is what is asserted; it bounds the
    difference between any two pass sizes at twice the bar. They are not compared bitwise, because the GEMM's split
    choice may differ with T."""
    name = "h384"
    _, ids, cu, _, _ = model_and_truth(name)
    seqs = [ids[cu[s]:cu[s + 1]].tolist() for s in range(len(cu) - 1)]
    enc = encoder(name)
    want = R.fixture()[f"{name}_emb"]
    for bs in (3, 11):
        check(f"passes of {bs}", enc.encode_ids(seqs, batch_size=bs), want, bar("embedding", name))
    order = list(reversed(range(len(seqs))))
    check("reversed order", enc.encode_ids([seqs[i] for i in order], batch_size=4), want[order],
          bar("embedding", name))


def test_compute_item_embeddings(tmp_path):
    from src.preprocessing import embeddings as E
    model_dir = R.write_model_dir(tmp_path / "models" / "tiny-bert", "h128", max_seq_length=64)
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
    with open(out.with_name("item_embeddings_mappings.pkl"), "rb") as f:
        maps = pickle.load(f)
    assert set(maps) == {"item_to_idx", "idx_to_item", "embedding_dim", "model_name", "n_items"}
    assert [maps["idx_to_item"][i] for i in range(len(uniq))] == uniq and maps["n_items"] == len(uniq)
    assert maps["embedding_dim"] == 128 and maps["model_name"] == str(model_dir)
    meta = out.with_name("item_embeddings_metadata.txt").read_text()
    assert [ln.split(":")[0] for ln in meta.splitlines()] == ["Model", "Dimension", "Items", "Shape", "Device"]

    # the first text per asin wins, and each row is that text's float64 embedding
    from src.preprocessing.sbert import load_model_dir
    model = load_model_dir(model_dir)
    tok = model.tokenizer()
    gen = E.ItemEmbeddingGenerator.__new__(E.ItemEmbeddingGenerator)
    first = {}
    for r in rows:
        first.setdefault(r["asin"], r["item_text"])
    seqs = [tok.encode(t) for t in gen._preprocess_text([first[a] for a in uniq])]
    assert max(len(s) for s in seqs) == 64 and seqs[uniq.index(asins[3])] == tok.encode("[NO TEXT]")
    cu = R.cu_of([len(s) for s in seqs])
    want = R.encode(model.tensors, model.heads, np.concatenate(seqs), cu)[1]
    check("compute_item_embeddings", emb, want, bar("embedding", "h128"))
    # by name under SBERT_MODEL_DIR
    E.config.SBERT_MODEL_DIR, saved = str(tmp_path / "models"), E.config.SBERT_MODEL_DIR
    try:
        assert E.resolve_model_dir("sentence-transformers/tiny-bert") == tmp_path / "models" / "tiny-bert"
    finally:
        E.config.SBERT_MODEL_DIR = saved
