"""The SBERT item encoder's host side, without a GPU: the WordPiece tokenizer against transformers' recorded ids, the
text preprocessing, the model-directory loader and its refusals, the float64 restatement against the fixture, the
command line, the no-fetch guarantee, and the K22 contract (header, bindings, ABI, Makefile)."""
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sbert_ref as R

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "recommendation-system_amd"
NETWORK_MODULES = ("transformers", "tokenizers", "sentence_transformers", "huggingface_hub", "safetensors")
K22 = ("hvae_sbert_supported", "hvae_sbert_embed_ln", "hvae_sbert_add_ln", "hvae_sbert_attention",
       "hvae_sbert_pool_norm")


def vocab() -> list[str]:
    return (R.GOLDEN / "sbert_vocab.txt").read_text(encoding="utf-8").split("\n")[:-1]


# ------------------------------------------------------------------------------------------------ tokenizer ----
TOK_KEYS = sorted(R.meta()["tokenizer_ids"])


@pytest.mark.parametrize("key", TOK_KEYS)
@pytest.mark.parametrize("case", range(len(R.meta()["tokenizer_cases"])))
def test_tokenizer_equals_bert_tokenizer(key, case):
    from src.preprocessing.sbert import WordPieceTokenizer
    m = R.meta()
    max_len = m["truncate_at"] if "max" in key else 512
    tok = WordPieceTokenizer(vocab(), do_lower_case=key.startswith("lower"), max_seq_length=max_len)
    text, want = m["tokenizer_cases"][case], m["tokenizer_ids"][key][case]
    assert tok.encode(text) == want, text
    assert len(want) <= max_len


def test_tokenizer_cases_cover_the_awkward_inputs():
    m = R.meta()
    ids = dict(zip(m["tokenizer_cases"], m["tokenizer_ids"]["lower"]))
    v = vocab()
    unk, sep = v.index("[UNK]"), v.index("[SEP]")
    assert ids["[NO TEXT]"] == [2, v.index("["), v.index("no"), v.index("text"), v.index("]"), 3]
    assert ids[""] == [2, 3] and ids["   "] == [2, 3]
    assert ids["x" * 120 + " play"] == [2, unk, v.index("play"), 3]
    assert ids["Café résumé naïve"] == [2, v.index("cafe"), v.index("resume"), v.index("naive"), 3]
    literal = ids["first part [SEP] second part [CLS][MASK] [UNK] [PAD] [sep]"]
    assert literal.count(sep) == 2 and v.index("[MASK]") in literal
    assert max(len(x) for x in m["tokenizer_ids"][f"lower_max{m['truncate_at']}"]) == m["truncate_at"]


def test_preprocess_text():
    from src.preprocessing.embeddings import MAX_CHARS, ItemEmbeddingGenerator
    gen = ItemEmbeddingGenerator.__new__(ItemEmbeddingGenerator)
    long = "ab " * 1000
    got = gen._preprocess_text([float("nan"), None, "", "  a \t b\n\nc  ", long, "x" * MAX_CHARS, np.float64("nan")])
    assert got[:4] == ["[NO TEXT]", "[NO TEXT]", "[NO TEXT]", "a b c"]
    assert got[4] == " ".join(long.split())[:MAX_CHARS] + "..." and len(got[4]) == MAX_CHARS + 3
    assert got[5] == "x" * MAX_CHARS and got[6] == "[NO TEXT]"
    import pandas as pd
    assert gen._preprocess_text([pd.NA]) == ["[NO TEXT]"]


# --------------------------------------------------------------------------------------------------- loader ----
@pytest.mark.parametrize("fmt,prefix", [("safetensors", ""), ("safetensors", "bert."), ("bin", ""), ("bin", "bert.")])
def test_model_dir_round_trip(tmp_path, fmt, prefix):
    from src.preprocessing.sbert import load_model_dir
    d = R.write_model_dir(tmp_path / "m", "h128", fmt=fmt, prefix=prefix, max_seq_length=200, do_lower_case=False)
    m = load_model_dir(d)
    w = R.weights("h128")
    assert set(m.tensors) == set(w)  # pooler.* and embeddings.position_ids are ignored
    assert all(m.tensors[k].dtype == np.float32 and np.array_equal(m.tensors[k], w[k]) for k in w)
    assert (m.hidden_size, m.heads, m.layers, m.intermediate_size, m.max_position) == (128, 4, 2, 512, 512)
    assert m.max_seq_length == 200 and m.do_lower_case is False and m.vocab == vocab()
    assert m.tokenizer().encode("Toy") == [2, vocab().index("Toy"), 3]


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_ignored_tensors_may_have_any_dtype_and_wanted_ones_may_not(tmp_path, fmt):
    """embeddings.position_ids is an int64 buffer in BertModel's checkpoints: it is skipped before any dtype check.
    A tensor the encoder reads is refused by name when it is not floating point."""
    from src.preprocessing.sbert import load_model_dir
    d = R.write_model_dir(tmp_path / "ok", "h128", fmt=fmt)
    if fmt == "safetensors":
        import struct
        raw = (d / "model.safetensors").read_bytes()
        (n,) = struct.unpack("<Q", raw[:8])
        assert json.loads(raw[8:8 + n])["embeddings.position_ids"]["dtype"] == "I64"
    else:
        import torch
        assert torch.load(d / "pytorch_model.bin", weights_only=True)["embeddings.position_ids"].dtype == torch.int64
    assert "embeddings.position_ids" not in load_model_dir(d).tensors
    w = R.weights("h128")
    w["encoder.layer.0.output.dense.bias"] = np.zeros(128, np.int64)
    d = R.write_model_dir(tmp_path / "bad", "h128", fmt=fmt, weights_=w)
    with pytest.raises(ValueError, match="encoder.layer.0.output.dense.bias.*dtype"):
        load_model_dir(d)


@pytest.mark.parametrize("field,cfg", [("strip_accents", {"strip_accents": False}),
                                       ("tokenize_chinese_chars", {"tokenize_chinese_chars": False})])
def test_loader_refuses_tokenizer_settings_by_field(tmp_path, field, cfg):
    from src.preprocessing.sbert import load_model_dir
    with pytest.raises(ValueError, match=field):
        load_model_dir(R.write_model_dir(tmp_path / "m", "h128", tokenizer_config=cfg))
    ok = {"strip_accents": None, "tokenize_chinese_chars": True}
    load_model_dir(R.write_model_dir(tmp_path / "ok", "h128", tokenizer_config=ok))


def test_model_dir_without_the_optional_files(tmp_path):
    from src.preprocessing.sbert import load_model_dir
    m = load_model_dir(R.write_model_dir(tmp_path / "m", "h128", extras=False))
    assert m.max_seq_length == 512 and m.do_lower_case is True and m.lower_text is False


def test_safetensors_half_precisions(tmp_path):
    from src.preprocessing.sbert import read_safetensors
    g = np.random.default_rng(3)
    a = g.standard_normal((5, 7)).astype(np.float32)
    bf = (a.view(np.uint32) >> 16).astype(np.uint16)  # truncated bfloat16
    R.write_safetensors(tmp_path / "x.safetensors", {"f32": a, "f16": a.astype(np.float16), "bf16": bf})
    got = read_safetensors(tmp_path / "x.safetensors")
    assert np.array_equal(got["f32"], a)
    assert np.array_equal(got["f16"], a.astype(np.float16).astype(np.float32))
    assert np.array_equal(got["bf16"], (bf.astype(np.uint32) << 16).view(np.float32))
    assert all(v.dtype == np.float32 and v.shape == (5, 7) for v in got.values())


def _refusal(tmp_path, field, **change):
    from src.preprocessing.sbert import load_model_dir
    cfg = R.config_json("h128")
    cfg.update(change)
    d = R.write_model_dir(tmp_path / "m", "h128", config=cfg)
    with pytest.raises(ValueError, match=field):
        load_model_dir(d)


@pytest.mark.parametrize("field,change", [
    ("model_type", {"model_type": "mpnet"}),
    ("position_embedding_type", {"position_embedding_type": "relative_key"}),
    ("hidden_act", {"hidden_act": "relu"}),
    ("num_attention_heads", {"num_attention_heads": 8}),   # head width 16
    ("hidden_size", {"hidden_size": 2048, "num_attention_heads": 32}),
])
def test_loader_refuses_by_field(tmp_path, field, change):
    _refusal(tmp_path, field, **change)


def test_loader_refuses_pooling_length_and_missing_tensor(tmp_path):
    from src.preprocessing.sbert import load_model_dir
    d = R.write_model_dir(tmp_path / "cls", "h128")
    (d / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": True,
                                                             "pooling_mode_mean_tokens": False}))
    with pytest.raises(ValueError, match="pooling_mode"):
        load_model_dir(d)
    cfg = R.config_json("h128")
    cfg["max_position_embeddings"] = 1024
    w = R.weights("h128")
    w["embeddings.position_embeddings.weight"] = np.zeros((1024, 128), np.float32)
    d = R.write_model_dir(tmp_path / "long", "h128", config=cfg, weights_=w, max_seq_length=1024)
    with pytest.raises(ValueError, match="max_seq_length"):
        load_model_dir(d)
    w = R.weights("h128")
    del w["encoder.layer.1.output.dense.bias"]
    d = R.write_model_dir(tmp_path / "missing", "h128", weights_=w)
    with pytest.raises(ValueError, match="encoder.layer.1.output.dense.bias"):
        load_model_dir(d)


# ---------------------------------------------------------------------------------------------- restatement ----
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_restatement_equals_transformers(name):
    H, heads, _ = R.CONFIGS[name]
    ids, cu = R.encoder_ids(name)
    f = R.fixture()
    assert np.array_equal(ids, f[f"{name}_ids"]) and np.array_equal(cu, f[f"{name}_cu"])
    hidden, emb = R.encode(R.weights(name), heads, ids, cu)
    assert np.abs(emb - f[f"{name}_emb"]).max() <= 1e-12
    assert np.abs(hidden[R.sample_rows(cu)] - f[f"{name}_hidden_rows"]).max() <= 1e-12
    assert R.meta()["logit_row_std"][name] >= 1.0


def test_kernel_restatements_equal_torch():
    f = R.fixture()
    for case in R.ATT_CASES:
        qkv, cu, heads = R.attention_input(case)
        assert np.abs(R.attention(qkv, cu, heads)[R.sample_rows(cu)] - f[f"att_{case}_rows"]).max() <= 1e-12
    for H in R.LN_WIDTHS:
        d = R.ln_input(H)
        got = R.layer_norm(d["x"].astype(np.float64) + d["res"].astype(np.float64), d["w"], d["b"])
        assert np.abs(got - f[f"ln_{H}"]).max() <= 1e-12
    d = R.embed_input()
    got = R.embed_ln(d["ids"], d["cu"], d["word"], d["pos"], d["type0"], d["w"], d["b"])
    assert np.abs(got[R.sample_rows(d["cu"])] - f["embed_rows"]).max() <= 1e-12
    for H in R.LN_WIDTHS[1:]:
        x, cu = R.pool_input(H)
        assert np.abs(R.pool_norm(x, cu) - f[f"pool_{H}"]).max() <= 1e-12


def test_fixture_records_every_error_bar():
    m = R.meta()
    for key, cases in (("embedding", R.CONFIGS), ("hidden", R.CONFIGS), ("attention", R.ATT_CASES),
                       ("ln", R.LN_WIDTHS), ("pool", R.LN_WIDTHS[1:])):
        for c in cases:
            assert 0.0 < m[f"fp32_ref_err_{key}"][str(c)] < 1e-3
    assert (R.GOLDEN / "sbert.npz").stat().st_size < 1 << 20


# ------------------------------------------------------------------------------------------- command line ----
def test_cli_accepts_the_reference_flags():
    from src.preprocessing.embeddings import build_parser
    a = build_parser().parse_args(["--input", "in.jsonl", "--output", "o.npy", "--model", "m", "--text-column", "t",
                                   "--item-column", "i", "--batch-size", "8", "--device", "cuda"])
    assert (a.input, a.output, a.model, a.text_column, a.item_column, a.batch_size, a.device) == \
        ("in.jsonl", "o.npy", "m", "t", "i", 8, "cuda")
    d = build_parser().parse_args([])
    assert (d.model, d.text_column, d.item_column, d.batch_size, d.device) == \
        ("all-MiniLM-L6-v2", "item_text", "asin", 32, None)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--device", "tpu"])


def test_missing_model_raises_without_any_network_import(tmp_path):
    code = f"""
import sys
sys.path[:0] = [{str(PKG)!r}]
from src.preprocessing import embeddings as E
try:
    E.ItemEmbeddingGenerator("sentence-transformers/all-MiniLM-L6-v2")
except FileNotFoundError as e:
    msg = str(e)
else:
    raise SystemExit("no FileNotFoundError")
assert "Nothing is fetched" in msg and "all-MiniLM-L6-v2" in msg and {str(tmp_path / "sbert")!r} in msg, msg
try:
    E.ItemEmbeddingGenerator("x", device="cpu")
except RuntimeError as e:
    assert "no CPU fallback" in str(e)
else:
    raise SystemExit("device='cpu' was accepted")
from src.preprocessing import sbert
bad = [m for m in {NETWORK_MODULES!r} if m in sys.modules]
assert not bad, bad
print("ok")
"""
    import os
    env = dict(os.environ, SBERT_MODEL_DIR=str(tmp_path / "sbert"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_sources_name_no_network_module():
    for p in (PKG / "src" / "preprocessing" / "sbert.py", PKG / "src" / "preprocessing" / "embeddings.py"):
        text = p.read_text()
        for m in NETWORK_MODULES:
            assert not re.search(rf"^\s*(import|from)\s+{m}\b", text, re.M), (p.name, m)


# ------------------------------------------------------------------------------------------------ contract ----
def test_header_bindings_abi_and_makefile():
    from hvae import _lib
    header = (ROOT / "include" / "hvae.h").read_text()
    assert "(K22)" in header and re.search(r"#define HVAE_ABI_VERSION\s+6\b", header)
    assert _lib.ABI_VERSION == 6
    for name in K22:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
    assert (PKG / "csrc" / "hvae_sbert.hip").exists()
    mk = (PKG / "Makefile").read_text()
    assert re.search(r"^embeddings: lib$", mk, re.M)
    assert "-m src.preprocessing.embeddings --input $(DATA_DIR)/cleaned_reviews.jsonl " \
           "--output $(EMBEDDINGS_DIR)/item_embeddings.npy --model $(EMBEDDING_MODEL)" in mk


def test_supported_is_host_arithmetic():
    from hvae import _lib
    f = _lib.lib().hvae_sbert_supported
    assert f(384, 12, 256) and f(768, 12, 512) and f(1024, 16, 1) and f(128, 4, 128)
    assert not f(384, 12, 513) and not f(384, 24, 128) and not f(2048, 32, 128) and not f(384, 12, 0)
    assert not f(96, 1, 128) and not f(384, 0, 128) and not f(100, 3, 128)
