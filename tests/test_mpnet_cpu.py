"""The MPNet body of the SBERT item encoder, host side, without a GPU: the float64 restatement and the bucket rule
against transformers' records, the tokenizer against MPNetTokenizer's recorded ids, the model-directory loader and its
refusals, and the contract of hvae_sbert_attention_relbias (header, bindings, ABI)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import mpnet_ref as M
import sbert_ref as R

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "recommendation-system_amd"


# ---------------------------------------------------------------------------------------------- restatement ----
@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_restatement_equals_transformers(name):
    _, ids, cu, hidden, emb = M.encoder_truth(name)
    f = M.fixture()
    assert np.array_equal(ids, f[f"{name}_ids"]) and np.array_equal(cu, f[f"{name}_cu"])
    assert tuple(np.diff(cu)) == M.SEQ_LENS
    assert np.abs(emb - f[f"{name}_emb"]).max() <= 1e-12
    assert np.abs(hidden[R.sample_rows(cu)] - f[f"{name}_hidden_rows"]).max() <= 1e-12
    assert M.meta()["logit_row_std"][name] >= 1.0


@pytest.mark.parametrize("case", list(M.ATT_CASES))
def test_attention_restatement_equals_torch(case):
    cu = M.attention_input(case)[1]
    assert np.abs(M.attention_truth(case)[R.sample_rows(cu)] - M.fixture()[f"att_{case}_rows"]).max() <= 1e-12


def test_bucket_rule_equals_the_recorded_table():
    from src.preprocessing.sbert import relative_bias_table, relative_position_bucket
    table = M.fixture()["bucket_table"].astype(np.int64)
    delta = np.arange(-(M.REL_L - 1), M.REL_L)
    assert table.shape == delta.shape and table.min() == 0 and table.max() == 31
    assert np.array_equal(relative_position_bucket(delta), table)
    assert np.array_equal(M.bucket(delta), table)
    # both saturated buckets are reached from 130 tokens on, and the sign convention is key - query
    assert table[delta == 129][0] == 31 and table[delta == -129][0] == 15
    assert table[delta == 1][0] == 17 and table[delta == -1][0] == 1 and table[delta == 0][0] == 0
    w = M.weights("h128")["encoder.relative_attention_bias.weight"]
    for L in (1, 2, 130, 512):
        rel = relative_bias_table(w, L)
        assert rel.dtype == np.float32 and rel.shape == (4, 2 * L - 1) and rel.flags.c_contiguous
        assert np.array_equal(rel.astype(np.float64), M.rel_table(w, L))
        assert np.array_equal(rel[:, L - 1], w[0])  # delta 0 is bucket 0
    with pytest.raises(ValueError, match="relative_bias_table"):
        relative_bias_table(w[:31], 8)


def test_fixture_records_every_error_bar():
    m = M.meta()
    for key, cases in (("embedding", M.CONFIGS), ("hidden", M.CONFIGS), ("attention", M.ATT_CASES)):
        for c in cases:
            assert 0.0 < m[f"fp32_ref_err_{key}"][str(c)] < 1e-3
    size = sum((M.GOLDEN / n).stat().st_size for n in ("mpnet.npz", "mpnet_meta.json", "mpnet_vocab.txt"))
    assert size < 1 << 20


# ------------------------------------------------------------------------------------------------ tokenizer ----
TOK_KEYS = sorted(M.meta()["tokenizer_ids"])


def mpnet_tokenizer(lower: bool, max_len: int):
    from src.preprocessing.sbert import SPECIALS, WordPieceTokenizer
    return WordPieceTokenizer(M.vocab(), do_lower_case=lower, max_seq_length=max_len, **SPECIALS["mpnet"])


@pytest.mark.parametrize("key", TOK_KEYS)
@pytest.mark.parametrize("case", range(len(M.meta()["tokenizer_cases"])))
def test_tokenizer_equals_mpnet_tokenizer(key, case):
    m = M.meta()
    max_len = m["truncate_at"] if "max" in key else 512
    tok = mpnet_tokenizer(key.startswith("lower"), max_len)
    text, want = m["tokenizer_cases"][case], m["tokenizer_ids"][key][case]
    assert tok.encode(text) == want, text
    assert len(want) <= max_len and want[0] == 0 and want[-1] == 2


def test_tokenizer_cases_cover_the_special_tokens():
    m = M.meta()
    v = M.vocab()
    assert [v.index(t) for t in (M.CLS, M.PAD, M.SEP, M.UNK_ALT, M.UNK)] == [0, 1, 2, 3, 4] and v[-1] == M.MASK
    ids = dict(zip(m["tokenizer_cases"], m["tokenizer_ids"]["lower"]))
    literal = ids["first part </s> second part <s><mask> [UNK] </S> <MASK>"]
    assert literal.count(2) == 2 and literal.count(0) == 2 and literal.count(len(v) - 1) == 1 and 4 in literal
    assert ids["<s></s><mask>"] == [0, 0, 2, len(v) - 1, 2]
    assert ids[""] == [0, 2]
    assert not any(M.PAD in t for t in m["tokenizer_cases"])
    assert not any(1 in row for rows in m["tokenizer_ids"].values() for row in rows)
    assert max(len(x) for x in m["tokenizer_ids"][f"lower_max{m['truncate_at']}"]) == m["truncate_at"]


def test_bert_tokenizer_is_unchanged():
    from src.preprocessing.sbert import WordPieceTokenizer
    m = R.meta()
    vocab = (R.GOLDEN / "sbert_vocab.txt").read_text(encoding="utf-8").split("\n")[:-1]
    for key, rows in m["tokenizer_ids"].items():
        tok = WordPieceTokenizer(vocab, do_lower_case=key.startswith("lower"),
                                 max_seq_length=m["truncate_at"] if "max" in key else 512)
        assert [tok.encode(t) for t in m["tokenizer_cases"]] == rows, key
    with pytest.raises(ValueError, match=r"special token <s> is missing"):
        WordPieceTokenizer(vocab, cls_token="<s>")


# --------------------------------------------------------------------------------------------------- loader ----
@pytest.mark.parametrize("fmt,prefix", [("safetensors", ""), ("safetensors", "mpnet."), ("bin", ""), ("bin", "mpnet.")])
def test_model_dir_round_trip(tmp_path, fmt, prefix):
    from src.preprocessing.sbert import load_model_dir
    d = M.write_model_dir(tmp_path / "m", "h128", fmt=fmt, prefix=prefix, max_seq_length=200, do_lower_case=False)
    m = load_model_dir(d)
    w = M.weights("h128")
    assert set(m.tensors) == set(w)  # pooler.* and embeddings.position_ids are ignored
    assert all(m.tensors[k].dtype == np.float32 and np.array_equal(m.tensors[k], w[k]) for k in w)
    assert (m.hidden_size, m.heads, m.layers, m.intermediate_size, m.max_position) == (128, 4, 2, 512, M.MAX_POS)
    assert m.model_type == "mpnet" and m.layer_norm_eps == M.LN_EPS
    assert m.max_seq_length == 200 and m.do_lower_case is False and m.vocab == M.vocab()
    v = M.vocab()
    assert m.tokenizer().encode("Toy <mask>") == [0, v.index("Toy"), v.index(M.MASK), 2]


def test_model_dir_without_the_optional_files_and_the_clamp(tmp_path):
    from src.preprocessing.sbert import load_model_dir
    m = load_model_dir(M.write_model_dir(tmp_path / "m", "h128", extras=False))
    assert m.max_seq_length == M.MAX_POS - 2 and m.do_lower_case is True and m.lower_text is False
    assert m.tokenizer().encode("toy") == [0, M.vocab().index("toy"), 2]
    m = load_model_dir(M.write_model_dir(tmp_path / "big", "h128", max_seq_length=514))
    assert m.max_seq_length == M.MAX_POS - 2
    m = load_model_dir(M.write_model_dir(tmp_path / "none", "h128", max_seq_length=None))
    assert m.max_seq_length == M.MAX_POS - 2
    cfg = M.config_json("h128")
    del cfg["layer_norm_eps"], cfg["relative_attention_num_buckets"], cfg["pad_token_id"]
    m = load_model_dir(M.write_model_dir(tmp_path / "defaults", "h128", config=cfg))
    assert m.layer_norm_eps == 1e-12


def test_special_tokens_come_from_the_tokenizer_files(tmp_path):
    """all-mpnet-base-v2 ships both <unk> and [UNK]; the tokenizer's files say which one is the unknown token.
    tokenizer_config.json wins over special_tokens_map.json."""
    from src.preprocessing.sbert import load_model_dir
    v = M.vocab()
    d = M.write_model_dir(tmp_path / "a", "h128", special_tokens_map={"unk_token": {"content": "<unk>"}})
    assert load_model_dir(d).tokenizer().encode("一") == [0, v.index(M.UNK), 2]
    d = M.write_model_dir(tmp_path / "b", "h128", tokenizer_config={"unk_token": "<unk>"})
    tok = load_model_dir(d).tokenizer()
    assert tok.encode("一") == [0, v.index(M.UNK_ALT), 2] and tok.encode("a <unk> b")[2] == v.index(M.UNK_ALT)
    d = M.write_model_dir(tmp_path / "c", "h128", special_tokens_map={"unk_token": {"content": "<unk>"}})
    (d / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": True}))
    assert load_model_dir(d).tokenizer().encode("一") == [0, v.index(M.UNK_ALT), 2]
    d = M.write_model_dir(tmp_path / "d", "h128", tokenizer_config={"cls_token": "<start>"})
    with pytest.raises(ValueError, match="<start>"):
        load_model_dir(d).tokenizer()


@pytest.mark.parametrize("field,change", [
    ("relative_attention_num_buckets", {"relative_attention_num_buckets": 64}),
    ("hidden_act", {"hidden_act": "relu"}),
    ("pad_token_id", {"pad_token_id": 0}),
    ("num_attention_heads", {"num_attention_heads": 8}),   # head width 16
    ("model_type", {"model_type": "roberta"}),
])
def test_loader_refuses_by_field(tmp_path, field, change):
    from src.preprocessing.sbert import load_model_dir
    cfg = M.config_json("h128")
    cfg.update(change)
    d = M.write_model_dir(tmp_path / "m", "h128", config=cfg)
    with pytest.raises(ValueError, match=field):
        load_model_dir(d)


def test_loader_refuses_tensors_and_pooling(tmp_path):
    from src.preprocessing.sbert import load_model_dir
    name = "encoder.relative_attention_bias.weight"
    w = M.weights("h128")
    del w[name]
    with pytest.raises(ValueError, match=rf"model_type = 'mpnet' expects tensor '{name}', which is missing"):
        load_model_dir(M.write_model_dir(tmp_path / "missing", "h128", weights_=w))
    w = M.weights("h128")
    w[name] = np.ascontiguousarray(w[name].T)
    with pytest.raises(ValueError, match=rf"model_type = 'mpnet' expects tensor '{name}' of shape \(32, 4\)"):
        load_model_dir(M.write_model_dir(tmp_path / "shape", "h128", weights_=w))
    # a BERT checkpoint under an MPNet config: the error names the model type whose state dict was expected
    with pytest.raises(ValueError, match=r"model_type = 'mpnet' expects tensor 'encoder.layer.0.attention.attn.q.weight'"):
        cfg = dict(R.config_json("h128"), model_type="mpnet", pad_token_id=1)
        load_model_dir(R.write_model_dir(tmp_path / "bert", "h128", config=cfg))
    # and an MPNet checkpoint under a BERT config keeps the BERT branch's wording
    with pytest.raises(ValueError, match="token_type_embeddings"):
        cfg = dict(M.config_json("h128"), model_type="bert", max_position_embeddings=M.MAX_POS)
        load_model_dir(M.write_model_dir(tmp_path / "as_bert", "h128", config=cfg))
    d = M.write_model_dir(tmp_path / "cls", "h128")
    (d / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": True,
                                                             "pooling_mode_mean_tokens": False}))
    with pytest.raises(ValueError, match="pooling_mode"):
        load_model_dir(d)


# ------------------------------------------------------------------------------------------------ contract ----
def test_header_bindings_and_abi():
    from hvae import _lib
    header = (ROOT / "include" / "hvae.h").read_text()
    name = "hvae_sbert_attention_relbias"
    assert re.search(r"#define HVAE_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    assert re.search(rf"\bint {name}\(", header)
    restype, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == 12 and len(_lib.SIGNATURES["hvae_sbert_attention"][1]) == 10
    assert hasattr(_lib.lib(), name)
    # host-side argument checks: no launch happens for a table length outside 1 .. 512 or a null table
    assert _lib.lib().hvae_sbert_attention_relbias(None, None, 1, 1, 64, 2, None, 1, None, 513, None, None) != 0
    mk = (PKG / "Makefile").read_text()
    assert "all-mpnet-base-v2" in mk


def test_wrapper_signature():
    import inspect
    from hvae import ops
    params = list(inspect.signature(ops.sbert_attention).parameters)
    assert params == ["qkv", "pack", "heads", "ctx", "rel", "rel_len"]
