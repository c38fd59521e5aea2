"""float64 numpy restatement of the packed MPNet sentence encoder (the relative-position bias of
hvae_sbert_attention_relbias in csrc/hvae_sbert.hip, the MPNet branch of src/preprocessing/sbert.py) and the synthetic
weights, inputs and model directories its tests share. The BERT encoder's helpers come from tests/sbert_ref.py.

Nothing here is committed as numbers: weights and kernel inputs are drawn from np.random.default_rng(seed) and rounded
to float32 once. tests/golden/make_mpnet_fixture.py records what transformers' MPNetModel (float64, eager attention)
and torch's float64 operators give for them; test_mpnet_cpu.py pins this restatement to those records at 1e-12, so a
device test may compare every row against the restatement.
"""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

import sbert_ref as R

GOLDEN = R.GOLDEN
LN_EPS = 1e-5        # all-mpnet-base-v2's; the library's default is 1e-12
LAYERS = 2
MAX_POS = 514        # 512 positions after the offset of 2
POS_OFFSET = 2       # padding_idx + 1
BUCKETS = 32
# name -> (H, heads, seed)
CONFIGS = {"h128": (128, 4, 111), "h384": (384, 12, 112), "h768": (768, 12, 113)}
# the encoder's sequences: each side of the 16-key tile and 64-query chunk edges; from 130 tokens on both saturated
# buckets (15 and 31: |key - query| >= 128) occur
SEQ_LENS = (2, 3, 15, 16, 17, 63, 64, 65, 128, 129, 130, 257, 384)
# attention cases: name -> (H, heads, seed); the sequences are sbert_ref.KERNEL_LENS, the table covers REL_L tokens
ATT_CASES = {"dh32": (64, 2, 211), "dh64": (128, 2, 212)}
REL_L = 512
# MPNetTokenizer's special tokens and where the vocabulary holds them (ids 0 .. 4, <mask> last)
CLS, PAD, SEP, UNK_ALT, UNK, MASK = "<s>", "<pad>", "</s>", "<unk>", "[UNK]", "<mask>"
FIRST_PIECE = 5


def vocab() -> list[str]:
    return (GOLDEN / "mpnet_vocab.txt").read_text(encoding="utf-8").split("\n")[:-1]


def vocab_size() -> int:
    return len(vocab())


# ------------------------------------------------------------------------------------------------ weights ----
def weights(name: str, vocab_n: int | None = None) -> dict[str, np.ndarray]:
    """MPNetModel's state dict (add_pooling_layer=False) for a config, float32. Linear weights are N(0, 1 / fan_in),
    query and key a further 3 x (a layer-0 logit row standard deviation far above 1); the relative-bias weight is
    N(0, 2^2), so that a wrong bucket moves the output."""
    H, heads, seed = CONFIGS[name]
    vocab_n = vocab_size() if vocab_n is None else vocab_n
    g = np.random.default_rng(seed)
    w: dict[str, np.ndarray] = {}

    def lin(prefix, out_f, in_f, scale=1.0):
        w[prefix + ".weight"] = R.f32(g.standard_normal((out_f, in_f)) * (scale / np.sqrt(in_f)))
        w[prefix + ".bias"] = R.f32(g.standard_normal(out_f) * 0.1)

    def ln(prefix):
        w[prefix + ".weight"] = R.f32(1.0 + 0.1 * g.standard_normal(H))
        w[prefix + ".bias"] = R.f32(0.1 * g.standard_normal(H))

    w["embeddings.word_embeddings.weight"] = R.f32(g.standard_normal((vocab_n, H)))
    w["embeddings.position_embeddings.weight"] = R.f32(0.5 * g.standard_normal((MAX_POS, H)))
    ln("embeddings.LayerNorm")
    for i in range(LAYERS):
        p = f"encoder.layer.{i}."
        lin(p + "attention.attn.q", H, H, 3.0)
        lin(p + "attention.attn.k", H, H, 3.0)
        lin(p + "attention.attn.v", H, H)
        lin(p + "attention.attn.o", H, H)
        ln(p + "attention.LayerNorm")
        lin(p + "intermediate.dense", 4 * H, H)
        lin(p + "output.dense", H, 4 * H)
        ln(p + "output.LayerNorm")
    w["encoder.relative_attention_bias.weight"] = R.f32(2.0 * g.standard_normal((BUCKETS, heads)))
    return w


def config_json(name: str, vocab_n: int | None = None) -> dict:
    H, heads, _ = CONFIGS[name]
    return {"model_type": "mpnet", "architectures": ["MPNetModel"], "hidden_size": H, "num_attention_heads": heads,
            "num_hidden_layers": LAYERS, "intermediate_size": 4 * H, "hidden_act": "gelu",
            "max_position_embeddings": MAX_POS, "layer_norm_eps": LN_EPS, "relative_attention_num_buckets": BUCKETS,
            "vocab_size": vocab_size() if vocab_n is None else vocab_n, "hidden_dropout_prob": 0.1,
            "attention_probs_dropout_prob": 0.1, "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2}


def encoder_ids(name: str) -> tuple[np.ndarray, np.ndarray]:
    """The encoder case's packed ids and cu: <s> random pieces </s> per sequence (no special token inside: MPNetModel
    derives its positions from the ids and does not count <pad>)."""
    g = np.random.default_rng(CONFIGS[name][2] + 1000)
    V = vocab_size()
    ids = []
    for n in SEQ_LENS:
        row = g.integers(FIRST_PIECE, V - 1, size=n)
        row[0], row[-1] = 0, 2
        ids.append(row)
    return np.concatenate(ids).astype(np.int32), R.cu_of(SEQ_LENS)


# ------------------------------------------------------------------------------------- float64 restatement ----
def bucket(delta) -> np.ndarray:
    """T5's bucket rule as MPNetModel applies it (32 buckets, max_distance 128) to delta = key - query, restated
    with integer comparisons: bucket 8 + k holds 8 * 16^(k/8) <= |delta| < 8 * 16^((k+1)/8), i.e. |delta|^8 against
    8^8 * 16^k, exactly."""
    out = []
    for d in np.asarray(delta, dtype=np.int64).ravel().tolist():
        n = -d
        a = abs(n)
        if a < 8:
            b = a
        else:
            k = 0
            while k < 7 and a ** 8 >= 8 ** 8 * 16 ** (k + 1):
                k += 1
            b = 8 + k
        out.append(b + (16 if n < 0 else 0))
    return np.asarray(out, dtype=np.int64).reshape(np.shape(delta))


def rel_table(weight: np.ndarray, L: int) -> np.ndarray:
    """[heads, 2 L - 1] float64: entry (h, (j - i) + L - 1) is the bias of key j for query i."""
    return weight.astype(np.float64)[bucket(np.arange(-(L - 1), L))].T.copy()


def attention(qkv: np.ndarray, cu: np.ndarray, heads: int, rel: np.ndarray, L: int) -> np.ndarray:
    """softmax(Q K^T / sqrt(dh) + rel[h][(j - i) + L - 1]) V inside each sequence and head."""
    qkv, rel = qkv.astype(np.float64), rel.astype(np.float64)
    H = qkv.shape[1] // 3
    dh = H // heads
    out = np.empty((qkv.shape[0], H))
    for s in range(len(cu) - 1):
        a, b = int(cu[s]), int(cu[s + 1])
        pos = np.arange(b - a)
        idx = pos[None, :] - pos[:, None] + L - 1
        for h in range(heads):
            q = qkv[a:b, h * dh:(h + 1) * dh]
            k = qkv[a:b, H + h * dh:H + (h + 1) * dh]
            v = qkv[a:b, 2 * H + h * dh:2 * H + (h + 1) * dh]
            sc = q @ k.T / np.sqrt(float(dh)) + rel[h][idx]
            sc -= sc.max(axis=1, keepdims=True)
            p = np.exp(sc)
            out[a:b, h * dh:(h + 1) * dh] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out


def encode(w: dict[str, np.ndarray], heads: int, ids: np.ndarray, cu: np.ndarray, eps: float = LN_EPS,
           want_logits: bool = False):
    """(last hidden state [T, H], embeddings [S, H]) of the packed sequences, float64."""
    W = {k: v.astype(np.float64) for k, v in w.items()}
    H = W["embeddings.LayerNorm.weight"].shape[0]
    x = R.embed_ln(ids, cu, W["embeddings.word_embeddings.weight"],
                   W["embeddings.position_embeddings.weight"][POS_OFFSET:], np.zeros(H),
                   W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    L = int(np.diff(cu).max())
    rel = rel_table(W["encoder.relative_attention_bias.weight"], L)
    n_layers = 1 + max(int(k.split(".")[2]) for k in W if k.startswith("encoder.layer."))
    for i in range(n_layers):
        p = f"encoder.layer.{i}."
        qkv = np.concatenate([x @ W[p + f"attention.attn.{n}.weight"].T + W[p + f"attention.attn.{n}.bias"]
                              for n in "qkv"], axis=1)
        if want_logits and i == 0:
            return qkv
        ctx = attention(qkv, cu, heads, rel, L)
        a = ctx @ W[p + "attention.attn.o.weight"].T + W[p + "attention.attn.o.bias"]
        x = R.layer_norm(a + x, W[p + "attention.LayerNorm.weight"], W[p + "attention.LayerNorm.bias"], eps)
        f = R.gelu(x @ W[p + "intermediate.dense.weight"].T + W[p + "intermediate.dense.bias"])
        o = f @ W[p + "output.dense.weight"].T + W[p + "output.dense.bias"]
        x = R.layer_norm(o + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
    return x, R.pool_norm(x, cu)


# -------------------------------------------------------------------------------------------- kernel inputs ----
def attention_input(case: str) -> tuple[np.ndarray, np.ndarray, int, np.ndarray]:
    """qkv [T, 3 H] (q and k entries N(0, 9)), cu, heads and rel [heads, 2 REL_L - 1], every entry drawn on its own
    from N(0, 2^2): a table built through buckets is constant over ranges of delta and would hide an off-by-one."""
    H, heads, seed = ATT_CASES[case]
    g = np.random.default_rng(seed)
    cu = R.cu_of(R.KERNEL_LENS)
    qkv = g.standard_normal((int(cu[-1]), 3 * H))
    qkv[:, :2 * H] *= 3.0
    rel = 2.0 * g.standard_normal((heads, 2 * REL_L - 1))
    return R.f32(qkv), cu, heads, R.f32(rel)


@functools.lru_cache(maxsize=None)
def attention_truth(case: str) -> np.ndarray:
    qkv, cu, heads, rel = attention_input(case)
    return attention(qkv, cu, heads, rel, REL_L)


@functools.lru_cache(maxsize=None)
def encoder_truth(name: str):
    """(weights, ids, cu, hidden, embeddings): the restatement's float64 result, computed once per session."""
    w = weights(name)
    ids, cu = encoder_ids(name)
    hidden, emb = encode(w, CONFIGS[name][1], ids, cu)
    for a in (ids, cu, hidden, emb):
        a.setflags(write=False)
    return w, ids, cu, hidden, emb


@functools.lru_cache(maxsize=None)
def fixture() -> dict[str, np.ndarray]:
    return dict(np.load(GOLDEN / "mpnet.npz", allow_pickle=False))


@functools.lru_cache(maxsize=None)
def meta() -> dict:
    return json.loads((GOLDEN / "mpnet_meta.json").read_text())


# ------------------------------------------------------------------------------------------ model directories ----
def write_model_dir(path: Path, name: str, fmt: str = "safetensors", prefix: str = "", config: dict | None = None,
                    weights_: dict | None = None, max_seq_length: int | None = 256, do_lower_case: bool = True,
                    extras: bool = True, tokenizer_config: dict | None = None,
                    special_tokens_map: dict | None = None) -> Path:
    """A sentence-transformers style MPNet model directory with this module's synthetic weights and vocabulary."""
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    w = weights(name) if weights_ is None else weights_
    w = {prefix + k: v for k, v in w.items()}
    H = CONFIGS[name][0]
    w[prefix + "pooler.dense.weight"] = np.zeros((2, 2), np.float32)       # ignored by the loader
    w[prefix + "embeddings.position_ids"] = np.arange(MAX_POS, dtype=np.int64)[None]  # ignored; an int64 buffer
    (path / "config.json").write_text(json.dumps(config_json(name) if config is None else config))
    (path / "vocab.txt").write_text((GOLDEN / "mpnet_vocab.txt").read_text(encoding="utf-8"), encoding="utf-8")
    if fmt == "safetensors":
        R.write_safetensors(path / "model.safetensors", w)
    elif fmt == "bin":
        import torch
        torch.save({k: torch.from_numpy(np.array(v)) for k, v in w.items()}, path / "pytorch_model.bin")
    else:
        raise ValueError(fmt)
    if extras:
        (path / "modules.json").write_text(json.dumps([
            {"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
            {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}]))
        (path / "1_Pooling").mkdir(exist_ok=True)
        (path / "1_Pooling" / "config.json").write_text(json.dumps({
            "word_embedding_dimension": H, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
            "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}))
        sb = {"do_lower_case": False}
        if max_seq_length is not None:
            sb["max_seq_length"] = max_seq_length
        (path / "sentence_bert_config.json").write_text(json.dumps(sb))
        (path / "tokenizer_config.json").write_text(json.dumps({
            "do_lower_case": do_lower_case, "tokenizer_class": "MPNetTokenizer", "cls_token": CLS, "sep_token": SEP,
            "pad_token": PAD, "mask_token": MASK, "unk_token": UNK, **(tokenizer_config or {})}))
        if special_tokens_map is not None:
            (path / "special_tokens_map.json").write_text(json.dumps(special_tokens_map))
    return path
