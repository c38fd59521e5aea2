"""float64 numpy restatement of the packed BERT sentence encoder (csrc/hvae_sbert.hip, src/preprocessing/sbert.py) and
the synthetic weights, inputs and model directories its tests share.

Nothing here is committed as numbers: weights and kernel inputs are drawn from np.random.default_rng(seed) and rounded
to float32 once, so the float64 truth and the device see the same values. tests/golden/make_sbert_fixture.py records
what transformers' BertModel (float64, eager attention) and torch's float64 operators give for them; the fixture
holds the encoder's embeddings in full and the larger arrays at sampled rows (sample_rows), and test_sbert_cpu.py
pins this restatement to those records at 1e-12, so a device test may compare every row against the restatement.
"""
from __future__ import annotations

import functools
import json
import struct
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
LN_EPS = 1e-12
LAYERS = 2
MAX_POS = 512
# name -> (H, heads, seed)
CONFIGS = {"h384": (384, 12, 101), "h768": (768, 12, 102), "h128": (128, 4, 103)}
# the encoder's sequences: each side of the 16-key tile and 64-query chunk edges
SEQ_LENS = (2, 3, 15, 16, 17, 63, 64, 65, 128, 129, 256)
# the per-kernel sequences
KERNEL_LENS = (1, 2, 16, 17, 64, 65, 512)
# attention cases: name -> (H, heads, seed): head widths 32 and 64, two heads each (the second head's offset)
ATT_CASES = {"dh32": (64, 2, 201), "dh64": (128, 2, 202)}
# row kernels (embed + LayerNorm, add + LayerNorm, pooling): the narrowest and widest widths, one below a wave's 64
# float4 columns and one that is no multiple of them
LN_WIDTHS = (4, 128, 384, 1024)
LN_ROWS = 9          # no multiple of the four rows of a block
EMB_VOCAB = 50       # the embedding kernel's table
EMB_H = 128
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")


def vocab_size() -> int:
    return len((GOLDEN / "sbert_vocab.txt").read_text(encoding="utf-8").splitlines())


def cu_of(lens) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def sample_rows(cu: np.ndarray) -> np.ndarray:
    """The rows of a packed array that the fixture keeps: per sequence the first and last row and both sides of every
    64-row chunk edge."""
    rows = []
    for s in range(len(cu) - 1):
        b, n = int(cu[s]), int(cu[s + 1] - cu[s])
        pos = {0, n - 1}
        for e in range(64, n, 64):
            pos.update((e - 1, e))
        rows.extend(b + p for p in sorted(pos))
    return np.asarray(rows, dtype=np.int64)


def f32(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ weights ----
def weights(name: str, vocab: int | None = None) -> dict[str, np.ndarray]:
    """BertModel's state dict (add_pooling_layer=False) for a config, float32. Linear weights are N(0, 1 / fan_in);
    query and key weights a further 3 x, so that the layer-0 logits have a row standard deviation near 9 and the
    softmax is far from flat."""
    H, heads, seed = CONFIGS[name]
    vocab = vocab_size() if vocab is None else vocab
    g = np.random.default_rng(seed)
    w: dict[str, np.ndarray] = {}

    def lin(prefix, out_f, in_f, scale=1.0):
        w[prefix + ".weight"] = f32(g.standard_normal((out_f, in_f)) * (scale / np.sqrt(in_f)))
        w[prefix + ".bias"] = f32(g.standard_normal(out_f) * 0.1)

    def ln(prefix):
        w[prefix + ".weight"] = f32(1.0 + 0.1 * g.standard_normal(H))
        w[prefix + ".bias"] = f32(0.1 * g.standard_normal(H))

    w["embeddings.word_embeddings.weight"] = f32(g.standard_normal((vocab, H)))
    w["embeddings.position_embeddings.weight"] = f32(0.5 * g.standard_normal((MAX_POS, H)))
    w["embeddings.token_type_embeddings.weight"] = f32(0.5 * g.standard_normal((2, H)))
    ln("embeddings.LayerNorm")
    for i in range(LAYERS):
        p = f"encoder.layer.{i}."
        lin(p + "attention.self.query", H, H, 3.0)
        lin(p + "attention.self.key", H, H, 3.0)
        lin(p + "attention.self.value", H, H)
        lin(p + "attention.output.dense", H, H)
        ln(p + "attention.output.LayerNorm")
        lin(p + "intermediate.dense", 4 * H, H)
        lin(p + "output.dense", H, 4 * H)
        ln(p + "output.LayerNorm")
    return w


def config_json(name: str, vocab: int | None = None) -> dict:
    H, heads, _ = CONFIGS[name]
    return {"model_type": "bert", "architectures": ["BertModel"], "hidden_size": H, "num_attention_heads": heads,
            "num_hidden_layers": LAYERS, "intermediate_size": 4 * H, "hidden_act": "gelu",
            "max_position_embeddings": MAX_POS, "type_vocab_size": 2, "layer_norm_eps": LN_EPS,
            "position_embedding_type": "absolute", "vocab_size": vocab_size() if vocab is None else vocab,
            "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1, "pad_token_id": 0}


def encoder_ids(name: str) -> tuple[np.ndarray, np.ndarray]:
    """The encoder case's packed ids and cu: [CLS] random pieces [SEP] per sequence."""
    g = np.random.default_rng(CONFIGS[name][2] + 1000)
    V = vocab_size()
    ids = []
    for n in SEQ_LENS:
        row = g.integers(len(SPECIALS), V, size=n)
        row[0], row[-1] = 2, 3
        ids.append(row)
    return np.concatenate(ids).astype(np.int32), cu_of(SEQ_LENS)


# ------------------------------------------------------------------------------------- float64 restatement ----
def layer_norm(x: np.ndarray, w: np.ndarray, b: np.ndarray, eps: float = LN_EPS) -> np.ndarray:
    x = x.astype(np.float64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w.astype(np.float64) + b.astype(np.float64)


def gelu(x: np.ndarray) -> np.ndarray:
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def embed_ln(ids, cu, word, pos, type0, ln_w, ln_b, eps: float = LN_EPS) -> np.ndarray:
    p = np.concatenate([np.arange(cu[s + 1] - cu[s]) for s in range(len(cu) - 1)])
    x = word.astype(np.float64)[ids] + pos.astype(np.float64)[p] + type0.astype(np.float64)
    return layer_norm(x, ln_w, ln_b, eps)


def attention(qkv: np.ndarray, cu: np.ndarray, heads: int) -> np.ndarray:
    qkv = qkv.astype(np.float64)
    H = qkv.shape[1] // 3
    dh = H // heads
    out = np.empty((qkv.shape[0], H))
    for s in range(len(cu) - 1):
        a, b = int(cu[s]), int(cu[s + 1])
        for h in range(heads):
            q = qkv[a:b, h * dh:(h + 1) * dh]
            k = qkv[a:b, H + h * dh:H + (h + 1) * dh]
            v = qkv[a:b, 2 * H + h * dh:2 * H + (h + 1) * dh]
            sc = q @ k.T / np.sqrt(float(dh))
            sc -= sc.max(axis=1, keepdims=True)
            p = np.exp(sc)
            out[a:b, h * dh:(h + 1) * dh] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out


def pool_norm(x: np.ndarray, cu: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    m = np.stack([x[cu[s]:cu[s + 1]].mean(axis=0) for s in range(len(cu) - 1)])
    return m / np.maximum(np.sqrt((m * m).sum(axis=1, keepdims=True)), 1e-12)


def encode(w: dict[str, np.ndarray], heads: int, ids: np.ndarray, cu: np.ndarray, eps: float = LN_EPS,
           want_logits: bool = False):
    """(last hidden state [T, H], embeddings [S, H]) of the packed sequences, float64."""
    W = {k: v.astype(np.float64) for k, v in w.items()}
    x = embed_ln(ids, cu, W["embeddings.word_embeddings.weight"], W["embeddings.position_embeddings.weight"],
                 W["embeddings.token_type_embeddings.weight"][0], W["embeddings.LayerNorm.weight"],
                 W["embeddings.LayerNorm.bias"], eps)
    n_layers = 1 + max(int(k.split(".")[2]) for k in W if k.startswith("encoder.layer."))
    for i in range(n_layers):
        p = f"encoder.layer.{i}."
        qkv = np.concatenate([x @ W[p + f"attention.self.{n}.weight"].T + W[p + f"attention.self.{n}.bias"]
                              for n in ("query", "key", "value")], axis=1)
        if want_logits and i == 0:
            return qkv
        ctx = attention(qkv, cu, heads)
        a = ctx @ W[p + "attention.output.dense.weight"].T + W[p + "attention.output.dense.bias"]
        x = layer_norm(a + x, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        f = gelu(x @ W[p + "intermediate.dense.weight"].T + W[p + "intermediate.dense.bias"])
        o = f @ W[p + "output.dense.weight"].T + W[p + "output.dense.bias"]
        x = layer_norm(o + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
    return x, pool_norm(x, cu)


# -------------------------------------------------------------------------------------------- kernel inputs ----
def attention_input(case: str) -> tuple[np.ndarray, np.ndarray, int]:
    """qkv [T, 3 H] with logits of row standard deviation near 9 (q and k entries N(0, 9)), cu, heads."""
    H, heads, seed = ATT_CASES[case]
    g = np.random.default_rng(seed)
    cu = cu_of(KERNEL_LENS)
    qkv = g.standard_normal((int(cu[-1]), 3 * H))
    qkv[:, :2 * H] *= 3.0
    return f32(qkv), cu, heads


def ln_input(H: int) -> dict[str, np.ndarray]:
    g = np.random.default_rng(300 + H)
    return {"x": f32(g.standard_normal((LN_ROWS, H)) * 2.0 + 0.5), "res": f32(g.standard_normal((LN_ROWS, H))),
            "w": f32(1.0 + 0.1 * g.standard_normal(H)), "b": f32(0.1 * g.standard_normal(H))}


def embed_input() -> dict[str, np.ndarray]:
    g = np.random.default_rng(400)
    cu = cu_of(KERNEL_LENS)
    return {"ids": g.integers(0, EMB_VOCAB, size=int(cu[-1])).astype(np.int32), "cu": cu,
            "word": f32(g.standard_normal((EMB_VOCAB, EMB_H))), "pos": f32(0.5 * g.standard_normal((MAX_POS, EMB_H))),
            "type0": f32(0.5 * g.standard_normal(EMB_H)), "w": f32(1.0 + 0.1 * g.standard_normal(EMB_H)),
            "b": f32(0.1 * g.standard_normal(EMB_H))}


def pool_input(H: int) -> tuple[np.ndarray, np.ndarray]:
    g = np.random.default_rng(500 + H)
    cu = cu_of(KERNEL_LENS)
    return f32(g.standard_normal((int(cu[-1]), H)) + 0.25), cu


@functools.lru_cache(maxsize=None)
def fixture() -> dict[str, np.ndarray]:
    return dict(np.load(GOLDEN / "sbert.npz", allow_pickle=False))


@functools.lru_cache(maxsize=None)
def meta() -> dict:
    return json.loads((GOLDEN / "sbert_meta.json").read_text())


# ------------------------------------------------------------------------------------------ model directories ----
def write_safetensors(path: Path, tensors: dict[str, np.ndarray]) -> None:
    """The safetensors container: 8-byte little-endian header length, a JSON header, the raw data."""
    codes = {np.dtype(np.float32): "F32", np.dtype(np.float16): "F16", np.dtype(np.uint16): "BF16",
             np.dtype(np.int64): "I64"}
    header, blobs, off = {}, [], 0
    for k, v in tensors.items():
        raw = np.ascontiguousarray(v).tobytes()
        header[k] = {"dtype": codes[v.dtype], "shape": list(v.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    header["__metadata__"] = {"format": "pt"}
    hj = json.dumps(header).encode()
    hj += b" " * (-len(hj) % 8)
    path.write_bytes(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))


def write_model_dir(path: Path, name: str, fmt: str = "safetensors", prefix: str = "", config: dict | None = None,
                    weights_: dict | None = None, max_seq_length: int | None = 256, do_lower_case: bool = True,
                    extras: bool = True, tokenizer_config: dict | None = None) -> Path:
    """A sentence-transformers style model directory with this module's synthetic weights and vocabulary."""
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    w = weights(name) if weights_ is None else weights_
    w = {prefix + k: v for k, v in w.items()}
    H = CONFIGS[name][0]
    w[prefix + "pooler.dense.weight"] = np.zeros((2, 2), np.float32)       # ignored by the loader
    # ignored by the loader; an int64 buffer, as BertModel's checkpoints carry it
    w[prefix + "embeddings.position_ids"] = np.arange(MAX_POS, dtype=np.int64)[None]
    (path / "config.json").write_text(json.dumps(config_json(name) if config is None else config))
    (path / "vocab.txt").write_text((GOLDEN / "sbert_vocab.txt").read_text(encoding="utf-8"), encoding="utf-8")
    if fmt == "safetensors":
        write_safetensors(path / "model.safetensors", w)
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
        (path / "tokenizer_config.json").write_text(json.dumps({"do_lower_case": do_lower_case,
                                                                 "tokenizer_class": "BertTokenizer",
                                                                 **(tokenizer_config or {})}))
    return path
