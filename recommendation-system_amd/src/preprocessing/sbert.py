"""A BERT-family sentence encoder on the device: what SentenceTransformer(model_dir).encode(texts,
normalize_embeddings=True) computes for a model such as all-MiniLM-L6-v2 (src/preprocessing/embeddings.py:35-63 of the
reference), from a local model directory and without transformers, tokenizers, sentence_transformers,
huggingface_hub or safetensors. Two bodies are served: BertModel (model_type "bert") and MPNetModel ("mpnet", as in
all-mpnet-base-v2): the same post-LayerNorm layers with a learned relative-position bias on every attention score,
positions that start at 2, no token types, and <s> ... </s> around the pieces.

  load_model_dir(path)   config.json, model.safetensors | pytorch_model.bin, vocab.txt and the optional
                         sentence-transformers files -> SbertModel (fp32 numpy weights, the vocabulary, the limits)
  WordPieceTokenizer     BertTokenizer restated: cleaning, CJK spacing, lower-casing with accent stripping,
                         punctuation split, greedy longest match, literal special tokens, truncation
  SbertEncoder.encode    tokenise, pack up to batch_size texts per pass without padding, run the K22 kernels and
                         hvae_gemm_f32 (hvae/ops.py), return the rows in input order

Nothing is fetched, here or anywhere below: a model is a directory on the local disk.
"""
from __future__ import annotations

import json
import re
import struct
import unicodedata
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

MAX_WORD_CHARS = 100  # WordPiece's max_input_chars_per_word
IGNORED_TENSORS = ("pooler.", "embeddings.position_ids")
SERVED_MODEL_TYPES = ("bert", "mpnet")
# the special tokens by model type: BertTokenizer's and MPNetTokenizer's defaults
SPECIALS = {"bert": {"cls_token": "[CLS]", "sep_token": "[SEP]", "pad_token": "[PAD]", "mask_token": "[MASK]",
                     "unk_token": "[UNK]"},
            "mpnet": {"cls_token": "<s>", "sep_token": "</s>", "pad_token": "<pad>", "mask_token": "<mask>",
                      "unk_token": "[UNK]"}}
# the layer tensors by model type: query, key, value, attention output, the LayerNorm after it
LAYER_NAMES = {"bert": ("attention.self.query", "attention.self.key", "attention.self.value",
                        "attention.output.dense", "attention.output.LayerNorm"),
               "mpnet": ("attention.attn.q", "attention.attn.k", "attention.attn.v", "attention.attn.o",
                         "attention.LayerNorm")}
REL_BIAS = "encoder.relative_attention_bias.weight"  # MPNet's [32, heads] table, shared by all layers
REL_BUCKETS, REL_MAX_DISTANCE = 32, 128  # MPNetEncoder.compute_position_bias's arguments; not read from the config
MPNET_POS_OFFSET = 2  # MPNet's positions start at padding_idx + 1


# ------------------------------------------------------------------------------------------------ weights ----
def _tensor_name(name: str, model_type: str = "bert") -> str | None:
    """The model's own name of a checkpoint tensor (an optional "bert." / "mpnet." prefix dropped), or None for one
    the encoder does not read: pooler.* and embeddings.position_ids (an int64 buffer in real checkpoints)."""
    prefix = model_type + "."
    name = name[len(prefix):] if name.startswith(prefix) else name
    return None if name.startswith(IGNORED_TENSORS) else name


def relative_position_bucket(delta) -> np.ndarray:
    """MPNetEncoder.relative_position_bucket (T5's rule, 32 buckets, max_distance 128) of delta = key - query: with
    n = -delta, 16 [n < 0] + (|n| if |n| < 8 else min(15, 8 + floor(log(|n| / 8) / log(16) * 8)))."""
    n = -np.asarray(delta, dtype=np.int64)
    half, exact = REL_BUCKETS // 2, REL_BUCKETS // 4
    a = np.abs(n)
    large = exact + (np.log(np.maximum(a, 1) / exact) / np.log(REL_MAX_DISTANCE / exact) * (half - exact)).astype(
        np.int64)
    return (n < 0) * half + np.where(a < exact, a, np.minimum(large, half - 1))


def relative_bias_table(weight: np.ndarray, L: int) -> np.ndarray:
    """rel [heads, 2 L - 1] float32 from MPNet's [32, heads] weight: rel[h][(j - i) + L - 1] is the bias of key j for
    query i, for sequences of up to L tokens (hvae_sbert_attention_relbias's table)."""
    weight = np.asarray(weight)
    if weight.ndim != 2 or weight.shape[0] != REL_BUCKETS or L < 1:
        raise ValueError(f"relative_bias_table: weight {weight.shape} must be [{REL_BUCKETS}, heads] and L = {L} >= 1")
    bucket = relative_position_bucket(np.arange(-(L - 1), L))
    return np.ascontiguousarray(weight[bucket].T, dtype=np.float32)


def read_safetensors(path, rename=lambda name: name) -> dict[str, np.ndarray]:
    """The safetensors container read natively: an 8-byte little-endian header length, a JSON header of
    {name: {dtype, shape, data_offsets}}, then the raw little-endian data. rename maps a stored name to the key it is
    returned under, or to None to skip the tensor whatever its dtype. F32, F16 and BF16 are served and returned as
    float32."""
    raw = Path(path).read_bytes()
    if len(raw) < 8:
        raise ValueError(f"{path}: not a safetensors file (shorter than its 8-byte header length)")
    (n,) = struct.unpack("<Q", raw[:8])
    if n > len(raw) - 8:
        raise ValueError(f"{path}: the header length {n} exceeds the file")
    header = json.loads(raw[8:8 + n].decode("utf-8"))
    data = memoryview(raw)[8 + n:]
    out = {}
    for name, info in header.items():
        key = None if name == "__metadata__" else rename(name)
        if key is None:
            continue
        dtype, shape, (a, b) = info["dtype"], tuple(info["shape"]), info["data_offsets"]
        count = int(np.prod(shape, dtype=np.int64))
        width = {"F32": 4, "F16": 2, "BF16": 2}.get(dtype)
        if width is None:
            raise ValueError(f"{path}: tensor {name!r} has dtype {dtype}; F32, F16 and BF16 are served")
        if b - a != count * width or b > len(data):
            raise ValueError(f"{path}: tensor {name!r} spans bytes {a}..{b}, its shape {shape} needs {count * width}")
        if dtype == "F32":
            arr = np.frombuffer(data[a:b], dtype="<f4").astype(np.float32)
        elif dtype == "F16":
            arr = np.frombuffer(data[a:b], dtype="<f2").astype(np.float32)
        else:  # bfloat16 is float32's upper half
            arr = (np.frombuffer(data[a:b], dtype="<u2").astype(np.uint32) << 16).view(np.float32)
        out[key] = arr.reshape(shape)
    return out


def read_torch_bin(path, rename=lambda name: name) -> dict[str, np.ndarray]:
    """A torch state dict (weights_only) under the same renaming; a wanted tensor that is not floating point is
    refused by name, as in read_safetensors."""
    import torch
    out = {}
    for name, v in torch.load(path, map_location="cpu", weights_only=True).items():
        key = rename(name)
        if key is None:
            continue
        if not isinstance(v, torch.Tensor) or not v.is_floating_point():
            kind = v.dtype if isinstance(v, torch.Tensor) else type(v).__name__
            raise ValueError(f"{path}: tensor {name!r} has dtype {kind}; floating-point tensors are served")
        out[key] = v.detach().to(torch.float32).numpy()
    return out


@dataclass
class SbertModel:
    path: Path
    hidden_size: int
    heads: int
    layers: int
    intermediate_size: int
    max_position: int
    layer_norm_eps: float
    max_seq_length: int
    do_lower_case: bool          # the tokenizer's
    lower_text: bool             # sentence_bert_config.json's: lower-case the text before tokenising
    vocab: list[str] = field(repr=False)
    tensors: dict[str, np.ndarray] = field(repr=False)
    model_type: str = "bert"
    special_tokens: dict[str, str] | None = None  # cls_token, sep_token, ...; None: the model type's defaults

    def tokenizer(self) -> "WordPieceTokenizer":
        return WordPieceTokenizer(self.vocab, self.do_lower_case, self.max_seq_length, self.lower_text,
                                  **{**SPECIALS[self.model_type], **(self.special_tokens or {})})


def _read_json(p: Path) -> dict | list | None:
    return json.loads(p.read_text(encoding="utf-8")) if p.exists() else None


def load_model_dir(path) -> SbertModel:
    """Read a sentence-transformers / BertModel or MPNetModel directory. Anything this encoder does not compute is
    refused with an error that names the field."""
    path = Path(path)
    cfg = _read_json(path / "config.json")
    if cfg is None:
        raise FileNotFoundError(f"{path}: config.json not found")
    mtype = cfg.get("model_type")
    if mtype not in SERVED_MODEL_TYPES:
        raise ValueError(f"{path}/config.json: model_type = {mtype!r}; only "
                         f"{' and '.join(repr(t) for t in SERVED_MODEL_TYPES)} are served")
    mpnet = mtype == "mpnet"
    if mpnet and cfg.get("relative_attention_num_buckets", REL_BUCKETS) != REL_BUCKETS:
        raise ValueError(f"{path}/config.json: relative_attention_num_buckets = "
                         f"{cfg['relative_attention_num_buckets']!r}; only {REL_BUCKETS} is served (MPNetModel itself "
                         "computes its buckets with 32 whatever the config says)")
    if mpnet and cfg.get("pad_token_id", 1) != 1:
        raise ValueError(f"{path}/config.json: pad_token_id = {cfg['pad_token_id']!r} with model_type = {mtype!r}; "
                         f"only 1 is served (MPNet's positions start at pad_token_id + 1 = {MPNET_POS_OFFSET})")
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"{path}/config.json: position_embedding_type = {cfg['position_embedding_type']!r}; only "
                         "'absolute' is served")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"{path}/config.json: hidden_act = {cfg['hidden_act']!r}; only 'gelu' (erf) is served")
    for key in ("hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size",
                "max_position_embeddings"):
        if not isinstance(cfg.get(key), int) or cfg[key] < 1:
            raise ValueError(f"{path}/config.json: {key} = {cfg.get(key)!r} must be a positive integer")
    H, heads, layers = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"]
    inter, max_pos = cfg["intermediate_size"], cfg["max_position_embeddings"]

    modules = _read_json(path / "modules.json")
    pool_dir = "1_Pooling"
    if modules is not None:
        for m in modules:
            kind = str(m.get("type", "")).rsplit(".", 1)[-1]
            if kind == "Pooling":
                pool_dir = m.get("path", pool_dir)
            elif kind not in ("Transformer", "Normalize"):
                raise ValueError(f"{path}/modules.json: module type {m.get('type')!r} is not served (Transformer, "
                                 "Pooling and Normalize are)")
    pooling = _read_json(path / pool_dir / "config.json")
    if pooling is not None:
        modes = {k: v for k, v in pooling.items() if k.startswith("pooling_mode_") and v}
        if set(modes) != {"pooling_mode_mean_tokens"}:
            raise ValueError(f"{path}/{pool_dir}/config.json: pooling_mode = {sorted(modes)}; only "
                             "pooling_mode_mean_tokens is served")
    sb = _read_json(path / "sentence_bert_config.json") or {}
    tk = _read_json(path / "tokenizer_config.json") or {}
    lower = bool(tk.get("do_lower_case", True))
    if tk.get("strip_accents") is not None and bool(tk["strip_accents"]) != lower:
        raise ValueError(f"{path}/tokenizer_config.json: strip_accents = {tk['strip_accents']!r} with do_lower_case = "
                         f"{lower}; accents are stripped exactly when lower-casing (strip_accents null or equal to it)")
    if not tk.get("tokenize_chinese_chars", True):
        raise ValueError(f"{path}/tokenizer_config.json: tokenize_chinese_chars = false is not served")
    max_seq = sb.get("max_seq_length") or tk.get("model_max_length") or max_pos
    max_seq = int(min(max_seq, max_pos - MPNET_POS_OFFSET if mpnet else max_pos))
    if max_seq < 3:
        raise ValueError(f"{path}: max_seq_length = {max_seq} leaves no room for a token between [CLS] and [SEP]")
    specials = None
    if mpnet:  # tokenizer_config.json wins over special_tokens_map.json, as in transformers
        specials = dict(SPECIALS[mtype])
        for source in (_read_json(path / "special_tokens_map.json") or {}, tk):
            for key in specials:
                v = source.get(key)
                v = v.get("content") if isinstance(v, dict) else v
                if isinstance(v, str):
                    specials[key] = v

    from hvae import _lib
    if not _lib.lib().hvae_sbert_supported(H, heads, max_seq):
        raise ValueError(f"{path}/config.json: hidden_size = {H} with num_attention_heads = {heads} and "
                         f"max_seq_length = {max_seq} is not served (head width 32 or 64, hidden_size a multiple of "
                         "4 up to 1024, at most 512 tokens)")
    if inter % 4:
        raise ValueError(f"{path}/config.json: intermediate_size = {inter} must be a multiple of 4")

    rename = lambda name: _tensor_name(name, mtype)  # noqa: E731
    if (path / "model.safetensors").exists():
        raw = read_safetensors(path / "model.safetensors", rename)
    elif (path / "pytorch_model.bin").exists():
        raw = read_torch_bin(path / "pytorch_model.bin", rename)
    else:
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin found")
    tensors = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in raw.items()}
    want = {"embeddings.word_embeddings.weight": None, "embeddings.position_embeddings.weight": (max_pos, H),
            "embeddings.token_type_embeddings.weight": None, "embeddings.LayerNorm.weight": (H,),
            "embeddings.LayerNorm.bias": (H,)}
    if mpnet:
        del want["embeddings.token_type_embeddings.weight"]
    nq, nk, nv, no, nln = LAYER_NAMES[mtype]
    linear = {nq: (H, H), nk: (H, H), nv: (H, H), no: (H, H), "intermediate.dense": (inter, H),
              "output.dense": (H, inter)}
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for n, (out_f, in_f) in linear.items():
            want[p + n + ".weight"], want[p + n + ".bias"] = (out_f, in_f), (out_f,)
        for n in (nln, "output.LayerNorm"):
            want[p + n + ".weight"], want[p + n + ".bias"] = (H,), (H,)
    if mpnet:
        want[REL_BIAS] = (REL_BUCKETS, heads)
    for n, shape in want.items():
        if mpnet:  # the state dict follows the config's model_type: name it, a BERT checkpoint has other names
            if n not in tensors:
                raise ValueError(f"{path}: model_type = {mtype!r} expects tensor {n!r}, which is missing from the "
                                 "weights")
            if shape is not None and tuple(tensors[n].shape) != shape:
                raise ValueError(f"{path}: model_type = {mtype!r} expects tensor {n!r} of shape {shape}, it has "
                                 f"{tuple(tensors[n].shape)}")
            continue
        if n not in tensors:
            raise ValueError(f"{path}: tensor {n!r} is missing from the weights")
        if shape is not None and tuple(tensors[n].shape) != shape:
            raise ValueError(f"{path}: tensor {n!r} has shape {tuple(tensors[n].shape)}, config.json implies {shape}")

    vocab_path = path / "vocab.txt"
    if not vocab_path.exists():
        raise FileNotFoundError(f"{path}: vocab.txt not found (a WordPiece vocabulary, one piece per line)")
    vocab = vocab_path.read_text(encoding="utf-8").split("\n")
    while vocab and vocab[-1] == "":
        vocab.pop()
    vocab = [v.rstrip("\r") for v in vocab]
    word = tensors["embeddings.word_embeddings.weight"]
    if word.ndim != 2 or word.shape[1] != H or word.shape[0] < len(vocab):
        raise ValueError(f"{path}: tensor 'embeddings.word_embeddings.weight' has shape {tuple(word.shape)}; vocab.txt "
                         f"holds {len(vocab)} pieces of width {H}")
    if not mpnet:
        tt = tensors["embeddings.token_type_embeddings.weight"]
        if tt.ndim != 2 or tt.shape[1] != H or tt.shape[0] < 1:
            raise ValueError(f"{path}: tensor 'embeddings.token_type_embeddings.weight' has shape {tuple(tt.shape)}")
    return SbertModel(path=path, hidden_size=H, heads=heads, layers=layers, intermediate_size=inter,
                      max_position=max_pos, layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-12)),
                      max_seq_length=max_seq, do_lower_case=lower,
                      lower_text=bool(sb.get("do_lower_case", False)), vocab=vocab, tensors=tensors,
                      model_type=mtype, special_tokens=specials)


# ---------------------------------------------------------------------------------------------- tokenizer ----
def _is_whitespace(c: str) -> bool:
    return c in " \t\n\r" or unicodedata.category(c) in ("Zs", "Zl", "Zp")


def _is_control(c: str) -> bool:
    return c not in "\t\n\r" and unicodedata.category(c).startswith("C")  # Cc, Cf, Cn, Co and lone surrogates (Cs)


def _is_punctuation(c: str) -> bool:
    cp = ord(c)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(c).startswith("P")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF
            or 0x2F800 <= cp <= 0x2FA1F)


class WordPieceTokenizer:
    """BertTokenizer restated. encode(text) -> [CLS] pieces [SEP] as vocabulary ids, at most max_seq_length. The
    special tokens default to BertTokenizer's; MPNetTokenizer is the same WordPiece with SPECIALS["mpnet"]."""

    def __init__(self, vocab: list[str], do_lower_case: bool = True, max_seq_length: int = 512,
                 lower_text: bool = False, cls_token: str = "[CLS]", sep_token: str = "[SEP]",
                 pad_token: str = "[PAD]", mask_token: str = "[MASK]", unk_token: str = "[UNK]"):
        self.ids = {}
        for i, piece in enumerate(vocab):
            self.ids.setdefault(piece, i)
        for t in (unk_token, cls_token, sep_token):
            if t not in self.ids:
                raise ValueError(f"vocab.txt: the special token {t} is missing")
        self.unk, self.cls, self.sep = self.ids[unk_token], self.ids[cls_token], self.ids[sep_token]
        self.do_lower_case, self.max_seq_length, self.lower_text = do_lower_case, int(max_seq_length), lower_text
        specials = [t for t in dict.fromkeys((unk_token, sep_token, pad_token, cls_token, mask_token))
                    if t in self.ids]
        self._special = re.compile("(" + "|".join(re.escape(t) for t in sorted(specials, key=len, reverse=True)) + ")")
        self._cache: dict[str, list[int]] = {}

    def _normalize(self, text: str) -> str:
        out = []
        for c in text:  # clean: drop NUL, U+FFFD and control characters; every whitespace becomes a space
            cp = ord(c)
            if cp == 0 or cp == 0xFFFD or _is_control(c):
                continue
            if _is_whitespace(c):
                out.append(" ")
            elif _is_cjk(cp):
                out.append(" " + c + " ")
            else:
                out.append(c)
        text = "".join(out)
        if self.do_lower_case:  # accents are stripped exactly when lower-casing (strip_accents = None)
            text = "".join(c for c in unicodedata.normalize("NFD", text) if unicodedata.category(c) != "Mn").lower()
        return text

    def _word(self, word: str) -> list[int]:
        got = self._cache.get(word)
        if got is not None:
            return got
        if len(word) > MAX_WORD_CHARS:
            return [self.unk]
        pieces, start = [], 0
        while start < len(word):
            end, cur = len(word), None
            while start < end:
                cur = self.ids.get(("##" if start else "") + word[start:end])
                if cur is not None:
                    break
                end -= 1
            if cur is None:
                pieces = [self.unk]
                break
            pieces.append(cur)
            start = end
        if len(self._cache) < 1 << 20:
            self._cache[word] = pieces
        return pieces

    def pieces(self, text: str) -> list[int]:
        """The ids of the text's pieces, without [CLS] / [SEP] and without truncation."""
        if self.lower_text:
            text = text.lower()
        out: list[int] = []
        for i, part in enumerate(self._special.split(text)):
            if i % 2:  # a special token that occurs literally in the text
                out.append(self.ids[part])
                continue
            for word in self._normalize(part).split():
                start = 0
                for j, c in enumerate(word):
                    if _is_punctuation(c):
                        if j > start:
                            out += self._word(word[start:j])
                        out += self._word(c)
                        start = j + 1
                if start < len(word):
                    out += self._word(word[start:])
        return out

    def encode(self, text: str) -> list[int]:
        return [self.cls] + self.pieces(text)[:self.max_seq_length - 2] + [self.sep]


# ------------------------------------------------------------------------------------------------ encoder ----
class SbertEncoder:
    """The model on one HIP device. encode(texts) -> float32 [len(texts), H], rows L2-normalised, in input order."""

    STAGES = ("embed", "qkv", "attention", "output", "ffn", "pool")

    def __init__(self, model: SbertModel, device=None):
        import torch
        from hvae import _lib
        self.model = model
        self.device = torch.device("cuda", 0) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SbertEncoder: device {self.device} is not served; the encoder's kernels are HIP "
                               "kernels for the MI355X and there is no CPU fallback")
        _lib.lib()
        t = model.tensors
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=self.device)  # noqa: E731
        self.word = up(t["embeddings.word_embeddings.weight"])
        if model.model_type == "mpnet":
            # position t of a sequence reads the table's row t + 2; no token types: an exact zero changes no sum's bits
            self.pos = up(t["embeddings.position_embeddings.weight"][MPNET_POS_OFFSET:])
            self.type0 = torch.zeros(model.hidden_size, device=self.device)
            self.rel_len = model.max_seq_length
            self.rel = up(relative_bias_table(t[REL_BIAS], self.rel_len))
        else:
            self.pos = up(t["embeddings.position_embeddings.weight"])
            self.type0 = up(t["embeddings.token_type_embeddings.weight"][0])
            self.rel, self.rel_len = None, None
        self.emb_ln = (up(t["embeddings.LayerNorm.weight"]), up(t["embeddings.LayerNorm.bias"]))
        nq, nk, nv, no, nln = LAYER_NAMES[model.model_type]
        self.layers = []
        for i in range(model.layers):
            p = f"encoder.layer.{i}."
            self.layers.append({
                "wqkv": up(np.concatenate([t[p + n + ".weight"] for n in (nq, nk, nv)], axis=0)),
                "bqkv": up(np.concatenate([t[p + n + ".bias"] for n in (nq, nk, nv)], axis=0)),
                "wo": up(t[p + no + ".weight"]), "bo": up(t[p + no + ".bias"]),
                "ln1": (up(t[p + nln + ".weight"]), up(t[p + nln + ".bias"])),
                "wi": up(t[p + "intermediate.dense.weight"]), "bi": up(t[p + "intermediate.dense.bias"]),
                "wd": up(t[p + "output.dense.weight"]), "bd": up(t[p + "output.dense.bias"]),
                "ln2": (up(t[p + "output.LayerNorm.weight"]), up(t[p + "output.LayerNorm.bias"])),
            })
        self._tok = model.tokenizer()
        self.stage_events = None  # scripts/bench_sbert.py: a list that receives (stage, start event, end event)

    def tokenize(self, texts) -> list[list[int]]:
        return [self._tok.encode(str(t)) for t in texts]

    def _stage(self, name, fn):
        if self.stage_events is None:
            return fn()
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.stage_events.append((name, a, b))
        return out

    def forward_packed(self, ids, cu):
        """(last hidden state [T, H], embeddings [S, H]) as device tensors, for packed ids [T] and offsets cu [S + 1]
        (host integer arrays)."""
        import torch
        from hvae import _lib, ops
        m, eps = self.model, self.model.layer_norm_eps
        pack = ops.SbertPack(ids, cu, self.device)
        T, H, heads = pack.T, m.hidden_size, m.heads
        bias = lambda b: ops.epilogue(_lib.EPI_BIAS, bias=b)  # noqa: E731
        x = self._stage("embed", lambda: ops.sbert_embed_ln(pack, self.word, self.pos, self.type0, *self.emb_ln, eps))
        qkv = torch.empty(T, 3 * H, device=self.device)
        ctx = torch.empty(T, H, device=self.device)
        a = torch.empty(T, H, device=self.device)
        f = torch.empty(T, m.intermediate_size, device=self.device)
        pre = torch.empty(T, m.intermediate_size, device=self.device)
        for L in self.layers:
            self._stage("qkv", lambda: ops.gemm(x, L["wqkv"].t(), out=qkv, epi=bias(L["bqkv"])))
            if self.rel is None:
                self._stage("attention", lambda: ops.sbert_attention(qkv, pack, heads, ctx))
            else:
                self._stage("attention", lambda: ops.sbert_attention(qkv, pack, heads, ctx, self.rel, self.rel_len))

            def output():
                ops.gemm(ctx, L["wo"].t(), out=a, epi=bias(L["bo"]))
                return ops.sbert_add_ln(a, x, *L["ln1"], eps)
            x1 = self._stage("output", output)

            def ffn():
                # the FFN's GELU is the GEMM's BIAS_GELU_DROP epilogue with train = 0; pre is its scratch pre_out
                ops.gemm(x1, L["wi"].t(), out=f,
                         epi=ops.epilogue(_lib.EPI_BIAS_GELU_DROP, bias=L["bi"], pre_out=pre, train=False))
                ops.gemm(f, L["wd"].t(), out=a, epi=bias(L["bd"]))
                return ops.sbert_add_ln(a, x1, *L["ln2"], eps)
            x = self._stage("ffn", ffn)
        emb = self._stage("pool", lambda: ops.sbert_pool_norm(x, pack))
        return x, emb

    def encode_ids(self, seqs, batch_size: int = 32) -> np.ndarray:
        """Embeddings of already tokenised sequences (lists of ids), batch_size sequences per pass, in input order."""
        import torch
        if batch_size < 1:
            raise ValueError(f"encode: batch_size = {batch_size} must be at least 1")
        out = torch.empty(len(seqs), self.model.hidden_size, device=self.device)
        for i in range(0, len(seqs), batch_size):
            part = seqs[i:i + batch_size]
            cu = np.concatenate([[0], np.cumsum([len(s) for s in part])])
            ids = np.concatenate([np.asarray(s, dtype=np.int64) for s in part])
            out[i:i + len(part)] = self.forward_packed(ids, cu)[1]
        return out.cpu().numpy()

    def encode(self, texts, batch_size: int = 32) -> np.ndarray:
        return self.encode_ids(self.tokenize(texts), batch_size)
