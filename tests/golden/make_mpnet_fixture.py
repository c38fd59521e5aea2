"""Writes tests/golden/mpnet.npz, mpnet_meta.json and mpnet_vocab.txt: the truth for the MPNet body of the SBERT item
encoder (hvae_sbert_attention_relbias and the MPNet branch of src/preprocessing/sbert.py).

Run on the CPU:  python tests/golden/make_mpnet_fixture.py

Truth comes from the installed transformers and torch, never from the code under test:
  * the encoder: MPNetModel(MPNetConfig(...), add_pooling_layer=False) with eager attention in float64, loaded with
    the weights tests/mpnet_ref.py draws, run one sequence at a time (no padding, no mask), then mean pooling and L2
    normalisation in float64;
  * the bucket table: MPNetEncoder.relative_position_bucket over the deltas -511 .. 511;
  * the attention kernel: torch's float64 softmax and matmul with an additive table gathered at (j - i) + L - 1, on
    the inputs tests/mpnet_ref.py draws (the table drawn per delta, not through buckets);
  * the tokenizer: transformers.MPNetTokenizer over the synthetic vocabulary written here.
Beside each truth the error of torch's own CPU float32 run of the same computation is recorded (max |difference|);
the device tests allow 8 x that. The npz keeps the embeddings in full and the larger arrays at sbert_ref.sample_rows.
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

from make_sbert_fixture import CJK, PUNCT, SUFFIXES, TOKENIZER_CASES as BERT_CASES, WORDS, err  # noqa: E402

# the BERT fixture's awkward strings, then MPNet's special tokens literally in the text (never <pad>: a pad id
# inside a sequence does not advance transformers' position, a known deviation of the packed encoder)
TOKENIZER_CASES = BERT_CASES + [
    "first part </s> second part <s><mask> [UNK] </S> <MASK>",
    "a toy<mask>game <s>play</s>",
    "<s></s><mask>",
    "toy < s > game </ s> <mask",
]
TRUNCATE_AT = 12


def write_vocab() -> list[str]:
    import string
    import mpnet_ref as M
    vocab = [M.CLS, M.PAD, M.SEP, M.UNK_ALT, M.UNK]
    vocab += list(string.ascii_lowercase) + list(string.digits) + list("TLGE")
    vocab += ["##" + c for c in string.ascii_lowercase + string.digits]
    vocab += PUNCT + CJK + WORDS + SUFFIXES + [M.MASK]
    seen, out = set(), []
    for v in vocab:
        if v not in seen:
            seen.add(v)
            out.append(v)
    (HERE / "mpnet_vocab.txt").write_text("\n".join(out) + "\n", encoding="utf-8")
    return out


def mpnet(name: str, dtype):
    from transformers import MPNetConfig, MPNetModel
    import mpnet_ref as M
    cfg = {k: v for k, v in M.config_json(name).items() if k not in ("model_type", "architectures")}
    cfg.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = MPNetModel(MPNetConfig(**cfg, attn_implementation="eager"), add_pooling_layer=False)
    sd = {k: torch.from_numpy(v) for k, v in M.weights(name).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    return model.to(dtype).eval()


def run_mpnet(model, ids, cu):
    hid = []
    with torch.no_grad():
        for s in range(len(cu) - 1):
            row = torch.from_numpy(ids[cu[s]:cu[s + 1]].astype(np.int64))[None]
            hid.append(model(input_ids=row, attention_mask=torch.ones_like(row)).last_hidden_state[0])
    pooled = torch.stack([h.mean(dim=0) for h in hid])
    return torch.cat(hid), pooled / pooled.norm(dim=1, keepdim=True).clamp_min(1e-12)


def torch_attention(qkv: torch.Tensor, cu, heads: int, rel: torch.Tensor, L: int) -> torch.Tensor:
    H = qkv.shape[1] // 3
    dh = H // heads
    out = torch.empty(qkv.shape[0], H, dtype=qkv.dtype)
    for s in range(len(cu) - 1):
        a, b = int(cu[s]), int(cu[s + 1])
        q, k, v = (qkv[a:b, i * H:(i + 1) * H].reshape(b - a, heads, dh).transpose(0, 1) for i in range(3))
        pos = torch.arange(b - a)
        bias = rel[:, pos[None, :] - pos[:, None] + L - 1]  # [heads, query, key]
        p = torch.softmax(q @ k.transpose(1, 2) / dh ** 0.5 + bias, dim=-1)
        out[a:b] = (p @ v).transpose(0, 1).reshape(b - a, H)
    return out


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vocab = write_vocab()
    import transformers
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    import mpnet_ref as M
    import sbert_ref as R
    out, meta = {}, {"transformers": transformers.__version__, "torch": torch.__version__, "vocab_size": len(vocab)}
    for key in ("embedding", "hidden", "attention"):
        meta[f"fp32_ref_err_{key}"] = {}
    meta["logit_row_std"] = {}

    # ---- the whole encoder
    for name, (H, heads, _) in M.CONFIGS.items():
        ids, cu = M.encoder_ids(name)
        hid64, emb64 = run_mpnet(mpnet(name, torch.float64), ids, cu)
        hid32, emb32 = run_mpnet(mpnet(name, torch.float32), ids, cu)
        out[f"{name}_ids"], out[f"{name}_cu"] = ids, cu
        out[f"{name}_emb"] = emb64.numpy()
        out[f"{name}_hidden_rows"] = hid64.numpy()[R.sample_rows(cu)]
        meta["fp32_ref_err_embedding"][name] = err(emb32, emb64)
        meta["fp32_ref_err_hidden"][name] = err(hid32, hid64)
        # the layer-0 logits (before the bias) of the longest sequence: a flat softmax would hide a wrong score
        qkv = M.encode(M.weights(name), heads, ids, cu, want_logits=True)
        a, b, dh = int(cu[-2]), int(cu[-1]), H // heads
        logits = qkv[a:b, :dh] @ qkv[a:b, H:H + dh].T / np.sqrt(dh)
        std = float(logits.std(axis=1).mean())
        assert std >= 1.0, std
        meta["logit_row_std"][name] = std

    # ---- the bucket table
    delta = torch.arange(-(M.REL_L - 1), M.REL_L)
    table = MPNetEncoder.relative_position_bucket(delta).numpy()
    assert table.min() == 0 and table.max() == 31
    out["bucket_table"] = table.astype(np.int8)

    # ---- attention with the bias
    for case in M.ATT_CASES:
        qkv, cu, heads, rel = M.attention_input(case)
        t64 = torch_attention(torch.from_numpy(qkv).double(), cu, heads, torch.from_numpy(rel).double(), M.REL_L)
        t32 = torch_attention(torch.from_numpy(qkv), cu, heads, torch.from_numpy(rel), M.REL_L)
        out[f"att_{case}_rows"] = t64.numpy()[R.sample_rows(cu)]
        meta["fp32_ref_err_attention"][case] = err(t32, t64)

    # ---- the tokenizer
    from transformers import MPNetTokenizer
    tok = {}
    ids_of = {t: i for i, t in enumerate(vocab)}
    for lower in (True, False):
        mt = MPNetTokenizer(vocab=dict(ids_of), do_lower_case=lower, unk_token=M.UNK)
        key = "lower" if lower else "cased"
        tok[key] = [mt(text, truncation=True, max_length=512)["input_ids"] for text in TOKENIZER_CASES]
        tok[key + f"_max{TRUNCATE_AT}"] = [mt(text, truncation=True, max_length=TRUNCATE_AT)["input_ids"]
                                          for text in TOKENIZER_CASES]
    assert not any(ids_of[M.PAD] in row for rows in tok.values() for row in rows)
    meta["tokenizer_cases"] = TOKENIZER_CASES
    meta["tokenizer_ids"] = tok
    meta["truncate_at"] = TRUNCATE_AT

    np.savez(HERE / "mpnet.npz", **out)
    (HERE / "mpnet_meta.json").write_text(json.dumps(meta, indent=1, ensure_ascii=True) + "\n")
    size = sum((HERE / n).stat().st_size for n in ("mpnet.npz", "mpnet_meta.json", "mpnet_vocab.txt"))
    assert size < 1 << 20, size
    print(json.dumps({k: v for k, v in meta.items() if k.startswith(("fp32", "logit"))}, indent=1), size)


if __name__ == "__main__":
    main()
