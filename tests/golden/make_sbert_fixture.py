"""Writes tests/golden/sbert.npz, sbert_meta.json and sbert_vocab.txt: the truth for the SBERT item encoder (K22).

Run on the CPU:  python tests/golden/make_sbert_fixture.py

Truth comes from the installed transformers and torch, never from the code under test:
  * the encoder: BertModel(BertConfig(...), add_pooling_layer=False) with eager attention in float64, loaded with the
    weights tests/sbert_ref.py draws, run one sequence at a time (no padding, no mask), then mean pooling and L2
    normalisation in float64;
  * the kernels: torch's float64 layer_norm, softmax and matmul on the inputs tests/sbert_ref.py draws;
  * the tokenizer: transformers.BertTokenizer over the synthetic vocabulary written here.
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

WORDS = """the toy game play great kids cafe resume naive no text fun puzzle train wooden set love super for and with
car a i it is of to in this my our was very good best little big red blue box piece pieces board card cards dice
Toy LEGO Great The""".split()
SUFFIXES = """##ing ##ed ##s ##er ##ly ##d ##e ##es ##y ##un ##able ##ful ##oo ##zz ##le""".split()
PUNCT = list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~") + ["’", "…", "。"]
CJK = list("玩具好")

# (text, what it exercises); every case is tokenised with do_lower_case True and False, max length 512, and the
# last one also at max length 12
TOKENIZER_CASES = [
    "The great wooden toy train set!",
    "Café résumé naïve",
    "fun!!! ...really?? (yes) -- $9.99/50% off",
    "玩具 is 好玩具toy",
    "null\x00byte\tand\ttabs\u00a0nbsp\u2028line\x07bell\ufffdrepl\u200bzw\u0085nel",
    "x" * 120 + " play",
    "a" * 100 + " " + "a" * 101,
    "first part [SEP] second part [CLS][MASK] [UNK] [PAD] [sep]",
    "[NO TEXT]",
    "",
    "   ",
    "playing played plays unplayable zzz qqq toys LEGO Toy TOY",
    "don't stop-me now’s … end。",
    "super " * 30,
]
TRUNCATE_AT = 12


def write_vocab() -> list[str]:
    import string
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += list(string.ascii_lowercase) + list(string.digits) + list("TLGE")
    vocab += ["##" + c for c in string.ascii_lowercase + string.digits]
    vocab += PUNCT + CJK + WORDS + SUFFIXES
    seen, out = set(), []
    for v in vocab:
        if v not in seen:
            seen.add(v)
            out.append(v)
    (HERE / "sbert_vocab.txt").write_text("\n".join(out) + "\n", encoding="utf-8")
    return out


def err(a: torch.Tensor, truth: torch.Tensor) -> float:
    return float((a.double() - truth).abs().max())


def bert(name: str, dtype):
    from transformers import BertConfig, BertModel
    import sbert_ref as R
    cfg = R.config_json(name)
    cfg = {k: v for k, v in cfg.items() if k not in ("model_type", "architectures")}
    cfg.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertModel(BertConfig(**cfg, attn_implementation="eager"), add_pooling_layer=False)
    sd = {k: torch.from_numpy(v) for k, v in R.weights(name).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    return model.to(dtype).eval()


def run_bert(model, ids, cu):
    hid = []
    with torch.no_grad():
        for s in range(len(cu) - 1):
            row = torch.from_numpy(ids[cu[s]:cu[s + 1]].astype(np.int64))[None]
            hid.append(model(input_ids=row, attention_mask=torch.ones_like(row)).last_hidden_state[0])
    pooled = torch.stack([h.mean(dim=0) for h in hid])
    return torch.cat(hid), pooled / pooled.norm(dim=1, keepdim=True).clamp_min(1e-12)


def torch_attention(qkv: torch.Tensor, cu, heads: int) -> torch.Tensor:
    H = qkv.shape[1] // 3
    dh = H // heads
    out = torch.empty(qkv.shape[0], H, dtype=qkv.dtype)
    for s in range(len(cu) - 1):
        a, b = int(cu[s]), int(cu[s + 1])
        q, k, v = (qkv[a:b, i * H:(i + 1) * H].reshape(b - a, heads, dh).transpose(0, 1) for i in range(3))
        p = torch.softmax(q @ k.transpose(1, 2) / dh ** 0.5, dim=-1)
        out[a:b] = (p @ v).transpose(0, 1).reshape(b - a, H)
    return out


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vocab = write_vocab()
    import sbert_ref as R
    out, meta = {}, {"transformers": None, "torch": torch.__version__, "vocab_size": len(vocab)}
    import transformers
    meta["transformers"] = transformers.__version__
    for key in ("embedding", "hidden", "attention", "ln", "pool", "embed_ln"):
        meta[f"fp32_ref_err_{key}"] = {}
    meta["logit_row_std"] = {}

    # ---- the whole encoder
    for name, (H, heads, _) in R.CONFIGS.items():
        ids, cu = R.encoder_ids(name)
        hid64, emb64 = run_bert(bert(name, torch.float64), ids, cu)
        hid32, emb32 = run_bert(bert(name, torch.float32), ids, cu)
        out[f"{name}_ids"], out[f"{name}_cu"] = ids, cu
        out[f"{name}_emb"] = emb64.numpy()
        out[f"{name}_hidden_rows"] = hid64.numpy()[R.sample_rows(cu)]
        meta["fp32_ref_err_embedding"][name] = err(emb32, emb64)
        meta["fp32_ref_err_hidden"][name] = err(hid32, hid64)
        # the layer-0 logits of the longest sequence: a flat softmax would hide a wrong score
        qkv = R.encode(R.weights(name), heads, ids, cu, want_logits=True)
        a, b, dh = int(cu[-2]), int(cu[-1]), H // heads
        logits = qkv[a:b, :dh] @ qkv[a:b, H:H + dh].T / np.sqrt(dh)
        std = float(logits.std(axis=1).mean())
        assert std >= 1.0, std
        meta["logit_row_std"][name] = std

    # ---- attention
    for case, (H, heads, _) in R.ATT_CASES.items():
        qkv, cu, heads = R.attention_input(case)
        t64 = torch_attention(torch.from_numpy(qkv).double(), cu, heads)
        t32 = torch_attention(torch.from_numpy(qkv), cu, heads)
        out[f"att_{case}_rows"] = t64.numpy()[R.sample_rows(cu)]
        meta["fp32_ref_err_attention"][case] = err(t32, t64)

    # ---- LayerNorm of a sum, embedding + LayerNorm, pooling
    F = torch.nn.functional
    for H in R.LN_WIDTHS:
        d = {k: torch.from_numpy(v) for k, v in R.ln_input(H).items()}
        t64 = F.layer_norm(d["x"].double() + d["res"].double(), (H,), d["w"].double(), d["b"].double(), R.LN_EPS)
        t32 = F.layer_norm(d["x"] + d["res"], (H,), d["w"], d["b"], R.LN_EPS)
        out[f"ln_{H}"] = t64.numpy()
        meta["fp32_ref_err_ln"][str(H)] = err(t32, t64)
    d = R.embed_input()
    pos = np.concatenate([np.arange(n) for n in R.KERNEL_LENS])
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    idx, pidx = t["ids"].long(), torch.from_numpy(pos)
    x64 = t["word"].double()[idx] + t["pos"].double()[pidx] + t["type0"].double()
    x32 = t["word"][idx] + t["pos"][pidx] + t["type0"]
    t64 = F.layer_norm(x64, (R.EMB_H,), t["w"].double(), t["b"].double(), R.LN_EPS)
    t32 = F.layer_norm(x32, (R.EMB_H,), t["w"], t["b"], R.LN_EPS)
    out["embed_rows"] = t64.numpy()[R.sample_rows(d["cu"])]
    meta["fp32_ref_err_embed_ln"][str(R.EMB_H)] = err(t32, t64)
    for H in R.LN_WIDTHS[1:]:
        x, cu = R.pool_input(H)

        def pool(xt):
            m = torch.stack([xt[cu[s]:cu[s + 1]].mean(dim=0) for s in range(len(cu) - 1)])
            return m / m.norm(dim=1, keepdim=True).clamp_min(1e-12)
        t64, t32 = pool(torch.from_numpy(x).double()), pool(torch.from_numpy(x))
        out[f"pool_{H}"] = t64.numpy()
        meta["fp32_ref_err_pool"][str(H)] = err(t32, t64)

    # ---- the tokenizer
    from transformers import BertTokenizer
    tok = {}
    for lower in (True, False):
        bt = BertTokenizer(str(HERE / "sbert_vocab.txt"), do_lower_case=lower)
        key = "lower" if lower else "cased"
        tok[key] = [bt(text, truncation=True, max_length=512)["input_ids"] for text in TOKENIZER_CASES]
        tok[key + f"_max{TRUNCATE_AT}"] = [bt(text, truncation=True, max_length=TRUNCATE_AT)["input_ids"]
                                          for text in TOKENIZER_CASES]
    meta["tokenizer_cases"] = TOKENIZER_CASES
    meta["tokenizer_ids"] = tok
    meta["truncate_at"] = TRUNCATE_AT

    np.savez(HERE / "sbert.npz", **out)
    (HERE / "sbert_meta.json").write_text(json.dumps(meta, indent=1, ensure_ascii=True) + "\n")
    size = (HERE / "sbert.npz").stat().st_size
    assert size < 1 << 20, size
    print(json.dumps({k: v for k, v in meta.items() if k.startswith(("fp32", "logit"))}, indent=1), size)


if __name__ == "__main__":
    main()
