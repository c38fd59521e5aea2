"""Item-text encoding rate on MI355X: src/preprocessing/sbert.py's SbertEncoder (the K22 kernels and hvae_gemm_f32,
sequences packed without padding) at the all-MiniLM-L6-v2 shape with seeded random weights, beside a plain torch
restatement of the same encoder on the same device (fp32, sequences sorted by length and padded per batch with an
additive mask, as SentenceTransformer.encode runs them). There is no earlier path of this project to compare with.

    python scripts/bench_sbert.py [--shape minilm-l6|mpnet-base] [--texts 32768] [--batch-sizes 32 256] [--reps 5]
                                  [--warmup 1] [--no-torch]

--shape mpnet-base is the all-mpnet-base-v2 shape (12 layers, H = 768, 12 heads of 64, FFN 3072, lengths clipped to
384): the MPNet body, whose attention adds a relative-position bias (hvae_sbert_attention_relbias), beside the torch
restatement with the same bias. Its attention is also timed on its own, with the bias and through the unbiased kernel
on the same qkv and packs (device events around each call, the two kernels alternating, 12 calls each per pass): the
unbiased time is the bar, the bias adds LDS reads and adds but no MFMA.

Token counts per text (with [CLS] and [SEP]) are drawn from round(lognormal(mean = log 48, sigma = 0.8)) clipped to
4 .. the model's max_seq_length (256, or 384 for mpnet-base), seed 0: short titles to reviews that hit the limit.
Tokenisation is host work and is not timed here; both paths get the same ids.

One JSON line per batch size: texts/s and tokens/s of both paths over whole passes of the set (host clock around
work that ends in a synchronise), the whole-program fp32 rate those imply (operations counted from the shapes; not
a kernel's share of peak), us per stage and pass from device events in a run of their own, and the largest
difference between the two paths' embeddings.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "recommendation-system_amd")]

import torch  # noqa: E402

SHAPES = {"minilm-l6": dict(H=384, heads=12, layers=6, inter=1536, vocab=30522, max_pos=512, max_seq=256, eps=1e-12),
          "mpnet-base": dict(H=768, heads=12, layers=12, inter=3072, vocab=30527, max_pos=514, max_seq=384, eps=1e-5,
                             model_type="mpnet")}
SHAPE = dict(SHAPES["minilm-l6"])  # main() replaces it with --shape's


def random_mpnet_model():
    from src.preprocessing.sbert import LAYER_NAMES, REL_BIAS, SbertModel
    g = np.random.default_rng(0)
    H, I, heads = SHAPE["H"], SHAPE["inter"], SHAPE["heads"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    t = {"embeddings.word_embeddings.weight": f32(g.standard_normal((SHAPE["vocab"], H))),
         "embeddings.position_embeddings.weight": f32(0.5 * g.standard_normal((SHAPE["max_pos"], H))),
         "embeddings.LayerNorm.weight": f32(np.ones(H)), "embeddings.LayerNorm.bias": f32(np.zeros(H)),
         REL_BIAS: f32(g.standard_normal((32, heads)))}
    nq, nk, nv, no, nln = LAYER_NAMES["mpnet"]
    for i in range(SHAPE["layers"]):
        p = f"encoder.layer.{i}."
        for n, (o, k) in {nq: (H, H), nk: (H, H), nv: (H, H), no: (H, H), "intermediate.dense": (I, H),
                          "output.dense": (H, I)}.items():
            t[p + n + ".weight"] = f32(g.standard_normal((o, k)) / np.sqrt(k))
            t[p + n + ".bias"] = f32(0.1 * g.standard_normal(o))
        for n in (nln, "output.LayerNorm"):
            t[p + n + ".weight"], t[p + n + ".bias"] = f32(np.ones(H)), f32(np.zeros(H))
    vocab = ["<s>", "<pad>", "</s>", "<unk>", "[UNK]"] + [f"w{i}" for i in range(SHAPE["vocab"] - 6)] + ["<mask>"]
    return SbertModel(path=None, hidden_size=H, heads=heads, layers=SHAPE["layers"], intermediate_size=I,
                      max_position=SHAPE["max_pos"], layer_norm_eps=SHAPE["eps"], max_seq_length=SHAPE["max_seq"],
                      do_lower_case=True, lower_text=False, vocab=vocab, tensors=t, model_type="mpnet")


def random_model():
    if SHAPE.get("model_type") == "mpnet":
        return random_mpnet_model()
    from src.preprocessing.sbert import SbertModel
    g = np.random.default_rng(0)
    H, I = SHAPE["H"], SHAPE["inter"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    t = {"embeddings.word_embeddings.weight": f32(g.standard_normal((SHAPE["vocab"], H))),
         "embeddings.position_embeddings.weight": f32(0.5 * g.standard_normal((SHAPE["max_pos"], H))),
         "embeddings.token_type_embeddings.weight": f32(0.5 * g.standard_normal((2, H))),
         "embeddings.LayerNorm.weight": f32(np.ones(H)), "embeddings.LayerNorm.bias": f32(np.zeros(H))}
    for i in range(SHAPE["layers"]):
        p = f"encoder.layer.{i}."
        for n, (o, k) in {"attention.self.query": (H, H), "attention.self.key": (H, H),
                          "attention.self.value": (H, H), "attention.output.dense": (H, H),
                          "intermediate.dense": (I, H), "output.dense": (H, I)}.items():
            t[p + n + ".weight"] = f32(g.standard_normal((o, k)) / np.sqrt(k))
            t[p + n + ".bias"] = f32(0.1 * g.standard_normal(o))
        for n in ("attention.output.LayerNorm", "output.LayerNorm"):
            t[p + n + ".weight"], t[p + n + ".bias"] = f32(np.ones(H)), f32(np.zeros(H))
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(SHAPE["vocab"] - 5)]
    return SbertModel(path=None, hidden_size=H, heads=SHAPE["heads"], layers=SHAPE["layers"], intermediate_size=I,
                      max_position=SHAPE["max_pos"], layer_norm_eps=SHAPE["eps"], max_seq_length=SHAPE["max_seq"],
                      do_lower_case=True, lower_text=False, vocab=vocab, tensors=t)


def draw_sequences(n: int):
    g = np.random.default_rng(0)
    lens = np.clip(np.rint(g.lognormal(np.log(48.0), 0.8, size=n)), 4, SHAPE["max_seq"]).astype(np.int64)
    seqs = []
    for ln in lens:
        mpnet = SHAPE.get("model_type") == "mpnet"  # ids 0 .. 4 and, in MPNet's vocabulary, the last are special
        row = g.integers(5, SHAPE["vocab"] - (1 if mpnet else 0), size=ln)
        row[0], row[-1] = (0, 2) if mpnet else (2, 3)
        seqs.append(row)
    return seqs, lens


def flops(lens: np.ndarray) -> float:
    """fp32 operations of the encoder body: the four linear layers per token and layer, and QK^T + PV per head."""
    H, I, L = SHAPE["H"], SHAPE["inter"], SHAPE["layers"]
    per_token = 2 * H * 3 * H + 2 * H * H + 2 * 2 * H * I
    return float(L * (per_token * lens.sum() + 4 * H * (lens.astype(np.float64) ** 2).sum()))


class TorchEncoder:
    """The same encoder in plain torch operators: padded batches, additive mask, fp32. For an MPNet body the
    positions start at row 2, there is no token type and every score gets the relative-position bias."""

    def __init__(self, model, device):
        from src.preprocessing.sbert import LAYER_NAMES, REL_BIAS, relative_bias_table
        self.m, self.dev = model, device
        self.t = {k: torch.as_tensor(v, device=device) for k, v in model.tensors.items()}
        self.names = LAYER_NAMES[model.model_type]
        self.mpnet = model.model_type == "mpnet"
        if self.mpnet:
            self.rel_len = model.max_seq_length
            self.rel = torch.as_tensor(relative_bias_table(model.tensors[REL_BIAS], self.rel_len), device=device)

    @torch.no_grad()
    def batch(self, seqs):
        F, t, m = torch.nn.functional, self.t, self.m
        B, Lmax = len(seqs), max(len(s) for s in seqs)
        ids = np.zeros((B, Lmax), np.int64)
        mask = np.zeros((B, Lmax), np.float32)
        for i, s in enumerate(seqs):
            ids[i, :len(s)], mask[i, :len(s)] = s, 1.0
        ids, mask = torch.as_tensor(ids, device=self.dev), torch.as_tensor(mask, device=self.dev)
        H, nh = m.hidden_size, m.heads
        nq, nk, nv, no, nln = self.names
        if self.mpnet:
            x = t["embeddings.word_embeddings.weight"][ids] + t["embeddings.position_embeddings.weight"][2:2 + Lmax]
        else:
            x = t["embeddings.word_embeddings.weight"][ids] + t["embeddings.position_embeddings.weight"][:Lmax] \
                + t["embeddings.token_type_embeddings.weight"][0]
        x = F.layer_norm(x, (H,), t["embeddings.LayerNorm.weight"], t["embeddings.LayerNorm.bias"], m.layer_norm_eps)
        add = (1.0 - mask)[:, None, None, :] * torch.finfo(torch.float32).min
        if self.mpnet:  # one [heads, Lmax, Lmax] gather per batch, as MPNetEncoder.compute_position_bias
            pos = torch.arange(Lmax, device=self.dev)
            add = add + self.rel[:, pos[None, :] - pos[:, None] + self.rel_len - 1][None]
        for i in range(m.layers):
            p = f"encoder.layer.{i}."
            q, k, v = (F.linear(x, t[p + n + ".weight"], t[p + n + ".bias"])
                       .view(B, Lmax, nh, H // nh).transpose(1, 2) for n in (nq, nk, nv))
            pr = torch.softmax(q @ k.transpose(-1, -2) / (H // nh) ** 0.5 + add, dim=-1)
            ctx = (pr @ v).transpose(1, 2).reshape(B, Lmax, H)
            a = F.linear(ctx, t[p + no + ".weight"], t[p + no + ".bias"])
            x = F.layer_norm(a + x, (H,), t[p + nln + ".weight"], t[p + nln + ".bias"], m.layer_norm_eps)
            f = F.gelu(F.linear(x, t[p + "intermediate.dense.weight"], t[p + "intermediate.dense.bias"]))
            o = F.linear(f, t[p + "output.dense.weight"], t[p + "output.dense.bias"])
            x = F.layer_norm(o + x, (H,), t[p + "output.LayerNorm.weight"], t[p + "output.LayerNorm.bias"],
                             m.layer_norm_eps)
        pooled = (x * mask[:, :, None]).sum(dim=1) / mask.sum(dim=1, keepdim=True).clamp_min(1e-9)
        return F.normalize(pooled, p=2, dim=1)

    def encode_ids(self, seqs, batch_size):
        order = np.argsort([-len(s) for s in seqs], kind="stable")  # SentenceTransformer.encode sorts by length
        out = torch.empty(len(seqs), self.m.hidden_size, device=self.dev)
        for i in range(0, len(seqs), batch_size):
            idx = order[i:i + batch_size]
            out[torch.as_tensor(idx, device=self.dev)] = self.batch([seqs[j] for j in idx])
        return out.cpu().numpy()


def timed(fn, warmup: int, reps: int):
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return out, float(np.median(times))


def attention_ab(enc, seqs, bs: int) -> dict:
    """The attention of every pass over the set on its own: the biased and the unbiased kernel on the same seeded
    qkv and the same packs, alternating, as many calls each per pass as the model has layers; device events around
    each call, summed, per pass. One run; the first pass is run once untimed for both kernels."""
    from hvae import ops
    m = enc.model
    g = torch.Generator(device=enc.device).manual_seed(0)
    us = {"biased": 0.0, "unbiased": 0.0}
    events = []
    passes = range(0, len(seqs), bs)
    for n, i in enumerate([0] + list(passes)):
        part = seqs[i:i + bs]
        cu = np.concatenate([[0], np.cumsum([len(s) for s in part])])
        pack = ops.SbertPack(np.zeros(int(cu[-1]), np.int64), cu, enc.device)
        qkv = torch.randn(pack.T, 3 * m.hidden_size, device=enc.device, generator=g)
        ctx = torch.empty(pack.T, m.hidden_size, device=enc.device)
        for _ in range(m.layers):
            for kind in ("unbiased", "biased"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if kind == "biased":
                    ops.sbert_attention(qkv, pack, m.heads, ctx, enc.rel, enc.rel_len)
                else:
                    ops.sbert_attention(qkv, pack, m.heads, ctx)
                b.record()
                if n:  # the first visit is the warm-up
                    events.append((kind, a, b))
        torch.cuda.synchronize()
        for kind, a, b in events:
            us[kind] += a.elapsed_time(b) * 1e3
        events.clear()
    return {"attention_biased_us_per_pass": round(us["biased"] / len(passes), 1),
            "attention_unbiased_us_per_pass": round(us["unbiased"] / len(passes), 1),
            "biased_over_unbiased": round(us["biased"] / us["unbiased"], 4),
            "method": "device events per call, kernels alternating, one run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="minilm-l6")
    ap.add_argument("--texts", type=int, default=32768)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    SHAPE.clear()
    SHAPE.update(SHAPES[args.shape])
    if not torch.cuda.is_available():
        raise SystemExit("bench_sbert: no HIP device; this measurement has no CPU fallback")
    from src.preprocessing.sbert import SbertEncoder
    dev = torch.device("cuda", 0)
    model = random_model()
    enc = SbertEncoder(model, dev)
    ref = None if args.no_torch else TorchEncoder(model, dev)
    seqs, lens = draw_sequences(args.texts)
    ops = flops(lens)
    for bs in args.batch_sizes:
        emb, t_hip = timed(lambda: enc.encode_ids(seqs, bs), args.warmup, args.reps)
        enc.stage_events = []
        enc.encode_ids(seqs, bs)
        torch.cuda.synchronize()
        passes = -(-len(seqs) // bs)
        stage_us = {s: 0.0 for s in enc.STAGES}
        for name, a, b in enc.stage_events:
            stage_us[name] += a.elapsed_time(b) * 1e3
        enc.stage_events = None
        row = {"bench": "sbert_encode", "shape": SHAPE, "texts": len(seqs), "tokens": int(lens.sum()),
               "length_distribution": f"round(lognormal(log 48, 0.8)) clipped to 4..{SHAPE['max_seq']}, seed 0",
               "mean_tokens": round(float(lens.mean()), 1), "batch_size": bs, "reps": args.reps,
               "warmup": args.warmup,
               "hip": {"seconds": round(t_hip, 4), "texts_per_s": round(len(seqs) / t_hip, 1),
                       "tokens_per_s": round(float(lens.sum()) / t_hip, 1),
                       "whole_program_tflops": round(ops / t_hip / 1e12, 2)},
               "hip_stage_us_per_pass": {k: round(v / passes, 1) for k, v in stage_us.items()},
               "hip_stage_us_per_pass_total": round(sum(stage_us.values()) / passes, 1)}
        if enc.rel is not None:
            row["attention_ab"] = attention_ab(enc, seqs, bs)
        if ref is not None:
            emb_t, t_torch = timed(lambda: ref.encode_ids(seqs, bs), args.warmup, args.reps)
            padded = sum(max(len(seqs[j]) for j in idx) * len(idx) for idx in
                         (np.argsort([-len(s) for s in seqs], kind="stable")[i:i + bs]
                          for i in range(0, len(seqs), bs)))
            row["torch"] = {"version": torch.__version__, "seconds": round(t_torch, 4),
                            "texts_per_s": round(len(seqs) / t_torch, 1),
                            "tokens_per_s": round(float(lens.sum()) / t_torch, 1), "padded_tokens": int(padded)}
            row["torch_over_hip_seconds"] = round(t_torch / t_hip, 2)
            row["max_abs_diff_hip_torch"] = float(np.abs(emb.astype(np.float64) - emb_t).max())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
