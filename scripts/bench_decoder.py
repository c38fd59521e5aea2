"""Standalone timing of the streaming decoder sweep (hvae_decoder_fwd with O) on one shape.

    python scripts/bench_decoder.py [--nb 4096] [--N 100000] [--D 384] [--dtype bf16|fp8|fp32] [--reps 20]

U rows are random with |u| ~ 4 (the scale trained projections reach), E is L2-normalised
random. The library's probe brackets every sweep launch with a hipEvent pair on its stream;
TFLOP/s counts the algorithmic 4 * nb * N * D of the sweep (S = U E^T and O = P E).
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "recommendation-system_amd")]

import torch  # noqa: E402

from hvae import _lib, ops  # noqa: E402
from hvae._lib import check, lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=4096)
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--D", type=int, default=384)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="time hvae_decoder_train (sweep + finalize with the CSR "
                                                          "batch's sparse terms) instead of hvae_decoder_fwd")
    ap.add_argument("--probe", default="decoder_sweep", choices=["decoder_sweep", "decoder_finalize"])
    ap.add_argument("--ab", nargs="*", default=[], help="A/B arms in one process: each arm a comma list of "
                    "ENV=VAL settings read by the A/B library (HVAE_LIB=build_var/libhvae_ab.so; e.g. HVAE_DEC_V3=0), timed in "
                    "interleaved rounds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lam", type=float, default=3.0, help="--train: CSR entries per user 5 + Poisson(lam) (15 at "
                                                           "the synthetic workloads)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    E32 = torch.randn(args.N, args.D, device=dev, generator=g)
    E32 /= E32.norm(dim=1, keepdim=True)
    U = torch.randn(args.nb, args.D, device=dev, generator=g) * (4.0 / args.D ** 0.5)
    if args.dtype == "fp32":
        E, enorm = E32, None
    else:
        from hvae import _lib
        E = ops.decoder_image(E32, _lib.HVAE_FP8 if args.dtype == "fp8" else _lib.HVAE_BF16)
        enorm = ops.row_norm_max(E)
    if args.train:
        sys.path.insert(0, str(ROOT / "tests" / "golden"))
        from gen import synth_csr
        x = ops.csr_from_scipy(synth_csr(args.nb, args.N, lam=args.lam, seed=5), dev)
        step = lambda: ops.decoder_train(x, U, E, enorm, E32, 1.0 / args.nb)  # noqa: E731
    else:
        step = lambda: ops.decoder_fwd(U, E, enorm)  # noqa: E731
    import os

    def timed(label):
        step()  # warm-up (and kernel attributes)
        torch.cuda.synchronize()
        check(lib().hvae_probe_arm(args.probe.encode(), 4 * args.reps), "probe_arm")
        for _ in range(args.reps):
            step()
        torch.cuda.synchronize()
        avg, n = C.c_double(), C.c_int()
        check(lib().hvae_probe_collect(C.byref(avg), C.byref(n)), "probe_collect")
        check(lib().hvae_probe_arm(None, 0), "probe_disarm")
        us = avg.value
        flops = 4.0 * args.nb * args.N * args.D
        print(json.dumps({"nb": args.nb, "N": args.N, "D": args.D, "dtype": args.dtype, "probe": args.probe,
                          "train": args.train, "arm": label, "launches": n.value,
                          "avg_us": round(us, 2), "tflops": round(flops / us / 1e6, 1)}), flush=True)

    if not args.ab:
        timed("")
        return
    for _ in range(args.rounds):
        for arm in args.ab:
            for kv in arm.split(","):
                k, v = kv.split("=")
                os.environ[k] = v
            timed(arm)


if __name__ == "__main__":
    main()
