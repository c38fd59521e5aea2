"""Records what the fused top-K's host side answers on a grid, through the one query every revision of the library
has: hvae_topk_fused_workspace (for fixed R it is strictly increasing in the segment count splits x (2 or 8), so it
pins the launch geometry the call derives beside it).

    python tests/golden/make_topk_plan_fixture.py --product recommendation-system_amd/hvae/libhvae.so \
        --ab build_var/libhvae_ab.so --out tests/golden/topk_plan_parent.json

was run on the libraries of the commit before the launch became one pure function (tk_plan in csrc/hvae_topk.hip);
tests/test_topk_plan_cpu.py holds every later library to that record. One child process per environment setting,
as tests/golden/make_decoder_plan_fixture.py does.

The file: {"product": [workspace, ...] in grid() order, "ab": {setting name: the same list for "default", and for
every other setting only the points that differ from "default", as {grid index: workspace}}}.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

RS = (0, 1, 31, 32, 33, 64, 65, 128, 129, 1000, 4096, 100_000)
NS = (1, 31, 32, 33, 128, 4097, 12101, 100_000, 1_000_000, 10_000_000, 600_000_000, 2_000_000_000)
# every served width, and two that are not (96, 2048)
DS = (64, 96, 128, 256, 384, 512, 768, 1024, 2048)
KS = (1, 20, 256)

# name -> the switches it sets (A/B library only; the product library ignores the environment)
SETTINGS = {
    "default": {},
    "LDS=0": {"HVAE_TOPK_LDS": 0},
    "LDS=0 WAVE_USERS=0": {"HVAE_TOPK_LDS": 0, "HVAE_TOPK_WAVE_USERS": 0},
    "WAVE_USERS=0": {"HVAE_TOPK_WAVE_USERS": 0},
    "TAU_PERIOD=4": {"HVAE_TK_TAU_PERIOD": 4},
    "TAU_PERIOD=3": {"HVAE_TK_TAU_PERIOD": 3},  # not a power of two: falls back to 8
}
SWITCHES = ("HVAE_TOPK_LDS", "HVAE_TOPK_WAVE_USERS", "HVAE_TK_TAU_PERIOD")


def grid():
    """(R, N, D, K) in the fixture's order."""
    return [(R, N, D, K) for D in DS for R in RS for N in NS for K in KS]


def setting_env(name, lib_path):
    """The environment of a child process that plans under setting `name` with the library at lib_path."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update({k: str(v) for k, v in SETTINGS[name].items()})
    env["HVAE_LIB"] = str(lib_path)
    return env


def old_query(L):
    """[hvae_topk_fused_workspace, ...] over grid() from the loaded library L."""
    L.hvae_topk_fused_workspace.restype = C.c_size_t
    L.hvae_topk_fused_workspace.argtypes = [C.c_int64] * 4
    return [int(L.hvae_topk_fused_workspace(*g)) for g in grid()]


def _child(lib_path, name):
    r = subprocess.run([sys.executable, __file__, "--worker"], env=setting_env(name, lib_path), check=True,
                       capture_output=True, text=True)
    return json.loads(r.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help="print old_query of $HVAE_LIB under this environment")
    ap.add_argument("--product")
    ap.add_argument("--ab")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(old_query(C.CDLL(os.environ["HVAE_LIB"]))))
        return
    rec = {"product": _child(a.product, "default"), "ab": {}}
    base = rec["ab"]["default"] = _child(a.ab, "default")
    for name in SETTINGS:
        if name != "default":
            got = _child(a.ab, name)
            rec["ab"][name] = {str(i): v for i, (v, b) in enumerate(zip(got, base)) if v != b}
    with open(a.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in rec["ab"].items()}, len(rec["product"]))


if __name__ == "__main__":
    main()
