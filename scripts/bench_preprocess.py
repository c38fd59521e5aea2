"""The index work of `make preprocess` on the device, stage by stage, beside a pandas / scipy restatement on the host.

    python scripts/bench_preprocess.py [--users 1000000] [--items 100000] [--per-user 20] [--out profiles/preprocess_bench.jsonl]

A synthetic review table at scripts/bench_loader.py's shape (1 M users, 100 K items, about 20 M rows: 13-byte user
ids, 10-byte item ids, Zipf item popularity, 0 / 1 ratings, millisecond timestamps). Per stage:
  * device: hvae.ops.prep_encode (users, items), prep_kcore, prep_split, prep_csr on device-resident inputs, the
    median of --repeats runs after one warm-up, each bracketed by a device synchronisation (the read-back of the
    stage's scalar results is inside, the upload of its inputs is not: "upload_s" states that once);
  * host: what the reference's scripts do for the same stage (LabelEncoder's np.unique over the object column,
    value_counts / isin per filter round, the two-key sort_values with the two group-bys, scipy's COO -> CSR), once.
The two results of every stage are compared for equality. One JSON line per stage is appended to --out, each with the
device's name and the host's core count; nothing else in the repository may quote a timing that is not such a line.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "recommendation-system_amd")]


def table(n_users: int, n_items: int, per_user: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    users = np.char.add("A", np.char.zfill(np.arange(n_users).astype(str), 12))
    items = np.char.add("B0", np.char.zfill(np.arange(n_items).astype(str), 8))
    cnt = 3 + rng.poisson(per_user - 3, n_users)  # a few users fall below the filter's 5
    uidx = np.repeat(np.arange(n_users), cnt)
    iidx = (rng.zipf(1.3, uidx.size) - 1) % n_items
    order = rng.permutation(uidx.size)  # file order is not user order
    uidx, iidx = uidx[order], iidx[order]
    rating = (rng.integers(1, 6, uidx.size) >= 4).astype(np.float32)
    ts = rng.integers(1_500_000_000_000, 1_700_000_000_000, uidx.size)
    return users, items, uidx, iidx, rating, ts


def timed(fn, repeats: int):
    import torch
    fn()  # warm-up: workspace growth, code load
    times, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return float(np.median(times)), out


def host_once(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--per-user", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="device stages only (no comparison)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "preprocess_bench.jsonl"))
    args = ap.parse_args()

    import pandas as pd
    import torch
    from scipy.sparse import csr_matrix

    from hvae import ops
    dev = torch.device("cuda", 0)
    users, items, uidx, iidx, rating, ts = table(args.users, args.items, args.per_user)
    n = int(uidx.size)
    box = {"device": torch.cuda.get_device_name(0), "host_cores": len(os.sched_getaffinity(0)), "rows": n,
           "users": args.users, "items": args.items}
    print(json.dumps({"table": box}), flush=True)
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def record(stage: str, device_s: float, host_s, equal, **extra):
        line = {"stage": stage, "device_s": round(device_s, 6), "host_s": None if host_s is None else round(host_s, 4),
                "equal": equal, **extra, **box}
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)

    # ids: the distinct ids are packed once, the rows gather their words (no 20 M Python strings on the way in)
    t = time.perf_counter()
    uw, _ = ops.prep_pack_ids(users.astype(object), "user_id")
    iw, _ = ops.prep_pack_ids(items.astype(object), "asin")
    ukeys = torch.from_numpy(uw.view(np.int64)[uidx]).to(dev)
    ikeys = torch.from_numpy(iw.view(np.int64)[iidx]).to(dev)
    ts_d = torch.from_numpy(ts).to(dev)
    val_d = torch.from_numpy(rating).to(dev)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t
    host = not args.skip_host
    ucol = users.astype(object)[uidx] if host else None
    icol = items.astype(object)[iidx] if host else None

    # ---- encode
    codes = {}
    for name, keys, col in (("encode_users", ukeys, ucol), ("encode_items", ikeys, icol)):
        dt, (c, first) = timed(lambda: ops.prep_encode(keys), args.repeats)
        codes[name] = c
        ht = eq = None
        if host:
            ht, (classes, inv) = host_once(lambda: np.unique(col, return_inverse=True))
            eq = bool(np.array_equal(c.cpu().numpy(), inv) and np.array_equal(col[first.cpu().numpy()], classes))
        record(name, dt, ht, eq, classes=int(first.numel()), upload_s=round(upload_s, 4))
    ucode, icode = codes["encode_users"], codes["encode_items"]
    n_users, n_items = int(ucode.max()) + 1, int(icode.max()) + 1

    # ---- k-core
    dt, (alive, n_alive, rounds) = timed(lambda: ops.prep_kcore(ucode, icode, n_users, n_items, 5, 5, 10), args.repeats)
    ht = eq = None
    if host:
        def host_filter():
            df = pd.DataFrame({"user_id": ucol, "asin": icol})
            for _ in range(10):
                prev = len(df)
                uc = df["user_id"].value_counts()
                df = df[df["user_id"].isin(uc[uc >= 5].index)]
                ic = df["asin"].value_counts()
                df = df[df["asin"].isin(ic[ic >= 5].index)]
                if len(df) == prev:
                    break
            return df.index.to_numpy()
        ht, kept = host_once(host_filter)
        eq = bool(np.array_equal(np.flatnonzero(alive.cpu().numpy()), kept))
    record("kcore", dt, ht, eq, alive=n_alive, rounds=rounds)

    # ---- split
    dt, (perm, train, val, test) = timed(lambda: ops.prep_split(ucode, ts_d, n_users), args.repeats)
    ht = eq = None
    if host:
        def host_split():
            df = pd.DataFrame({"user_id": ucol, "timestamp": ts, "row": np.arange(n)})
            df = df.sort_values(["user_id", "timestamp"]).reset_index(drop=True)
            df["_rank"] = df.groupby("user_id").cumcount(ascending=False) + 1
            df["_count"] = df["user_id"].map(df.groupby("user_id").size())
            te = (df["_rank"] == 1) & (df["_count"] >= 2)
            va = (df["_rank"] == 2) & (df["_count"] >= 3)
            return [df["row"][m].to_numpy() for m in (~te & ~va, va, te)]
        ht, want = host_once(host_split)
        eq = all(bool(np.array_equal(g.cpu().numpy(), w)) for g, w in zip((train, val, test), want))
    record("split", dt, ht, eq, train=int(train.numel()), val=int(val.numel()), test=int(test.numel()))

    # ---- csr
    dt, m = timed(lambda: ops.prep_csr(ucode, icode, val_d, n_users, n_items), args.repeats)
    ht = eq = None
    if host:
        uc_h, ic_h = ucode.cpu().numpy(), icode.cpu().numpy()
        ht, want = host_once(lambda: csr_matrix((rating, (uc_h, ic_h)), shape=(n_users, n_items), dtype=np.float32))
        want.sort_indices()
        eq = bool(np.array_equal(m.row_ptr.cpu().numpy(), want.indptr) and
                  np.array_equal(m.col_idx.cpu().numpy(), want.indices) and
                  np.array_equal(m.vals.cpu().numpy(), want.data))
    record("csr", dt, ht, eq, nnz=int(m.col_idx.numel()))


if __name__ == "__main__":
    main()
