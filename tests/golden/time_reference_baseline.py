"""Time the reference's own evaluate_model loop (src/ml/baseline.py:411-471) on the All_Beauty-shaped planted set
(gen.PLANTED_CONFIG), on the CPU, for the figures beside scripts/bench_baselines.py in DESIGN.md.

Run in the build container (where the reference checkout exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/time_reference_baseline.py [rows] [model ...]
rows: how many test rows to time (default 2000; 0 = all 22,363); models: Popularity and / or Item-KNN.
Prints one JSON line per model and protocol.
"""
from __future__ import annotations

import importlib
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from gen import write_planted_artifacts  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    import pandas as pd
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    names = sys.argv[2:] or ["Item-KNN"]
    import_reference()
    b = importlib.import_module("src.ml.baseline")
    with tempfile.TemporaryDirectory() as td:
        data, _ = write_planted_artifacts(td)
        full, train_df, val_df, maps = b.load_training_data(str(data))
        u2i, i2i = maps["user_to_idx"], maps["item_to_idx"]
        matrix, _ = b._build_input_matrix(train_df, val_df, u2i, i2i, full.shape)
        test_df = pd.read_csv(Path(data) / "test.csv")
    if rows:
        test_df = test_df.head(rows)
    classes = {"Popularity": b.PopularityRecommender, "Item-KNN": b.ItemKNNRecommender}
    for name in names:
        model = classes[name]()
        t0 = time.perf_counter()
        model.fit(matrix)
        fit_s = time.perf_counter() - t0
        for n_neg in (99, None):
            np.random.seed(0)
            t0 = time.perf_counter()
            b.evaluate_model(model, name, matrix, test_df, u2i, i2i, [5, 10, 20], n_neg)
            dt = time.perf_counter() - t0
            print(json.dumps({"model": name, "protocol": "neg99" if n_neg else "full", "users": len(test_df),
                              "shape": list(matrix.shape), "fit_s": round(fit_s, 3), "s": round(dt, 2),
                              "users_per_s": round(len(test_df) / dt, 1)}), flush=True)


if __name__ == "__main__":
    main()
