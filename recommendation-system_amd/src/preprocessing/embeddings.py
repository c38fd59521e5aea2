"""Item text embeddings: generation on the device and the file format the hot path consumes.

Mirrors src/preprocessing/embeddings.py of the reference: ItemEmbeddingGenerator / compute_item_embeddings / main
(:27-131, :161-219) encode item text with a Sentence-BERT model, and load_embeddings / the save format (:93-158) are
``<name>.npy`` (float32 [N, d], L2-normalised rows, items sorted by asin) plus ``<name>_mappings.pkl``
({item_to_idx, idx_to_item, embedding_dim, model_name, n_items}) and ``<name>_metadata.txt``.

The reference hands the model name to SentenceTransformer, which fetches it. Here nothing is fetched: model_name is a
model directory, or the name of one under config.SBERT_MODEL_DIR, and the encoder is src/preprocessing/sbert.py on
the K22 kernels (BERT and MPNet bodies, such as all-MiniLM-L6-v2 and all-mpnet-base-v2; anything else is refused by
name).
"""
from __future__ import annotations

import argparse
import logging
import pickle
from pathlib import Path

import numpy as np

from ..config import config

logger = logging.getLogger(__name__)

MAX_CHARS = 2048  # ~512 tokens


def resolve_model_dir(model_name) -> Path:
    """model_name as a directory, else <config.SBERT_MODEL_DIR>/<its last path component>."""
    tried = [Path(model_name), Path(config.SBERT_MODEL_DIR) / Path(str(model_name)).name]
    for p in tried:
        if p.is_dir():
            return p
    raise FileNotFoundError(
        f"SBERT model {str(model_name)!r} not found; tried {', '.join(str(p) for p in tried)}. Nothing is fetched: "
        "place the model's directory (config.json, model.safetensors or pytorch_model.bin, vocab.txt) there, or "
        "set SBERT_MODEL_DIR.")


def _is_missing(text) -> bool:
    """pandas.isna for a scalar: None, a float NaN, pandas.NA / NaT."""
    if text is None:
        return True
    if isinstance(text, (float, np.floating)):
        return bool(text != text)
    return type(text).__name__ in ("NAType", "NaTType")


class ItemEmbeddingGenerator:
    """The reference's ItemEmbeddingGenerator (embeddings.py:27-131) with the encoder on the HIP device: the same
    constructor and methods, a local model directory in place of a fetched one."""

    def __init__(self, model_name: str = "all-MiniLM-L6-v2", device: str | None = None):
        self.model_name = model_name
        self.device = device or "cuda"
        if str(self.device).split(":")[0] != "cuda":
            raise RuntimeError(f"ItemEmbeddingGenerator: device {device!r} is not served; the encoder runs HIP "
                               "kernels on the MI355X (torch device 'cuda') and there is no CPU fallback")
        model_dir = resolve_model_dir(model_name)
        from .sbert import SbertEncoder, load_model_dir
        logger.info("Loading SBERT model: %s from %s on %s", model_name, model_dir, self.device)
        self.model = SbertEncoder(load_model_dir(model_dir), self.device)
        self.embedding_dim = self.model.model.hidden_size
        logger.info("Embedding dimension: %d", self.embedding_dim)

    def _preprocess_text(self, texts: list[str]) -> list[str]:
        """What the encoder is given for each text: runs of whitespace become one space, the result is cut at
        MAX_CHARS characters, "..." marks a text that was longer than that before the clean-up, and a missing or
        empty text becomes the placeholder "[NO TEXT]"."""
        def one(text) -> str:
            if _is_missing(text) or text == "":
                return "[NO TEXT]"
            raw = str(text)
            return " ".join(raw.split())[:MAX_CHARS] + ("..." if len(raw) > MAX_CHARS else "")
        return [one(t) for t in texts]

    def encode_texts(self, texts: list[str], batch_size: int = 32, show_progress: bool = True) -> np.ndarray:
        """float32 [len(texts), embedding_dim], rows L2-normalised, in input order; batch_size texts are packed per
        pass over the device. show_progress is accepted for the signature and ignored."""
        rows = self.model.encode(self._preprocess_text(texts), batch_size=batch_size)
        logger.info("Encoded %d texts in passes of %d -> %s", len(texts), batch_size, rows.shape)
        return rows

    def create_item_embeddings(self, df, text_column: str = "item_text", item_id_column: str = "asin",
                               batch_size: int = 32):
        """(embeddings, item_to_idx, idx_to_item) over the frame's distinct items: row i belongs to the i-th item id
        in sorted order, and an item that occurs more than once is encoded from its first row's text."""
        first = df.drop_duplicates(subset=[item_id_column], keep="first").sort_values(item_id_column)
        items = first[item_id_column].tolist()
        logger.info("%d rows hold %d distinct items", len(df), len(items))
        embeddings = self.encode_texts(first[text_column].tolist(), batch_size)
        if embeddings.shape != (len(items), self.embedding_dim):
            raise RuntimeError(f"the encoder returned {embeddings.shape} for {len(items)} items of width "
                               f"{self.embedding_dim}")
        return embeddings, {item: i for i, item in enumerate(items)}, dict(enumerate(items))

    def save_embeddings(self, embeddings: np.ndarray, item_to_idx: dict, idx_to_item: dict, output_path) -> None:
        """The three files load_embeddings and the trainer read: <name>.npy, <name>_mappings.pkl, <name>_metadata.txt."""
        _write_embedding_files(Path(output_path), embeddings, item_to_idx, idx_to_item, self.model_name,
                               self.embedding_dim, str(self.device))
        logger.info("Wrote %s with its mappings and metadata", output_path)


def _write_embedding_files(out: Path, embeddings, item_to_idx, idx_to_item, model_name, dim, device) -> None:
    out.parent.mkdir(parents=True, exist_ok=True)
    np.save(out, embeddings)
    record = {"item_to_idx": item_to_idx, "idx_to_item": idx_to_item, "embedding_dim": int(dim),
              "model_name": model_name, "n_items": len(item_to_idx)}
    with open(out.with_name(out.stem + "_mappings.pkl"), "wb") as f:
        pickle.dump(record, f)
    lines = {"Model": model_name, "Dimension": int(dim), "Items": len(item_to_idx), "Shape": embeddings.shape,
             "Device": device}
    out.with_name(out.stem + "_metadata.txt").write_text("".join(f"{k}: {v}\n" for k, v in lines.items()))


def load_embeddings(embeddings_path, mappings_path=None):
    """(embeddings, item_to_idx | None, idx_to_item | None), as embeddings.py:134-158."""
    embeddings_path = Path(embeddings_path)
    embeddings = np.load(embeddings_path)
    item_to_idx, idx_to_item = None, None
    if mappings_path is None:
        mappings_path = embeddings_path.with_name(f"{embeddings_path.stem}_mappings.pkl")
    if Path(mappings_path).exists():
        with open(mappings_path, "rb") as f:
            mappings = pickle.load(f)  # the project's own artifact (written by save_embeddings)
        item_to_idx = mappings.get("item_to_idx")
        idx_to_item = mappings.get("idx_to_item")
    logger.info("Loaded embeddings %s", embeddings.shape)
    return embeddings, item_to_idx, idx_to_item


def save_embeddings(embeddings: np.ndarray, item_to_idx: dict, idx_to_item: dict, output_path,
                    model_name: str = "all-MiniLM-L6-v2") -> None:
    """Write the three files of ItemEmbeddingGenerator.save_embeddings (embeddings.py:93-131)."""
    out = Path(output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    np.save(out, embeddings)
    with open(out.with_name(f"{out.stem}_mappings.pkl"), "wb") as f:
        pickle.dump({"item_to_idx": item_to_idx, "idx_to_item": idx_to_item,
                     "embedding_dim": int(embeddings.shape[1]), "model_name": model_name,
                     "n_items": len(item_to_idx)}, f)
    out.with_name(f"{out.stem}_metadata.txt").write_text(
        f"Model: {model_name}\nDimension: {embeddings.shape[1]}\nItems: {len(item_to_idx)}\n"
        f"Shape: {embeddings.shape}\nDevice: n/a\n")


def compute_item_embeddings(input_path, output_path, model_name: str = "all-MiniLM-L6-v2",
                            text_column: str = "item_text", item_id_column: str = "asin", batch_size: int = 32,
                            device: str | None = None) -> None:
    """Read a .csv or .jsonl table of (item id, text) rows, encode each distinct item's text on the device and write
    the three embedding files at output_path. The table and its columns are checked before the model is loaded."""
    import pandas as pd
    readers = {".csv": pd.read_csv, ".jsonl": lambda p: pd.read_json(p, lines=True)}
    suffix = Path(str(input_path)).suffix
    if suffix not in readers:
        raise ValueError("Input must be CSV or JSONL")
    df = readers[suffix](str(input_path))
    for column in (text_column, item_id_column):
        if column not in df.columns:
            raise ValueError(f"Column '{column}' not found")
    logger.info("Read %d rows from %s", len(df), input_path)
    generator = ItemEmbeddingGenerator(model_name, device)
    generator.save_embeddings(*generator.create_item_embeddings(df, text_column, item_id_column, batch_size),
                              output_path)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Compute SBERT item embeddings")
    parser.add_argument("--input", default=config.PROCESSED_DATA_FILE)
    parser.add_argument("--output", default=config.EMBEDDINGS_FILE)
    parser.add_argument("--model", default="all-MiniLM-L6-v2")
    parser.add_argument("--text-column", default="item_text")
    parser.add_argument("--item-column", default="asin")
    parser.add_argument("--batch-size", type=int, default=32)
    parser.add_argument("--device", choices=["cuda", "cpu"], default=None)
    return parser


def main(argv=None) -> None:
    """CLI entry point (embeddings.py:195-215)."""
    logging.basicConfig(level=logging.INFO, format="%(levelname)s:%(name)s:%(message)s")
    args = build_parser().parse_args(argv)
    compute_item_embeddings(input_path=args.input, output_path=args.output, model_name=args.model,
                            text_column=args.text_column, item_id_column=args.item_column,
                            batch_size=args.batch_size, device=args.device)


if __name__ == "__main__":
    main()
