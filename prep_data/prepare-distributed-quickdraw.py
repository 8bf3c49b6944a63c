#!/usr/bin/env python
"""Per-class QuickDraw files -> the chunk files the `stroke3-distributed` and `stroke3-distributed-device` loaders open:
train_000.npz .. (x, y, label_names, std, mean), valid.npz and test.npz (x, y, label_names) and meta.npz.

The command line and the files are those of the reference's prep_data/prepare-distributed-quickdraw.py, its habits included:
  - a class gives len(train) // n_chunks sketches to every chunk, in file order; --cut-chunks C writes only the first
    n_chunks - C chunks and takes the first int((n_chunks - C) / n_chunks * len) sketches of every valid and test split;
  - std and mean of a chunk are taken over all dx and dy jointly, in the sketches' own dtype; meta.npz holds their sums over the
    written chunks divided by --n-chunks, also when --cut-chunks wrote fewer;
  - the class files are named for the whole list before --n-classes cuts it.
The statistics are taken over one concatenated array instead of a Python list of points: the same array, the same bits.

--class-list has no default here: the file of class names, one per line, is the caller's (the repository ships none).

One option is new.  --simplify-epsilon E (default 0 = off): every train, valid and test sketch is simplified stroke by stroke
on the GPU first (sketchformer_amd.simplify.simplify_sketches, Ramer-Douglas-Peucker at E in the units of the offsets), and the
statistics are those of the simplified sketches.  A coarser epsilon shortens long sketches without cutting their tail off, which
is what max_seq_len does to them in the loader.

    python prep_data/prepare-distributed-quickdraw.py --dataset-dir /data/quickdraw --class-list classes.txt --target-dir /data/chunks
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPLITS = ("train", "valid", "test")
PICKLED = {"allow_pickle": True, "encoding": "latin1"}           # the class files hold object arrays, some pickled by Python 2


def parse(argv):
    ap = argparse.ArgumentParser(description="Cut per-class stroke-3 files into the chunk files the distributed loaders open")
    ap.add_argument("--dataset-dir", help="where <class>.npz (train / valid / test object arrays) lie")
    ap.add_argument("--class-list", required=True, help="text file of class names, one per line (must be supplied)")
    ap.add_argument("--n-chunks", type=int, default=10, help="every class is cut into this many train chunks")
    ap.add_argument("--n-classes", type=int, default=10, help="take the first so many names of the list")
    ap.add_argument("--cut-chunks", type=int, default=0, help="leave the last so many chunks unwritten")
    ap.add_argument("--target-dir", help="where the chunk files go")
    ap.add_argument("--simplify-epsilon", type=float, default=0.0, help="> 0: simplify every sketch on the GPU at this epsilon")
    return ap.parse_args(argv)


def load_classes(dataset_dir, list_path, n_classes):
    """-> (names, [{split: object array}]) of the first n_classes names of the list."""
    with open(list_path) as f:
        names = f.read().splitlines()
    paths = [os.path.join(dataset_dir, name + ".npz") for name in names]         # (named before the list is cut)
    names, paths = names[:n_classes], paths[:n_classes]
    loaded = []
    for path in paths:
        with np.load(path, **PICKLED) as npz:
            loaded.append({split: npz[split] for split in SPLITS})
    return names, loaded


def gather(loaded, split, bounds):
    """Rows bounds(len) = (first, last) of `split` of every class, class after class -> (sketches, labels)."""
    xs, ys = [], []
    for label, arrays in enumerate(loaded):
        first, last = bounds(len(arrays[split]))
        xs.append(arrays[split][first:last])
        ys.append(np.full(last - first, label, dtype=int))
    return np.concatenate(xs), np.concatenate(ys)


def offsets_std_mean(sketches):
    """np.std and np.mean over the (dx, dy) of every point of the sketches, as one (P, 2) array of the sketches' dtype."""
    points = np.concatenate([np.asarray(s)[:, :2] for s in sketches]) if len(sketches) else np.array([])
    return np.std(points), np.mean(points)


def main(argv=None):
    args = parse(argv)
    names, loaded = load_classes(args.dataset_dir, args.class_list, args.n_classes)
    if args.simplify_epsilon > 0:
        from sketchformer_amd.simplify import simplify_sketches
        prepared = lambda sketches: simplify_sketches(sketches, args.simplify_epsilon)
    else:
        prepared = lambda sketches: sketches
    os.makedirs(args.target_dir, exist_ok=True)
    out = lambda name: os.path.join(args.target_dir, name)

    whole = args.n_chunks
    written = whole - args.cut_chunks
    counts = dict.fromkeys(SPLITS, 0)
    chunk_stds, chunk_means = [], []
    for c in range(written):
        x, y = gather(loaded, "train", lambda n: ((n // whole) * c, (n // whole) * (c + 1)))
        x = prepared(x)
        std, mean = offsets_std_mean(x)
        chunk_stds.append(std)
        chunk_means.append(mean)
        np.savez(out("train_%03d.npz" % c), x=x, y=y, label_names=names, std=std, mean=mean)
        counts["train"] += len(x)
        print("train chunk %d of %d: %d sketches of %d classes" % (c + 1, whole, len(x), len(names)))
    if written > 0:
        for split in ("valid", "test"):
            x, y = gather(loaded, split, lambda n: (0, int((written / whole) * n)))
            x = prepared(x)
            np.savez(out(split + ".npz"), x=x, y=y, label_names=names)
            counts[split] = len(x)

    # (the sums run over the chunks written and are divided by the number asked for: the reference's files say the same)
    meta = {"std": sum(chunk_stds) / whole, "mean": sum(chunk_means) / whole, "class_names": names, "n_classes": len(names),
            "n_samples_train": counts["train"], "n_samples_test": counts["test"], "n_samples_valid": counts["valid"]}
    np.savez(out("meta.npz"), **meta)


if __name__ == '__main__':
    main()
