#!/usr/bin/env python
"""Build the dictionary of the default tokenizer (token_type="dictionary", tokenizer_dict_file): a k-means codebook over the
normalised (dx, dy) offsets of the QuickDraw training sketches, fitted on the GPU by sketchformer_amd.kmeans.

The flags and defaults are those of the reference's prep_data/sketch_token/create_token_dict.py; --n-samples is honoured (the
reference reads a name its parser never defines).  Only `-m k-means` is built.

    python prep_data/sketch_token/create_token_dict.py --dataset-dir /data/quickdraw --target-file prep_data/sketch_token/token_dict.pkl
    python train.py ... --data-hparams tokenizer_dict_file=prep_data/sketch_token/token_dict.pkl

A --target-file ending in .npz needs no scikit-learn, to write or to read.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def normalize_sketch(sketch):
    """Clamp every entry to +-1000 (removes large gaps), then divide the offsets by max(width, height, 1) of the bounds of the
    pen path; float32 (create_token_dict.py:44-54)."""
    from sketchformer_amd.dataloaders.distributed_stroke3 import get_bounds
    sketch = np.maximum(np.minimum(sketch, 1000), -1000)
    min_x, max_x, min_y, max_y = get_bounds(sketch)
    max_dim = max([max_x - min_x, max_y - min_y, 1])
    sketch = sketch.astype(np.float32)
    sketch[:, :2] /= max_dim
    return sketch


def split_offsets(sketch):
    """(pen-hold offsets, pen-lift successors) of one normalised sketch: the points that follow a pen lift - the jumps between
    strokes - go to the second group, except the successor of the last lift, which the reference drops from it
    (create_token_dict.py:35-40)."""
    lift = (np.where(sketch[:, 2] == 1)[0] + 1)[:-1]
    hold = np.ones(len(sketch), dtype=bool)
    hold[lift] = False
    return sketch[hold, :2], sketch[lift, :2]


def load_data(files, verbose=True):
    """All offsets of the `train` split of the class files as two (N, 2) float32 arrays: pen-hold points, pen-lift successors
    (create_token_dict.py:20-41)."""
    out0, out1 = [], []
    for i, path in enumerate(files):
        if verbose:
            print("Loading {} ({}/{})".format(path, i, len(files)))
        data = np.load(path, encoding="latin1", allow_pickle=True)
        for sketch in data["train"]:
            p0, p1 = split_offsets(normalize_sketch(sketch))
            out0.append(p0)
            out1.append(p1)
    return np.concatenate(out0), np.concatenate(out1)


def subsample(data_p0, data_p1, n_samples, p1_ratio, seed=0, verbose=True):
    """n_samples points with the p1_ratio share of pen-lift successors (a group smaller than its share is kept whole), drawn
    without replacement, seeded; the two groups concatenated (create_token_dict.py:88-99).  p1_ratio = 0 keeps everything."""
    if p1_ratio > 0:
        rng = np.random.RandomState(seed)
        n_p1 = int(p1_ratio * n_samples)
        n_p0 = n_samples - n_p1
        if len(data_p0) > n_p0:
            if verbose:
                print("Sample %d out of %d points with penstate 0" % (n_p0, len(data_p0)))
            data_p0 = data_p0[rng.choice(len(data_p0), n_p0, replace=False)]
        if len(data_p1) > n_p1:
            if verbose:
                print("Sample %d out of %d points with penstate 1" % (n_p1, len(data_p1)))
            data_p1 = data_p1[rng.choice(len(data_p1), n_p1, replace=False)]
    return np.r_[data_p0, data_p1]


def build_parser():
    parser = argparse.ArgumentParser(description="Build the k-means dictionary of sketch tokens")
    parser.add_argument("--dataset-dir")
    parser.add_argument("-s", "--vocab-size", default=1000, type=int)
    parser.add_argument("--n-samples", default=5000000, type=int)
    parser.add_argument("-m", "--method", default="k-means")
    parser.add_argument("-r", "--p1-ratio", default=0.2, type=float,
                        help="Ratio of points with penstate=1 (minority) vs penstate=0 (majority) in SAMPLES; set to 0 if disable")
    parser.add_argument("--class-list", type=str, default="prep_data/quickdraw/list_quickdraw.txt")
    parser.add_argument("--target-file", type=str, default="prep_data/sketch_token/token_dict.pkl")
    parser.add_argument("--n-init", default=10, type=int)
    parser.add_argument("--max-iter", default=500, type=int)
    parser.add_argument("--tol", default=1e-6, type=float)
    parser.add_argument("--seed", default=0, type=int)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)

    if args.method != "k-means":
        print("Unsupported clustering method: %s" % args.method)
        sys.exit(1)

    with open(args.class_list) as clf:
        class_names = clf.read().splitlines()
    class_files = ["{}/{}.npz".format(args.dataset_dir, name) for name in class_names if name]

    t0 = time.time()
    print("Loading data ...")
    data_p0, data_p1 = load_data(class_files)
    print("p1/p0 natural ratio: %f" % (len(data_p1) / max(len(data_p0), 1)))
    data = subsample(data_p0, data_p1, args.n_samples, args.p1_ratio, seed=args.seed)
    t1 = time.time()
    print("Loading data done, took %.1f s: %d points" % (t1 - t0, len(data)))

    print("Building dictionary ...")
    from sketchformer_amd import kmeans
    result = kmeans.fit(data, args.vocab_size, n_init=args.n_init, max_iter=args.max_iter, tol=args.tol, seed=args.seed,
                        return_labels=False)
    t2 = time.time()
    print("Dictionary built: %.1f s; inertia %.9g, %d iterations, %d empty centres" %
          (t2 - t1, result.inertia_, result.n_iter_, result.n_empty_))
    print("Iterations per run: %s" % " ".join(str(r["n_iter"]) for r in result.runs_))
    print("Inertia per run: %s" % " ".join("%.9g" % r["inertia"] for r in result.runs_))
    kmeans.save_dictionary(args.target_file, result)
    print("Wrote %s.  Total time: %.1f s" % (args.target_file, time.time() - t0))


if __name__ == "__main__":
    main()
