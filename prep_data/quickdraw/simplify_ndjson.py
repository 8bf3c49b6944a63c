#!/usr/bin/env python
"""Raw QuickDraw drawings -> the per-class .npz files that prep_data/prepare-distributed-quickdraw.py reads.

Every line of <ndjson-dir>/<class>.ndjson is one JSON record whose "drawing" is a list of strokes [[x...], [y...], [t...]].  Per
drawing, in this order: align to the top-left corner; scale uniformly, in float64, so that the larger extent is 255 (an extent of
0 leaves the drawing alone); cast to float32; with --resample-spacing S > 0, resample every stroke along its arc length at a
spacing of S; Ramer-Douglas-Peucker at --epsilon; round the kept positions (np.rint); take differences -> int16 stroke-3, one row
per kept point, the first counted from (0, 0).  The resampling and the simplification run on the GPU, a whole class per call, the
resampled points never leaving it (sketchformer_amd.simplify.simplify_lines).  Records with "recognized": false are skipped unless
--keep-unrecognized is given.

With --resample-spacing 1.0 these are the steps of Google's published recipe for the simplified QuickDraw files, in its order:
align, scale, resample at a spacing of one pixel, simplify at epsilon 2.0, round.  Google publishes the steps, not their
arithmetic (how a length is measured, where the last sample falls, how ties are broken), so the files follow the published
recipe's steps and are not promised to be byte-equal to the published files.  The resampling rule used here is written out in
include/skf.h.  The default, --resample-spacing 0, leaves the step out and writes the files this script has always written.

The first --n-train usable drawings of a class go to `train`, the next --n-valid to `valid`, the next --n-test to `test`.
--class-list names a text file of class names, one per line; the repository ships none, so it must be supplied.

    python prep_data/quickdraw/simplify_ndjson.py --ndjson-dir /data/raw --class-list classes.txt --target-dir /data/quickdraw
    python prep_data/prepare-distributed-quickdraw.py --dataset-dir /data/quickdraw --class-list classes.txt --target-dir /data/chunks
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def read_drawings(path, limit, keep_unrecognized=False):
    """Up to `limit` usable drawings of one .ndjson file, each a list of float64 (n, 2) polylines."""
    from sketchformer_amd.simplify import quickdraw_lines
    out = []
    with open(path) as f:
        for line in f:
            if len(out) >= limit:
                break
            line = line.strip()
            if not line:
                continue
            record = json.loads(line)
            if not keep_unrecognized and record.get("recognized") is False:
                continue
            lines = quickdraw_lines(record["drawing"])
            if lines:
                out.append(lines)
    return out


def simplify_drawings(drawings, epsilon, resample_spacing=0.0):
    """A list of drawings -> an object array of int16 stroke-3 sketches; one device call for all of them (with a
    resample_spacing > 0: one per run of strokes whose resampled points fit simplify.RESAMPLE_ROW_BUDGET)."""
    from sketchformer_amd.simplify import drawing_to_stroke3, scale_to_255, simplify_lines
    scaled = [scale_to_255(d) for d in drawings]
    every = [l for d in scaled for l in d]
    kept = simplify_lines(every, epsilon, resample_spacing=resample_spacing) if resample_spacing > 0 else simplify_lines(every, epsilon)
    out, at = np.empty(len(drawings), dtype=object), 0
    for i, d in enumerate(scaled):
        out[i] = drawing_to_stroke3(kept[at:at + len(d)])
        at += len(d)
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description="Simplify raw QuickDraw .ndjson files into per-class stroke-3 .npz files")
    parser.add_argument('--ndjson-dir', required=True)
    parser.add_argument('--class-list', required=True, help="text file of class names, one per line (must be supplied)")
    parser.add_argument('--target-dir', required=True)
    parser.add_argument('--epsilon', type=float, default=2.0)
    parser.add_argument('--resample-spacing', type=float, default=0.0,
                        help="resample every stroke at this spacing before the simplification; 1.0 is the published recipe, 0 = off")
    parser.add_argument('--n-train', type=int, default=70000)
    parser.add_argument('--n-valid', type=int, default=2500)
    parser.add_argument('--n-test', type=int, default=2500)
    parser.add_argument('--keep-unrecognized', action='store_true')
    args = parser.parse_args(argv)
    if not 0.0 <= args.resample_spacing < float("inf"):
        parser.error("--resample-spacing must be finite and not negative (0 = off)")

    with open(args.class_list) as f:
        class_names = [c for c in f.read().splitlines() if c]
    os.makedirs(args.target_dir, exist_ok=True)
    total = args.n_train + args.n_valid + args.n_test
    for i, name in enumerate(class_names):
        drawings = read_drawings(os.path.join(args.ndjson_dir, name + ".ndjson"), total, args.keep_unrecognized)
        print("Class {} ({}/{}): {} drawings".format(name, i + 1, len(class_names), len(drawings)))
        sketches = simplify_drawings(drawings, args.epsilon, args.resample_spacing)
        a, b = args.n_train, args.n_train + args.n_valid
        np.savez(os.path.join(args.target_dir, name + ".npz"), train=sketches[:a], valid=sketches[a:b], test=sketches[b:])


if __name__ == '__main__':
    main()
