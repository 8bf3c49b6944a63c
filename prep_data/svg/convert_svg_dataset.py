#!/usr/bin/env python
"""SVG sketch corpora (TU-Berlin, Sketchy: <svg-dir>/<class>/*.svg) -> the per-class .npz files that
prep_data/prepare-distributed-quickdraw.py and prep_data/sketch_token/create_token_dict.py read: `train` / `valid` / `test` object
arrays of int16 stroke-3 sketches, exactly what prep_data/quickdraw/simplify_ndjson.py writes.

Per drawing, in this order: parse the file (paths, basic shapes, group transforms; erased - white - strokes are dropped); move the
control points into the working frame (larger side 1024) so that --tol means the same for every file; flatten the curves on the
GPU at --tol, a whole class per call (sketchformer_amd.svg.flatten_paths; the rule is written out in include/skf.h); then the
QuickDraw steps: align and scale to 255, with --resample-spacing S > 0 resample every stroke at that spacing, Ramer-Douglas-Peucker
at --epsilon, round, take differences.

The files of a class are taken in sorted name order; of the n usable ones the last int(n * test-fraction) go to `test`, the
int(n * valid-fraction) before them to `valid`, the rest to `train`.  A file that does not parse is reported with its path and
skipped; the number of skipped files is printed at the end.  --class-list names a text file of class names, one per line.

    python prep_data/svg/convert_svg_dataset.py --svg-dir /data/tu-berlin/svg --class-list classes.txt --target-dir /data/tub
    python prep_data/prepare-distributed-quickdraw.py --dataset-dir /data/tub --class-list classes.txt --target-dir /data/chunks
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def read_class(folder):
    """-> (the drawings of the folder's .svg files in sorted name order, in their working frames; the paths that were skipped).
    A drawing without ink counts as skipped."""
    from sketchformer_amd.svg import parse_svg, working_frame
    drawings, skipped = [], []
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(".svg")) if os.path.isdir(folder) else []
    for name in names:
        path = os.path.join(folder, name)
        try:
            drawing = working_frame(parse_svg(path))
        except (ValueError, OSError) as e:
            print("skipped {}: {}".format(path, e))
            skipped.append(path)
            continue
        if not drawing:
            print("skipped {}: no ink".format(path))
            skipped.append(path)
            continue
        drawings.append(drawing)
    return drawings, skipped


def convert_drawings(drawings, epsilon, tol, resample_spacing=0.0):
    """Drawings in their working frames -> an object array of int16 stroke-3 sketches: one flatten call for all of them, then the
    steps of simplify_ndjson.simplify_drawings."""
    from sketchformer_amd.simplify import drawing_to_stroke3, scale_to_255, simplify_lines
    from sketchformer_amd.svg import flatten_paths
    scaled = [scale_to_255(lines) for lines in flatten_paths(drawings, tol)]
    every = [l for d in scaled for l in d]
    kept = simplify_lines(every, epsilon, resample_spacing=resample_spacing) if resample_spacing > 0 else simplify_lines(every, epsilon)
    out, at = np.empty(len(drawings), dtype=object), 0
    for i, d in enumerate(scaled):
        out[i] = drawing_to_stroke3(kept[at:at + len(d)])
        at += len(d)
    return out


def split_bounds(n, valid_fraction, test_fraction):
    """-> (a, b): train = [0, a), valid = [a, b), test = [b, n)"""
    n_test, n_valid = int(n * test_fraction), int(n * valid_fraction)
    return n - n_test - n_valid, n - n_test


def main(argv=None):
    parser = argparse.ArgumentParser(description="Convert folders of SVG sketches into per-class stroke-3 .npz files")
    parser.add_argument('--svg-dir', required=True, help="holds one folder of .svg files per class")
    parser.add_argument('--class-list', required=True, help="text file of class names, one per line (must be supplied)")
    parser.add_argument('--target-dir', required=True)
    parser.add_argument('--epsilon', type=float, default=2.0)
    parser.add_argument('--tol', type=float, default=0.0625, help="flattening tolerance in the working frame (larger side 1024)")
    parser.add_argument('--valid-fraction', type=float, default=0.1)
    parser.add_argument('--test-fraction', type=float, default=0.1)
    parser.add_argument('--resample-spacing', type=float, default=0.0,
                        help="resample every stroke at this spacing (in 0 .. 255 units) before the simplification; 0 = off")
    args = parser.parse_args(argv)
    if not 0.0 <= args.resample_spacing < float("inf"):
        parser.error("--resample-spacing must be finite and not negative (0 = off)")
    if not 0.0 < args.tol < float("inf"):
        parser.error("--tol must be finite and above 0")
    if not (args.valid_fraction >= 0 and args.test_fraction >= 0 and args.valid_fraction + args.test_fraction <= 1):
        parser.error("--valid-fraction and --test-fraction must not be negative and must not add up to more than 1")

    with open(args.class_list) as f:
        class_names = [c for c in f.read().splitlines() if c]
    os.makedirs(args.target_dir, exist_ok=True)
    n_skipped = 0
    for i, name in enumerate(class_names):
        drawings, skipped = read_class(os.path.join(args.svg_dir, name))
        n_skipped += len(skipped)
        print("Class {} ({}/{}): {} drawings".format(name, i + 1, len(class_names), len(drawings)))
        sketches = convert_drawings(drawings, args.epsilon, args.tol, args.resample_spacing)
        a, b = split_bounds(len(sketches), args.valid_fraction, args.test_fraction)
        np.savez(os.path.join(args.target_dir, name + ".npz"), train=sketches[:a], valid=sketches[a:b], test=sketches[b:])
    print("{} files skipped".format(n_skipped))
    return n_skipped


if __name__ == '__main__':
    main()
