#!/usr/bin/env python
"""Records tests/golden/prepare_quickdraw/: three tiny synthetic class files (int16, a dozen sketches in `train`, fewer in
`valid` and `test`) and what the reference's prep_data/prepare-distributed-quickdraw.py writes for them with
`--n-chunks 2 --n-classes 3`, once as it is (cut0/) and once with `--cut-chunks 1` (cut1/).  The reference script is run by path
in a child process; only data is written - the inputs and the .npz files it produced.

    python tools/record_prepare_quickdraw_golden.py --reference /path/to/reference/checkout

tests/test_simplify_cpu.py holds prep_data/prepare-distributed-quickdraw.py of this repository against these files.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prepare_quickdraw")
CLASSES = ("anvil", "bee", "cactus", "unused")          # the list names one class more than --n-classes takes
SPLITS = (("train", 13), ("valid", 5), ("test", 4))     # 13 // 2 = 6 a chunk: the last train sketch of a class is left over


def synthetic_class(seed):
    rng = np.random.RandomState(seed)
    out = {}
    for split, count in SPLITS:
        arr = np.empty(count, dtype=object)
        for i in range(count):
            n = int(rng.randint(3, 30))
            s = np.zeros((n, 3), np.int16)
            s[:, :2] = rng.randint(-25, 26, size=(n, 2))
            s[rng.randint(0, n, size=2), 2] = 1
            s[-1, 2] = 1
            arr[i] = s
        out[split] = arr
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reference", required=True, help="the reference checkout")
    args = parser.parse_args()
    script = os.path.join(args.reference, "prep_data", "prepare-distributed-quickdraw.py")
    inputs = os.path.join(GOLDEN, "input")
    os.makedirs(inputs, exist_ok=True)
    for i, name in enumerate(CLASSES[:3]):
        np.savez(os.path.join(inputs, name + ".npz"), **synthetic_class(100 + i))
    with open(os.path.join(inputs, "classes.txt"), "w") as f:
        f.write("\n".join(CLASSES) + "\n")
    for tag, cut in (("cut0", 0), ("cut1", 1)):
        with tempfile.TemporaryDirectory() as tmp:
            target = os.path.join(tmp, "chunks")
            subprocess.run([sys.executable, script, "--dataset-dir", inputs, "--class-list", os.path.join(inputs, "classes.txt"),
                            "--n-chunks", "2", "--n-classes", "3", "--cut-chunks", str(cut), "--target-dir", target],
                           check=True, stdout=subprocess.DEVNULL)
            out = os.path.join(GOLDEN, tag)
            os.makedirs(out, exist_ok=True)
            for name in sorted(os.listdir(target)):
                with np.load(os.path.join(target, name), allow_pickle=True) as npz:      # rewritten compressed: data only
                    np.savez_compressed(os.path.join(out, name), **{k: npz[k] for k in npz.files})
                print(tag, name)


if __name__ == "__main__":
    main()
