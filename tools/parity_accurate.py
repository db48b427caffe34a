"""The accurate network's parity figures as one JSON object (kept as profiles/parity_accurate.json): for every case of
tests/test_accurate_gpu.py and both volume layouts, the decision stage's maximum score error against the float64
restatement (tests/accurate_reference.py) - split-operand kernel, plain-f16 kernel, float32 library route - beside the
two yardsticks computed on the same inputs (E32, E16) and the ratios the tests bound (src/tolerances.py).

    python tools/parity_accurate.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", os.path.join("mc-cnn-python_amd", "src")):
    sys.path.insert(0, os.path.join(ROOT, p))

import _hipabi as hip
import tolerances as tol
import test_accurate_gpu as t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    hip.require_device()
    cases = {}
    for name in t.CASES:
        c = t._case(name)
        rec = dict(E32=c["e32"], E16=c["e16"], voxels=int(c["mask"].sum()))
        for layout in t.LAYOUTS:
            split = t._score_error(name, t._volumes(name, layout, "kernel", hip.MCCNN_CV_EXACT)[0])
            f16 = t._score_error(name, t._volumes(name, layout, "kernel", hip.MCCNN_CV_MFMA)[0])
            lib = t._score_error(name, t._volumes(name, layout, "library", hip.MCCNN_CV_EXACT)[0])
            rec[layout] = dict(split_max_err=split, split_over_E32=split / c["e32"], library_max_err=lib,
                               library_over_E32=lib / c["e32"], f16_max_err=f16,
                               f16_over_bound=f16 / (tol.ACCURATE_F16_E16_FACTOR * c["e16"] +
                                                     tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]))
        cases[name] = rec
    result = dict(bounds=dict(split="%d x E32" % tol.ACCURATE_SPLIT_E32_FACTOR,
                              f16="%d x E16 + %d x E32" % (tol.ACCURATE_F16_E16_FACTOR, tol.ACCURATE_SPLIT_E32_FACTOR)),
                  cases=cases)
    print(json.dumps(result, sort_keys=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
