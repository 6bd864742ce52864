"""Reader of the golden .npz fixtures that are stored in parts.  No committed file may exceed 1 MiB, so tests/golden/make_golden.py
writes a larger fixture NAME as NAME.npz plus NAME.part2.npz, NAME.part3.npz, ... (disjoint keys); load() merges them into one dict."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name: str) -> dict:
    out = {}
    for f in [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".part*.npz"))):
        with np.load(f) as z:
            for k in z.files:
                assert k not in out, (f, k)
                out[k] = z[k]
    return out
