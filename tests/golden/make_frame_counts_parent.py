#!/usr/bin/env python3
"""Records tests/golden/frame_counts_parent.npz: the counters of the cases of tests/frame_counts_cases.py as the library built from the
commit BEFORE the frame kernels' packed fp32 arithmetic was written per component computes them, on an MI355X.

    python tests/golden/make_frame_counts_parent.py [out.npz]      # in a tree of that commit, built, plus tests/frame_counts_cases.py

The values are what tests/test_gpu_counts_pinned.py holds every later build to, bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import frame_counts_cases as FC  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "frame_counts_parent.npz")
    channels = np.load(os.path.join(HERE, "channels_vehA.npz"), allow_pickle=False)["h"]
    arrays = {}
    for name in FC.CASES:
        for off, got in zip(FC.OFFSETS, FC.run_case(name, channels)):
            arrays["%s/%d" % (name, off)] = got
            print("%-22s offset %-11d bit errors %s of %s" % (name, off, got[..., 0].ravel(), got[..., 1].ravel()))
    np.savez_compressed(out, **arrays)
    print("wrote %s: %d arrays" % (out, len(arrays)))


if __name__ == "__main__":
    main()
