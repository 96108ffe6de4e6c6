#!/usr/bin/env python3
"""Developer tool (GPU box): the bytes of the five receive-profile entry points, as SHA-256 digests -- for comparing two
builds of the library (WOFDM_LIB=... selects one; run the tool once per build and diff the outputs line for line).

It runs the tests' own cases with the tests' own frame counts, so the shapes are the smallest that reach S < W, S no multiple
of W, W = 4 at N = 1024, the fold with and without an Rx tail and both noise orders:
  rx_profile          tests/rx_profile_cases.py: every N, a plain and a masked variant, the systems rotated
  rx_profile_aci      CASES of tests/test_gpu_rx_profile_aci.py
  rx_profile_sync     CASES and points of tests/test_gpu_rx_profile_sync.py
  rx_profile_doppler  tests/doppler_cases.py CASES, and the extra steps and knot counts of its EXTRA case
  rx_profile_pa       tests/pa_cases.py
and for each entry point the chunk-straddling shape of its test file (N = 1024, S = 16, cp + cs = 64, four chunks and a bit).
The seeds are the cases' base seeds: the tests pick theirs with the oracle or the mirrors, which no digest needs.

One JSON line per (entry point, case): {"entry", "case", "sha256": {field: digest of the array's bytes}}.  The bytes depend on
the compiler, so a recorded output is a comparison of two builds, never a golden for the suite.

    WOFDM_LIB=/path/to/libwofdm_hip.so python tools/rx_profile_digest.py [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wofdm_amd as W  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402

import doppler_cases as DC  # noqa: E402
import pa_cases as PC  # noqa: E402
import rx_profile_cases as RC  # noqa: E402
import test_gpu_rx_profile_aci as TA  # noqa: E402
import test_gpu_rx_profile_doppler as TD  # noqa: E402
import test_gpu_rx_profile_pa as TP  # noqa: E402
import test_gpu_rx_profile_sync as TS  # noqa: E402


def digests(prof):
    return {f: hashlib.sha256(np.ascontiguousarray(getattr(prof, f)).tobytes()).hexdigest() for f in prof._fields}


def runs():
    """(entry, case, callable that returns the profile)"""
    for i, n in enumerate(RC.NS):
        for variant in ("plain", "half_masked"):
            system = RC.SYSTEMS[(i + (variant != "plain")) % len(RC.SYSTEMS)]
            cp, S, k = RC.shape_of(n, system, variant)
            c = RC.make_case(W.make_structure(system, n, cp), k, S, variant, 2000 + n + RC.SYSTEMS.index(system))
            yield "rx_profile", "n%d_%s_%s" % (n, system, variant), lambda c=c, n=n: RC.run_gpu(c, 10 * n, 0, RC.FRAMES)
    for j, name in enumerate(TA.CASES):
        yield "rx_profile_aci", name, lambda name=name, j=j: TA.run_gpu(TA.case(name), 100 * (1 + j), 0, RC.FRAMES)
    for j, name in enumerate(TS.CASES):
        yield "rx_profile_sync", name, lambda name=name, j=j: TS.run_gpu(TS.case(name), 100 * (1 + j), 0, RC.FRAMES)
    for j, name in enumerate(DC.CASES):
        yield "rx_profile_doppler", name, lambda name=name, j=j: TD.run_gpu(DC.case(name), 100 * (1 + j), 0, RC.FRAMES)
    for i, (tracks, step) in enumerate(DC.extra_tracks(DC.case(DC.EXTRA))):
        yield ("rx_profile_doppler", "%s_step%d_knots%d" % (DC.EXTRA, step, tracks.shape[2]),
               lambda tracks=tracks, step=step: TD.run_gpu(DC.case(DC.EXTRA), 100, 0, RC.FRAMES, tracks=tracks, knot_step=step))
    for j, name in enumerate(PC.CASES):
        yield "rx_profile_pa", name, lambda name=name, j=j: TP.run_gpu(PC.case(name), 100 * (1 + j), 0, RC.FRAMES)
    # the chunk-straddling shape of the five test files: N = 1024, S = 16, cp + cs = 64, seed 7000
    st, S = W.make_structure("wtx", 1024, 56), 16
    big = RC.make_case(st, 4, S, "plain", 3001)
    half = CM.half_band_allocation(1024)

    def frames_of(per_chunk):
        return per_chunk // 2 + 19

    yield "rx_profile", "chunks", lambda: RC.run_gpu(big, 7000, 0, frames_of(R.rx_profile_chunk_frames(st, S, False)))
    ca = dict(big, active=half, aci_active=~half, delay=501, level=0.0, aci_h=None)
    yield "rx_profile_aci", "chunks", lambda: TA.run_gpu(ca, 7000, 0, frames_of(R.rx_profile_aci_chunk_frames(st, S, False)))
    cs = dict(big, active=half, points=[R.SyncPoint(0, 0.0, 1), R.SyncPoint(-40, 0.03, 0)])
    yield "rx_profile_sync", "chunks", lambda: TS.run_gpu(cs, 7000, 0, frames_of(R.rx_profile_sync_chunk_frames(st, S, False, 2)))
    cd = dict(big, active=half, knot_step=st.stride)
    cd["tracks"] = DC.tracks_of(cd, (0.0, 0.002), st.stride, S + 2)
    yield "rx_profile_doppler", "chunks", lambda: TD.run_gpu(cd, 7000, 0, frames_of(R.rx_profile_doppler_chunk_frames(st, S, False, 2)))
    cq = dict(big, active=half, name="over_the_frame_limit")
    pts, ref = (R.PaPoint(R.PA_LINEAR, 0.0), R.PaPoint(R.PA_RAPP, 3.0, 2.0)), np.full(RC.PAIRS, 1.0 / 1024, np.float32)
    yield "rx_profile_pa", "chunks", lambda: TP.run_gpu(cq, 7000, 0, frames_of(R.rx_profile_pa_chunk_frames(st, S, False, 2)),
                                                        points=pts, ref=ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for entry, case, call in runs():
        line = json.dumps({"entry": entry, "case": case, "sha256": digests(call())}, sort_keys=True)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
