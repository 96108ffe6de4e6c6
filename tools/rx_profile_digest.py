#!/usr/bin/env python3
"""Developer tool: the bytes of the thirteen receive-profile entry points and of wofdm_tx_papr, as SHA-256 digests -- for comparing two builds of the
library (WOFDM_LIB=... selects one) or two versions of the Python layer above it: run the tool once per build or tree and diff
the outputs line for line.  It uses the package's public names and the case modules of tests/, so against a tree or a library
that lacks the youngest entry point run THAT tree's own copy of this tool: the earlier entries' lines are made the same way by both
copies, and the younger copy only adds lines (profiles/rx_profile_ldpc.txt section 6 is such a comparison).

It runs the tests' own cases with the tests' own frame counts, so the shapes are the smallest that reach S < W, S no multiple
of W, W = 4 at N = 1024, the fold with and without an Rx tail and both noise orders:
  rx_profile          tests/rx_profile_cases.py: every N, a plain and a masked variant, the systems rotated
  rx_profile_aci      CASES of tests/test_gpu_rx_profile_aci.py
  rx_profile_sync     CASES and points of tests/test_gpu_rx_profile_sync.py
  rx_profile_doppler  tests/doppler_cases.py CASES, and the extra steps and knot counts of its EXTRA case
  rx_profile_pa       tests/pa_cases.py
  rx_profile_pn       CASES and POINTS of tests/test_gpu_rx_profile_pn.py
  rx_profile_link     the cases of tests/test_gpu_rx_profile_link.py, composed points and their single-impairment points
  rx_profile_soft     the same cases with the points and default scales of tests/test_gpu_rx_profile_soft.py: the link fields and
                      beside them bit_penalty and bit_penalty_sym (the ABI's sym_penalty)
  rx_profile_tracking the cases of tests/test_gpu_rx_profile_tracking.py with its comb, points, receivers and scales, and the
                      decisions per point and per symbol
  rx_profile_coded    the same cases with the one link point and the four receivers of tests/test_gpu_rx_profile_coded.py, its
                      interleaver and three codes: the tracking fields, info_err, cw_err, info_bits, codewords and the exported
                      soft bits (the chunk shape without them)
  rx_profile_coded_frame  the same cases, points, receivers, interleaver and codes, one codeword per frame (tests/
                      test_gpu_rx_profile_coded_frame.py): the tracking fields, info_err, cw_err, info_bits, codewords, sym_rot and
                      the exported soft bits (the chunk shape without them)
  rx_profile_ldpc     the same cases, points, receivers and interleaver with the three LDPC codes of tests/
                      test_gpu_rx_profile_ldpc.py: the tracking fields, info_err, cw_err, unconverged, iterations, info_bits,
                      codewords, sym_rot and the exported soft bits (the chunk shape without them)
  rx_profile_coset    the same cases, points, receivers and interleaver with the three Viterbi rates and the three LDPC codes of tests/
                      test_gpu_rx_profile_coset.py: the tracking fields, both families' counters, info bits and codewords, sym_rot
                      and the exported soft bits (the chunk shape without them)
  tx_papr             tests/papr_cases.py: every N, system and variant; hist, max_papr and periods (--route gpu only: the
                      oracle is its only mirror, and the tests hold it against that)
and for each entry point the chunk-straddling shape of its test file (N = 1024, S = 16, cp + cs = 64, four chunks and a bit;
tx_papr: one pair, a full chunk and 37 frames, periods from the 39 frames around the boundary).
The seeds are the cases' base seeds: the tests pick theirs with the oracle or the mirrors, which no digest needs.

--route gpu (the default, GPU box): the ``rx_profile_*_gpu`` functions.  --route host (any machine, no library, no GPU): the
fp64 mirrors ``rx_profile_*_host`` with with_near=True on the same small cases, the near counts hashed as a field of their
own, the pa arm's reference power from ``pa_ref_power(..., gpu=False)``; the chunk shapes are left out (chunking is a GPU
notion, and they are too large for the mirror).  The seconds per case go to stderr, the slowest case last.

One JSON line per (entry point, case): {"entry", "case", "sha256": {field: digest of the array's bytes}}.  The bytes depend on
the compiler, so a recorded output is a comparison of two runs, never a golden for the suite.

    WOFDM_LIB=/path/to/libwofdm_hip.so python tools/rx_profile_digest.py [--route gpu|host] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wofdm_amd as W  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402
from wofdm_amd import timefreq as TF  # noqa: E402

import doppler_cases as DC  # noqa: E402
import pa_cases as PC  # noqa: E402
import papr_cases as XC  # noqa: E402
import rx_profile_cases as RC  # noqa: E402
import test_gpu_rx_profile_aci as TA  # noqa: E402
import test_gpu_rx_profile_coded as TC  # noqa: E402
import test_gpu_rx_profile_coded_frame as TCF  # noqa: E402
import test_gpu_rx_profile_coset as TCS  # noqa: E402
import test_gpu_rx_profile_doppler as TD  # noqa: E402
import test_gpu_rx_profile_ldpc as TLD  # noqa: E402
import test_gpu_rx_profile_link as TL  # noqa: E402
import test_gpu_rx_profile_pa as TP  # noqa: E402
import test_gpu_rx_profile_pn as TN  # noqa: E402
import test_gpu_rx_profile_soft as TQ  # noqa: E402
import test_gpu_rx_profile_sync as TS  # noqa: E402
import test_gpu_rx_profile_tracking as TT  # noqa: E402


def host_plain(c, seed, frame_offset, frames):
    return R.rx_profile_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                             active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], with_near=True)


def host_aci(c, seed, frame_offset, frames):
    return R.rx_profile_aci_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                 c["aci_active"], c["delay"], c["level"], c["aci_h"], active=c["active"], mask=c["mask"],
                                 noise_before_truncate=c["nbt"], with_near=True)


def gpu_link(c, seed, frame_offset, frames, **kw):
    if "ref_power" in kw:                                              # (the chunk shape: its own sides, no case name)
        return W.rx_profile_link_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                     c["points"], active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], **kw)
    return TL.run_gpu(c, seed, frame_offset, frames)


def gpu_soft(c, seed, frame_offset, frames, **kw):
    if "scales" in kw:                                                 # (the chunk shape: its own points and scales)
        return W.rx_profile_soft_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                     c["points"], kw["scales"], active=c["active"])
    return TQ.run_soft(c, seed, frame_offset, frames)


def gpu_tracking(c, seed, frame_offset, frames, **kw):
    if "scales" in kw:                                                 # (the chunk shape: its own comb, points and scales)
        return W.rx_profile_tracking_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                         c["points"], c["tracking"], c["pilots"], kw["scales"], active=c["active"])
    return TT.run_gpu(c, seed, frame_offset, frames)


def gpu_coded(c, seed, frame_offset, frames, **kw):
    if "scales" in kw:                                                 # (the chunk shape: its own comb, points, scales and codes)
        return W.rx_profile_coded_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                      c["points"], c["tracking"], c["pilots"], kw["scales"], R.LLR_SCALE, c["perm"], kw["codes"],
                                      active=c["active"])
    return TC.run_gpu(c, seed, frame_offset, frames, export=True)


def host_coded(c, seed, frame_offset, frames):
    return R.rx_profile_coded_host(*TT.head(c, seed, frame_offset, frames), c["points"], c["tracking"], c["pilots"], TC.SCALES,
                                   R.LLR_SCALE, c["perm"], TC.CODES, with_near=True, **TT.sides(c, seed, frame_offset, frames))


def gpu_coded_frame(c, seed, frame_offset, frames, **kw):
    if "scales" in kw:                                                 # (the chunk shape: its own comb, points, scales and codes)
        return W.rx_profile_coded_frame_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                            c["points"], c["tracking"], c["pilots"], kw["scales"], R.LLR_SCALE, c["perm"], kw["codes"],
                                            active=c["active"])
    return TCF.run_gpu(c, seed, frame_offset, frames, export=True)


def host_coded_frame(c, seed, frame_offset, frames):
    return R.rx_profile_coded_frame_host(*TT.head(c, seed, frame_offset, frames), c["points"], c["tracking"], c["pilots"], TC.SCALES,
                                         R.LLR_SCALE, c["perm"], TC.CODES, with_near=True, **TT.sides(c, seed, frame_offset, frames))


def gpu_ldpc(c, seed, frame_offset, frames, **kw):
    if "scales" in kw:                                                 # (the chunk shape: its own comb, points, scales and codes)
        return W.rx_profile_ldpc_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                     c["points"], c["tracking"], c["pilots"], kw["scales"], R.LLR_SCALE, c["perm"], kw["codes"],
                                     active=c["active"])
    return TLD.run_gpu(c, seed, frame_offset, frames, export=True)


def host_ldpc(c, seed, frame_offset, frames):
    return R.rx_profile_ldpc_host(*TT.head(c, seed, frame_offset, frames), c["points"], c["tracking"], c["pilots"], TC.SCALES,
                                  R.LLR_SCALE, c["perm"], TLD.CODES, with_near=True, **TT.sides(c, seed, frame_offset, frames))


def gpu_coset(c, seed, frame_offset, frames, **kw):
    if "scales" in kw:                                                 # (the chunk shape: its own comb, points, scales and codes)
        return W.rx_profile_coset_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                      c["points"], c["tracking"], c["pilots"], kw["scales"], R.LLR_SCALE, c["perm"], kw["codes"],
                                      kw["ldpc_codes"], active=c["active"])
    return TCS.run_gpu(c, seed, frame_offset, frames, export=True)


def host_coset(c, seed, frame_offset, frames):
    return R.rx_profile_coset_host(*TT.head(c, seed, frame_offset, frames), c["points"], c["tracking"], c["pilots"], TC.SCALES,
                                   R.LLR_SCALE, c["perm"], TCS.RATES, TCS.CODES, with_near=True, **TT.sides(c, seed, frame_offset, frames))


def papr_digests(c, seed, frame_offset, frames, periods_at=None):
    """hist, max_papr and periods of one wofdm_tx_papr call; periods_at: (frame_offset, frames) of a second call the periods
    come from, where the first has too many to ask for"""
    kw = dict(active=c["active"], mask=c["mask"], lo_db=XC.LO_DB, step_db=XC.STEP_DB, n_bins=XC.N_BINS)
    out = TF.tx_papr_gpu(c["st"], c["k"], c["S"], c["w"], seed, frame_offset, frames, periods=periods_at is None, **kw)
    per = out[2] if periods_at is None else TF.tx_papr_gpu(c["st"], c["k"], c["S"], c["w"], seed, *periods_at, periods=True, **kw)[2]
    return {f: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
            for f, a in (("hist", out[0]), ("max_papr", out[1]), ("periods", per))}


#: entry -> (gpu route -> profile, host route -> (profile, near)), both (case, seed, frame_offset, frames, **kw)
ROUTES = {
    "rx_profile": (RC.run_gpu, host_plain),
    "rx_profile_aci": (TA.run_gpu, host_aci),
    "rx_profile_sync": (TS.run_gpu, TS.host),
    "rx_profile_doppler": (TD.run_gpu, DC.host),
    "rx_profile_pa": (TP.run_gpu, PC.host),
    "rx_profile_pn": (TN.run_gpu, TN.host),
    "rx_profile_link": (gpu_link, TL.host),
    "rx_profile_soft": (gpu_soft, lambda *a, **kw: (TQ.host_soft(*a, **kw), None)),   # (the link entry has the near counts)
    "rx_profile_tracking": (gpu_tracking, TT.host),
    "rx_profile_coded": (gpu_coded, host_coded),
    "rx_profile_coded_frame": (gpu_coded_frame, host_coded_frame),
    "rx_profile_ldpc": (gpu_ldpc, host_ldpc),
    "rx_profile_coset": (gpu_coset, host_coset),
}


def digests(prof, near=None):
    d = {f: hashlib.sha256(np.ascontiguousarray(getattr(prof, f)).tobytes()).hexdigest() for f in prof._fields
         if getattr(prof, f) is not None}                               # (None: soft bits that were not asked for)
    if near is not None:
        d["near"] = hashlib.sha256(np.ascontiguousarray(near).tobytes()).hexdigest()
    return d


def small_cases():
    """(entry, case name, case, seed, extra keywords): RC.FRAMES frames each"""
    for i, n in enumerate(RC.NS):
        for variant in ("plain", "half_masked"):
            system = RC.SYSTEMS[(i + (variant != "plain")) % len(RC.SYSTEMS)]
            cp, S, k = RC.shape_of(n, system, variant)
            c = RC.make_case(W.make_structure(system, n, cp), k, S, variant, 2000 + n + RC.SYSTEMS.index(system))
            yield "rx_profile", "n%d_%s_%s" % (n, system, variant), c, 10 * n, {}
    for j, name in enumerate(TA.CASES):
        yield "rx_profile_aci", name, TA.case(name), 100 * (1 + j), {}
    for j, name in enumerate(TS.CASES):
        yield "rx_profile_sync", name, TS.case(name), 100 * (1 + j), {}
    for j, name in enumerate(DC.CASES):
        yield "rx_profile_doppler", name, DC.case(name), 100 * (1 + j), {}
    for tracks, step in DC.extra_tracks(DC.case(DC.EXTRA)):
        yield ("rx_profile_doppler", "%s_step%d_knots%d" % (DC.EXTRA, step, tracks.shape[2]), DC.case(DC.EXTRA), 100,
               dict(tracks=tracks, knot_step=step))
    for j, name in enumerate(PC.CASES):
        yield "rx_profile_pa", name, PC.case(name), 100 * (1 + j), {}
    for j, name in enumerate(TN.CASES):
        yield "rx_profile_pn", name, TN.case(name), 100 * (1 + j), {}
    for j, name in enumerate(TL.CASES):
        c = TL.case(name)
        yield "rx_profile_link", name, dict(c, points=c["composed"] + c["singles"]), 100 * (1 + j), {}
    for j, name in enumerate(TQ.CASES):
        yield "rx_profile_soft", name, TL.case(name), 100 * (1 + j), {}
    for name in TT.CASES:
        yield "rx_profile_tracking", name, TT.case(name), TT.base_seed(name), {}
    for name in TT.CASES:
        yield "rx_profile_coded", name, TC.case(name), TC.seed_of(name), {}
    for name in TT.CASES:
        yield "rx_profile_coded_frame", name, TC.case(name), TC.seed_of(name), {}
    for name in TT.CASES:
        yield "rx_profile_ldpc", name, TC.case(name), TC.seed_of(name), {}
    for name in TT.CASES:
        yield "rx_profile_coset", name, TC.case(name), TC.seed_of(name), {}


def papr_cases():
    """(case name, case, seed): tests/papr_cases.py without its oracle, XC.FRAMES frames each"""
    for n in XC.NS:
        for system in XC.SYSTEMS:
            for variant in XC.VARIANTS:
                _, S, k = XC.shape_of(n, system, variant)
                st = XC.structure(n, system)
                c = dict(st=st, k=k, S=S, w=XC.random_windows(st, XC.PAIRS, 1000 + n + XC.SYSTEMS.index(system)),
                         active=XC.allocation(n, variant), mask=XC.mask_of(st, variant))
                yield "n%d_%s_%s" % (n, system, variant), c, 10 * (n + 7 * XC.SYSTEMS.index(system) + XC.VARIANTS.index(variant))


def chunk_cases():
    """(entry, case, frames, extra keywords): the chunk-straddling shape of the thirteen test files, N = 1024, S = 16, cp + cs = 64"""
    st, S = W.make_structure("wtx", 1024, 56), 16
    big = RC.make_case(st, 4, S, "plain", 3001)
    half = CM.half_band_allocation(1024)

    def frames_of(per_chunk):
        return per_chunk // 2 + 19

    yield "rx_profile", big, frames_of(R.rx_profile_chunk_frames(st, S, False)), {}
    ca = dict(big, active=half, aci_active=~half, delay=501, level=0.0, aci_h=None)
    yield "rx_profile_aci", ca, frames_of(R.rx_profile_aci_chunk_frames(st, S, False)), {}
    cs = dict(big, active=half, points=[R.SyncPoint(0, 0.0, 1), R.SyncPoint(-40, 0.03, 0)])
    yield "rx_profile_sync", cs, frames_of(R.rx_profile_sync_chunk_frames(st, S, False, 2)), {}
    cd = dict(big, active=half, knot_step=st.stride)
    cd["tracks"] = DC.tracks_of(cd, (0.0, 0.002), st.stride, S + 2)
    yield "rx_profile_doppler", cd, frames_of(R.rx_profile_doppler_chunk_frames(st, S, False, 2)), {}
    cq = dict(big, active=half, name="over_the_frame_limit")
    pts, ref = (R.PaPoint(R.PA_LINEAR, 0.0), R.PaPoint(R.PA_RAPP, 3.0, 2.0)), np.full(RC.PAIRS, 1.0 / 1024, np.float32)
    yield "rx_profile_pa", cq, frames_of(R.rx_profile_pa_chunk_frames(st, S, False, 2)), dict(points=pts, ref=ref)
    cn = dict(big, active=half, points=[R.PnPoint(0.0, 1), R.PnPoint(0.01, 0)])
    yield "rx_profile_pn", cn, frames_of(R.rx_profile_pn_chunk_frames(st, S, False, 2)), {}
    cl = dict(cd, points=[R.LinkPoint(), R.LinkPoint(pts[1], 1, 2, 0.02, 1, 0.01, 0, (501, 0.0))])
    yield ("rx_profile_link", cl, frames_of(R.rx_profile_link_chunk_frames(st, S, False, 2, True)),
           dict(tracks=cd["tracks"], knot_step=st.stride, aci_active=~half, ref_power=ref))
    cq = dict(big, active=half, points=[R.LinkPoint(), R.LinkPoint(linewidth=0.01)])
    yield "rx_profile_soft", cq, frames_of(R.rx_profile_soft_chunk_frames(st, S, False, 2, False, 2)), dict(scales=(0.5, 0.1))
    ct = dict(big, active=half, pilots=R.pilot_comb(half, 8), points=[R.LinkPoint(linewidth=0.01), R.LinkPoint(cfo=0.01, cfo_tracked=0)],
              tracking=[R.TrackingPoint(1, 1), R.TrackingPoint(0, 1)])
    yield "rx_profile_tracking", ct, frames_of(R.rx_profile_tracking_chunk_frames(st, S, False, 2, False, 2)), dict(scales=(0.5, 0.1))
    cc = dict(ct, perm=R.default_interleaver(4 * int((half & ~ct["pilots"]).sum())))
    yield ("rx_profile_coded", cc, frames_of(R.rx_profile_coded_chunk_frames(st, S, False, 2, False, 1)),
           dict(scales=(0.5,), codes=(0, 2)))
    yield ("rx_profile_coded_frame", cc,
           frames_of(R.rx_profile_coded_frame_chunk_frames(st, 4, S, False, 2, False, 1, int((half & ~ct["pilots"]).sum()), (0, 2), True)),
           dict(scales=(0.5,), codes=(0, 2)))
    yield ("rx_profile_ldpc", cc, frames_of(R.rx_profile_ldpc_chunk_frames(st, S, False, 2, False, 1)),
           dict(scales=(0.5,), codes=((4, 8, 6), (4, 16, 10))))
    yield ("rx_profile_coset", cc,
           frames_of(R.rx_profile_coset_chunk_frames(st, 4, S, False, 2, False, 1, int((half & ~ct["pilots"]).sum()), (0, 2), True)),
           dict(scales=(0.5,), codes=(0, 2), ldpc_codes=((4, 8, 6), (4, 16, 10))))


def runs(route):
    """(entry, case, callable that returns the digests)"""
    for entry, name, c, seed, kw in small_cases():
        if route == "host":
            yield entry, name, lambda e=entry, c=c, s=seed, kw=kw: digests(*ROUTES[e][1](c, s, 0, RC.FRAMES, **kw))
        else:
            yield entry, name, lambda e=entry, c=c, s=seed, kw=kw: digests(ROUTES[e][0](c, s, 0, RC.FRAMES, **kw))
    if route == "gpu":
        # by entry point, the chunk shape behind its small cases (seed 7000)
        for entry, c, frames, kw in chunk_cases():
            yield entry, "chunks", lambda e=entry, c=c, f=frames, kw=kw: digests(ROUTES[e][0](c, 7000, 0, f, **kw))
        for name, c, seed in papr_cases():
            yield "tx_papr", name, lambda c=c, s=seed: papr_digests(c, s, 0, XC.FRAMES)
        st = XC.structure(1024, "wtx")
        c = dict(st=st, k=4, S=16, w=XC.random_windows(st, 1, 9), active=None, mask=None)
        per_chunk = TF.tx_papr_chunk_frames(st, 16, False)
        yield "tx_papr", "chunks", lambda c=c, n=per_chunk: papr_digests(c, 40, 0, n + 37, periods_at=(n - 2, 39))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("gpu", "host"), default="gpu")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    slowest = (0.0, None)
    for entry, case, call in runs(args.route):
        t0 = time.perf_counter()
        line = json.dumps({"entry": entry, "case": case, "sha256": call()}, sort_keys=True)
        dt = time.perf_counter() - t0
        slowest = max(slowest, (dt, "%s %s" % (entry, case)))
        print(line, flush=True)
        if args.route == "host":
            print("%s %s: %.1f s" % (entry, case, dt), file=sys.stderr, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if args.route == "host":
        print("slowest case: %s, %.1f s" % (slowest[1], slowest[0]), file=sys.stderr)


if __name__ == "__main__":
    main()
