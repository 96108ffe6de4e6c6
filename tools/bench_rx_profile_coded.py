#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_coded beside wofdm_rx_profile_tracking with the same point, in ONE run -- the
shape of tools/bench_rx_profile_tracking.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.
Pair 0 is the raised-cosine pair, pair 1 a pair with linear edges.

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms).  The calls of a run are made in rounds
-- every variant once per round, --rounds rounds after a warm-up round --, so that a drift of the clocks meets every variant alike;
per variant the median, the smallest and the largest of its rounds are reported, and the tracking call's own spread is what a
difference has to exceed to mean anything:
  - the link point has a free-running carrier offset of 0.02 and a linewidth of 1e-3, the receiver is (1, 1) behind a comb on every
    eighth loaded bin, one scale;
  - wofdm_rx_profile_tracking; wofdm_rx_profile_coded with one code (rate 1/2) and with three (1/2, 2/3, 3/4) behind the default
    interleaver at the default llr_scale, without the soft bits' export.
From the three medians: what a further code costs, (three - one) / 2 -- the decoder, one wave per codeword --, and what is left
of (one - tracking) beyond one such decode -- the soft-bit stores and the chunk's larger scratch.  The coded call's nine tracking
fields are compared with the tracking call's by bytes on the way.  The run also reports the uncoded and the coded BER over the
cells, per pair and rate.  One JSON line per run.  A diagnostic route, not the hot path; the boxes switch clock states, so only
figures of one run compare.

    python tools/bench_rx_profile_coded.py [--frames 2000] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wofdm_amd as W  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    n, k, S, n_ch = 256, 4, 16, 4
    st = W.make_structure("CPW", n, 32)
    h = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"][:n_ch].astype(np.complex64)
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    lin_tx = W.expand_tx_window(st, np.concatenate(([1.0], np.linspace(1.0, 0.0, st.tail_tx + 2)[1:-1])))
    lin_rx = W.expand_rx_window(st, np.concatenate(([1.0], np.linspace(0.5, 0.0, st.tail_rx // 2 + 2)[1:-1])))
    names = ("rc", "linear")
    w_tx = np.stack([W.tx_rc_window(st), lin_tx]).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st), lin_rx]).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    pil = R.pilot_comb(alloc, 8)
    n_c = k * int((alloc & ~pil).sum())
    perm = R.default_interleaver(n_c)
    point, tp, sc = R.LinkPoint(cfo=0.02, cfo_tracked=0, linewidth=1e-3, cpe_tracked=0), (1, 1), R.SOFT_SCALES[:1]
    cells = w_tx.shape[0] * snr.size * n_ch
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    base = (st, k, S, w_tx, w_rx, h, snr, 1, 0)
    for name, m in (("plain", None), ("masked", mask)):
        kw = dict(active=alloc, mask=m)
        variants = {
            "tracking": lambda f: R.rx_profile_tracking_gpu(*base, f, [point], [tp], pil, sc, **kw),
            "coded_1_code": lambda f: R.rx_profile_coded_gpu(*base, f, [point], [tp], pil, sc, R.LLR_SCALE, perm, (0,), **kw),
            "coded_3_codes": lambda f: R.rx_profile_coded_gpu(*base, f, [point], [tp], pil, sc, R.LLR_SCALE, perm, (0, 1, 2), **kw),
        }
        ms, last = {v: [] for v in variants}, {}
        for call in variants.values():
            call(8)                                                        # warm-up
        for rnd in range(args.rounds + 1):
            for v, call in variants.items():
                last[v] = call(args.frames)
                if rnd > 0:
                    ms[v].append(R.rx_profile_kernel_ms())
        res = {}
        med = {v: float(np.median(ms[v])) for v in variants}
        for v in variants:
            a = np.asarray(ms[v])
            res[v + "_kernels_ms"] = {"median": round(med[v], 2), "min": round(float(a.min()), 2), "max": round(float(a.max()), 2)}
            if v != "tracking":
                res[v + "_over_tracking"] = round(med[v] / med["tracking"], 4)
        per_code = (med["coded_3_codes"] - med["coded_1_code"]) / 2.0
        res["per_code_ms"] = round(per_code, 2)
        res["per_code_over_tracking"] = round(per_code / med["tracking"], 4)
        res["stores_and_scratch_ms"] = round(med["coded_1_code"] - med["tracking"] - per_code, 2)
        for v in ("coded_1_code", "coded_3_codes"):
            for a, b in zip(last[v][:9], last["tracking"][:9]):
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), v
        prof = last["coded_3_codes"]
        assert np.array_equal(prof.info_err[..., :1, :], last["coded_1_code"].info_err)
        uncoded = (prof.bit_err[0].sum(axis=-1) / (k * float(prof.decisions[0].sum()))).mean(axis=(1, 2))
        ber = R.coded_ber(prof)[1][0].mean(axis=(1, 2))                    # [pairs, codes]
        res["uncoded_ber"] = dict(zip(names, np.round(uncoded, 5).tolist()))
        res["coded_ber"] = {nm: dict(zip(R.CODE_RATES, np.round(ber[i], 5).tolist())) for i, nm in enumerate(names)}
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_coded N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, one "
                    "point (cfo 0.02 and linewidth 1e-3, both free-running) behind the (1, 1) receiver, %d pilot bins of %d loaded, n_c "
                    "= %d (T = %s), llr_scale %g, %d rounds"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S, int(pil.sum()), int(alloc.sum()), n_c,
                       " / ".join(str(R.code_steps(r, n_c)) for r in (0, 1, 2)), R.LLR_SCALE, args.rounds),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": {"tracking": R.rx_profile_tracking_chunk_frames(st, S, m is not None, 1, False, 1),
                             "coded": R.rx_profile_coded_chunk_frames(st, S, m is not None, 1, False, 1)}}, **res)), flush=True)


if __name__ == "__main__":
    main()
