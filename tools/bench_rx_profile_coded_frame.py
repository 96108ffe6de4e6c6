#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_coded_frame beside wofdm_rx_profile_coded with the same point, in ONE run -- the
shape of tools/bench_rx_profile_coded.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.
Pair 0 is the raised-cosine pair, pair 1 a pair with linear edges.

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms).  The calls of a run are made in rounds
-- every variant once per round, --rounds rounds after a warm-up round --, so that a drift of the clocks meets every variant alike;
per variant the median, the smallest and the largest of its rounds are reported:
  - the link point has a free-running carrier offset of 0.02 and a linewidth of 1e-3, the receiver is (1, 1) behind a comb on every
    eighth loaded bin, one scale; the interleaver within a symbol is the default one, the rotation default_sym_rot over S - 1 symbols;
  - wofdm_rx_profile_coded (one codeword per data symbol) with one code (rate 1/2) and with three (1/2, 2/3, 3/4);
    wofdm_rx_profile_coded_frame (one codeword per frame over its S - 2 data symbols) with the same; neither exports soft bits.
From the medians: what a further code costs in either call, (three - one) / 2 -- the per-symbol decoder's figure is the yardstick of
the frame decoder's, in the same run --, and what the frame call with one code costs over the per-symbol call with one.  The frame
call's nine tracking fields are compared with the per-symbol call's by bytes on the way.  The run also reports, per pair and rate,
the coded BER and the codeword error rate of both calls over the cells.  One JSON line per run.  A diagnostic route, not the hot
path; the boxes switch clock states, so only figures of one run compare.

    python tools/bench_rx_profile_coded_frame.py [--frames 2000] [--rounds 5]
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
    n_data = int((alloc & ~pil).sum())
    n_c = k * n_data
    perm = R.default_interleaver(n_c)
    point, tp, sc = R.LinkPoint(cfo=0.02, cfo_tracked=0, linewidth=1e-3, cpe_tracked=0), (1, 1), R.SOFT_SCALES[:1]
    s_d = S - 2                                                            # (the receiver has a postamble)
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
        head = ([point], [tp], pil, sc, R.LLR_SCALE, perm)
        variants = {
            "symbol_1_code": lambda f: R.rx_profile_coded_gpu(*base, f, *head, (0,), **kw),
            "symbol_3_codes": lambda f: R.rx_profile_coded_gpu(*base, f, *head, (0, 1, 2), **kw),
            "frame_1_code": lambda f: R.rx_profile_coded_frame_gpu(*base, f, *head, (0,), None, **kw),
            "frame_3_codes": lambda f: R.rx_profile_coded_frame_gpu(*base, f, *head, (0, 1, 2), None, **kw),
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
        per_sym = (med["symbol_3_codes"] - med["symbol_1_code"]) / 2.0
        per_frm = (med["frame_3_codes"] - med["frame_1_code"]) / 2.0
        res["per_code_ms"] = {"symbol": round(per_sym, 2), "frame": round(per_frm, 2), "frame_over_symbol": round(per_frm / per_sym, 4)}
        res["frame_1_code_minus_symbol_1_code_ms"] = round(med["frame_1_code"] - med["symbol_1_code"], 2)
        for v in ("frame_1_code", "frame_3_codes"):
            for a, b in zip(last[v][:9], last["symbol_3_codes"][:9]):
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), v
        frm, sym = last["frame_3_codes"], last["symbol_3_codes"]
        assert np.array_equal(frm.info_err[..., :1], last["frame_1_code"].info_err)
        uncoded = (sym.bit_err[0].sum(axis=-1) / (k * float(sym.decisions[0].sum()))).mean(axis=(1, 2))
        res["uncoded_ber"] = dict(zip(names, np.round(uncoded, 5).tolist()))

        def table(a):                                                      # [pairs, n_snr, n_ch, codes] -> per pair and rate
            a = a.mean(axis=(1, 2))
            return {nm: dict(zip(R.CODE_RATES, np.round(a[i], 5).tolist())) for i, nm in enumerate(names)}
        res["symbol_coded_ber"], res["symbol_cwer"] = table(R.coded_ber(sym)[1][0]), table(R.coded_cwer(sym)[1][0])
        res["frame_coded_ber"], res["frame_fer"] = table(R.coded_frame_ber(frm)[0]), table(R.coded_fer(frm)[0])
        # (the harsh end, where the per-symbol figures of profiles/rx_profile_coded.txt come from: the SNR points as they are)
        res["frame_coded_ber_by_snr_rc"] = {str(float(s)): np.round(R.coded_frame_ber(frm)[0][0, i].mean(axis=0), 5).tolist()
                                            for i, s in enumerate(snr)}
        res["symbol_coded_ber_by_snr_rc"] = {str(float(s)): np.round(R.coded_ber(sym)[1][0][0, i].mean(axis=0), 5).tolist()
                                             for i, s in enumerate(snr)}
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_coded_frame N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, one "
                    "point (cfo 0.02 and linewidth 1e-3, both free-running) behind the (1, 1) receiver, %d pilot bins of %d loaded, n_c "
                    "= %d per symbol (T = %s), n_f = %d per frame over %d data symbols (T = %s), sym_rot %d, llr_scale %g, %d rounds"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S, int(pil.sum()), int(alloc.sum()), n_c,
                       " / ".join(str(R.code_steps(r, n_c)) for r in (0, 1, 2)), n_c * s_d, s_d,
                       " / ".join(str(R.code_steps(r, n_c * s_d)) for r in (0, 1, 2)), frm.sym_rot, R.LLR_SCALE, args.rounds),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": {"symbol": R.rx_profile_coded_chunk_frames(st, S, m is not None, 1, False, 1),
                             "frame_1_code": R.rx_profile_coded_frame_chunk_frames(st, k, S, m is not None, 1, False, 1, n_data, (0,), True),
                             "frame_3_codes": R.rx_profile_coded_frame_chunk_frames(st, k, S, m is not None, 1, False, 1, n_data,
                                                                                    (0, 1, 2), True)}}, **res)), flush=True)


if __name__ == "__main__":
    main()
