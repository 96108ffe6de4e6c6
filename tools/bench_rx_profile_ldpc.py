#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_ldpc beside wofdm_rx_profile_coded_frame with the same point, in ONE run -- the
shape of tools/bench_rx_profile_coded_frame.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.
Pair 0 is the raised-cosine pair, pair 1 a pair with linear edges.

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms).  The calls of a run are made in rounds
-- every variant once per round, --rounds rounds after a warm-up round --, so that a drift of the clocks meets every variant alike;
per variant the median, the smallest and the largest of its rounds are reported:
  - the link point has a free-running carrier offset of 0.02 and a linewidth of 1e-3, the receiver is (1, 1) behind a comb on every
    eighth loaded bin, one scale; the interleaver within a symbol is the default one, the rotation default_sym_rot over S - 1 symbols;
  - wofdm_rx_profile_coded_frame (the streaming Viterbi decoder, one codeword per frame) with one code (rate 1/2) and with three
    (1/2, 2/3, 3/4); wofdm_rx_profile_ldpc with (4, 8) alone and with (4, 8), (4, 12), (4, 16) -- rates 1/2, 2/3, 3/4 --, --max-iter
    iterations at most; neither exports soft bits.
From the medians: what a further code costs in either call, (three - one) / 2 -- the streaming Viterbi decoder's figure is the
yardstick of the LDPC decoder's, in the same run.  The LDPC call's nine tracking fields are compared with the frame call's by bytes
on the way.  The run also reports, per pair and code, the coded BER, the codeword error rate, the share of unconverged words and
the mean iterations of the LDPC call beside the frame call's BER and FER, over the cells and by SNR for the raised-cosine pair.  One
JSON line per run.  A diagnostic route, not the hot path; the boxes switch clock states, so only figures of one run compare.

    python tools/bench_rx_profile_ldpc.py [--frames 2000] [--rounds 5] [--max-iter 20]
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
    ap.add_argument("--max-iter", type=int, default=20)
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
    n_f = n_c * s_d
    ldpc = tuple((4, L, args.max_iter) for L in (8, 12, 16))
    labels = ["(%d, %d)" % c[:2] for c in ldpc]
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
            "viterbi_1_code": lambda f: R.rx_profile_coded_frame_gpu(*base, f, *head, (0,), None, **kw),
            "viterbi_3_codes": lambda f: R.rx_profile_coded_frame_gpu(*base, f, *head, (0, 1, 2), None, **kw),
            "ldpc_1_code": lambda f: R.rx_profile_ldpc_gpu(*base, f, *head, ldpc[:1], None, **kw),
            "ldpc_3_codes": lambda f: R.rx_profile_ldpc_gpu(*base, f, *head, ldpc, None, **kw),
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
        per_vit = (med["viterbi_3_codes"] - med["viterbi_1_code"]) / 2.0
        per_ldpc = (med["ldpc_3_codes"] - med["ldpc_1_code"]) / 2.0
        res["per_code_ms"] = {"viterbi": round(per_vit, 2), "ldpc": round(per_ldpc, 2), "ldpc_over_viterbi": round(per_ldpc / per_vit, 4)}
        res["ldpc_1_code_minus_viterbi_1_code_ms"] = round(med["ldpc_1_code"] - med["viterbi_1_code"], 2)
        for v in ("ldpc_1_code", "ldpc_3_codes"):
            for a, b in zip(last[v][:9], last["viterbi_3_codes"][:9]):
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), v
        ld, vit = last["ldpc_3_codes"], last["viterbi_3_codes"]
        for f in ("info_err", "cw_err", "unconverged", "iterations"):
            assert np.array_equal(getattr(ld, f)[..., :1], getattr(last["ldpc_1_code"], f)), f
        uncoded = (vit.bit_err[0].sum(axis=-1) / (k * float(vit.decisions[0].sum()))).mean(axis=(1, 2))
        res["uncoded_ber"] = dict(zip(names, np.round(uncoded, 5).tolist()))

        def table(a, keys):                                                # [pairs, n_snr, n_ch, codes] -> per pair and code
            a = a.mean(axis=(1, 2))
            return {nm: dict(zip(keys, np.round(a[i], 5).tolist())) for i, nm in enumerate(names)}

        def by_snr(a):                                                     # the raised-cosine pair, per SNR point
            return {str(float(s)): np.round(a[0, i].mean(axis=0), 5).tolist() for i, s in enumerate(snr)}
        unconv = ld.unconverged[0] / float(ld.codewords[0])
        res["viterbi_coded_ber"], res["viterbi_fer"] = table(R.coded_frame_ber(vit)[0], R.CODE_RATES), table(R.coded_fer(vit)[0], R.CODE_RATES)
        res["ldpc_coded_ber"], res["ldpc_fer"] = table(R.ldpc_ber(ld)[0], labels), table(R.ldpc_fer(ld)[0], labels)
        res["ldpc_unconverged"], res["ldpc_mean_iterations"] = table(unconv, labels), table(R.ldpc_mean_iterations(ld)[0], labels)
        res["ldpc_coded_ber_by_snr_rc"], res["viterbi_coded_ber_by_snr_rc"] = by_snr(R.ldpc_ber(ld)[0]), by_snr(R.coded_frame_ber(vit)[0])
        res["ldpc_mean_iterations_by_snr_rc"] = by_snr(R.ldpc_mean_iterations(ld)[0])
        res["ldpc_coded_ber_by_snr_linear"] = {str(float(s)): np.round(R.ldpc_ber(ld)[0][1, i].mean(axis=0), 5).tolist()
                                               for i, s in enumerate(snr)}
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_ldpc N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, one "
                    "point (cfo 0.02 and linewidth 1e-3, both free-running) behind the (1, 1) receiver, %d pilot bins of %d loaded, n_f "
                    "= %d per frame over %d data symbols, W = %d word(s) of n = %d; LDPC %s with Z = %s, K = %s, max_iter %d; Viterbi T = "
                    "%s; sym_rot %d, llr_scale %g, %d rounds"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S, int(pil.sum()), int(alloc.sum()), n_f, s_d,
                       *R.ldpc_frame_words(n_f), " / ".join(labels),
                       " / ".join(str(R.ldpc_lift(J, L, R.ldpc_frame_words(n_f)[1])) for J, L, _ in ldpc),
                       " / ".join(str(int(x)) for x in ld.info_bits[0]), args.max_iter,
                       " / ".join(str(R.code_steps(r, n_f)) for r in (0, 1, 2)), ld.sym_rot, R.LLR_SCALE, args.rounds),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": {"ldpc": R.rx_profile_ldpc_chunk_frames(st, S, m is not None, 1, False, 1),
                             "viterbi_3_codes": R.rx_profile_coded_frame_chunk_frames(st, k, S, m is not None, 1, False, 1, n_data,
                                                                                      (0, 1, 2), True)}}, **res)), flush=True)


if __name__ == "__main__":
    main()
