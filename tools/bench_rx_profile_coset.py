#!/usr/bin/env python3
"""Developer tool (GPU box): wofdm_rx_profile_coset beside wofdm_rx_profile_coded_frame and wofdm_rx_profile_ldpc with the same
point and codes, in ONE run -- the shape of tools/bench_rx_profile_ldpc.py: the half-band system of main_channel_mask.m at N = 256,
16-QAM, 16 symbols per frame (CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with
the reference's Tx mask.  Pair 0 is the raised-cosine pair, pair 1 a pair with linear edges.  The link point has a free-running
carrier offset of 0.02 and a linewidth of 1e-3 (the harsh point), the receiver is (1, 1) behind a comb on every eighth loaded bin;
Viterbi 1/2, 2/3, 3/4; LDPC (4, 8), (4, 12), (4, 16) at --max-iter iterations.

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms).  The calls of a run are made in rounds
-- every variant once per round, --rounds rounds after a warm-up round --, so that a drift of the clocks meets every variant alike;
per variant the median, the smallest and the largest of its rounds are reported:
  - the all-zero calls with one code and with three, as tools/bench_rx_profile_ldpc.py runs them;
  - the coset call with the Viterbi codes alone (one, three), the LDPC codes alone (one, three) and all six.
From the medians: the coset call with all six codes against the SUM of the two all-zero calls with three each (it runs the receive
chain once where they run it twice: it must cost less); what a further code costs in the coset view against the all-zero view,
(three - one) / 2 per family.  By bytes on the way: the coset call's nine tracking fields are the frame call's, and its counters do
not depend on which family runs beside.  The run also reports, by SNR for the raised-cosine pair and over the cells per pair, the
coded BER, the word error rate and the share of unconverged words in the coset view beside the all-zero view's, from the same
frames.  One JSON line per run.  A diagnostic route, not the hot path; the boxes switch clock states, so only figures of one run
compare.

    python tools/bench_rx_profile_coset.py [--frames 2000] [--rounds 5] [--max-iter 20]
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
    ap.add_argument("--variants", choices=("plain", "masked", "both"), default="both")
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
    n_f = n_c * (S - 2)                                                    # (the receiver has a postamble)
    rates = (0, 1, 2)
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
        if args.variants not in (name, "both"):
            continue
        kw = dict(active=alloc, mask=m)
        head = ([point], [tp], pil, sc, R.LLR_SCALE, perm)
        variants = {
            "zero_viterbi_1": lambda f: R.rx_profile_coded_frame_gpu(*base, f, *head, rates[:1], None, **kw),
            "zero_viterbi_3": lambda f: R.rx_profile_coded_frame_gpu(*base, f, *head, rates, None, **kw),
            "zero_ldpc_1": lambda f: R.rx_profile_ldpc_gpu(*base, f, *head, ldpc[:1], None, **kw),
            "zero_ldpc_3": lambda f: R.rx_profile_ldpc_gpu(*base, f, *head, ldpc, None, **kw),
            "coset_viterbi_1": lambda f: R.rx_profile_coset_gpu(*base, f, *head, rates[:1], (), None, **kw),
            "coset_viterbi_3": lambda f: R.rx_profile_coset_gpu(*base, f, *head, rates, (), None, **kw),
            "coset_ldpc_1": lambda f: R.rx_profile_coset_gpu(*base, f, *head, (), ldpc[:1], None, **kw),
            "coset_ldpc_3": lambda f: R.rx_profile_coset_gpu(*base, f, *head, (), ldpc, None, **kw),
            "coset_all_6": lambda f: R.rx_profile_coset_gpu(*base, f, *head, rates, ldpc, None, **kw),
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
        both = med["zero_viterbi_3"] + med["zero_ldpc_3"]
        res["coset_all_6_over_the_two_all_zero_calls"] = {"coset_ms": round(med["coset_all_6"], 2), "sum_ms": round(both, 2),
                                                          "ratio": round(med["coset_all_6"] / both, 4)}
        per = {f + "_" + fam: (med["%s_%s_3" % (f, fam)] - med["%s_%s_1" % (f, fam)]) / 2.0 for f in ("zero", "coset")
               for fam in ("viterbi", "ldpc")}
        res["per_code_ms"] = dict({v: round(x, 2) for v, x in per.items()},
                                  coset_over_zero_viterbi=round(per["coset_viterbi"] / per["zero_viterbi"], 4),
                                  coset_over_zero_ldpc=round(per["coset_ldpc"] / per["zero_ldpc"], 4))
        co, vit, ld = last["coset_all_6"], last["zero_viterbi_3"], last["zero_ldpc_3"]
        for v in variants:
            for a, b in zip(last[v][:9], vit[:9]):
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), v
        for f in ("info_err", "cw_err"):
            assert np.array_equal(getattr(co, f), getattr(last["coset_viterbi_3"], f)), f
            assert np.array_equal(getattr(co, f)[..., :1], getattr(last["coset_viterbi_1"], f)), f
        for f in ("ldpc_info_err", "ldpc_cw_err", "unconverged", "iterations"):
            assert np.array_equal(getattr(co, f), getattr(last["coset_ldpc_3"], f)), f
            assert np.array_equal(getattr(co, f)[..., :1], getattr(last["coset_ldpc_1"], f)), f
        uncoded = (vit.bit_err[0].sum(axis=-1) / (k * float(vit.decisions[0].sum()))).mean(axis=(1, 2))
        res["uncoded_ber"] = dict(zip(names, np.round(uncoded, 5).tolist()))

        def table(a, keys):                                                # [pairs, n_snr, n_ch, codes] -> per pair and code
            a = a.mean(axis=(1, 2))
            return {nm: dict(zip(keys, np.round(a[i], 5).tolist())) for i, nm in enumerate(names)}

        def by_snr(a):                                                     # the raised-cosine pair, per SNR point
            return {str(float(s)): np.round(a[0, i].mean(axis=0), 5).tolist() for i, s in enumerate(snr)}
        cber, cfer = R.coset_ber(co), R.coset_fer(co)
        zero = {"viterbi_ber": R.coded_frame_ber(vit)[0], "viterbi_fer": R.coded_fer(vit)[0], "ldpc_ber": R.ldpc_ber(ld)[0],
                "ldpc_fer": R.ldpc_fer(ld)[0], "ldpc_unconverged": ld.unconverged[0] / float(ld.codewords[0]),
                "ldpc_mean_iterations": R.ldpc_mean_iterations(ld)[0]}
        coset = {"viterbi_ber": cber[0][0], "viterbi_fer": cfer[0][0], "ldpc_ber": cber[1][0], "ldpc_fer": cfer[1][0],
                 "ldpc_unconverged": co.unconverged[0] / float(co.ldpc_codewords[0]),
                 "ldpc_mean_iterations": co.iterations[0] / float(co.ldpc_codewords[0])}
        for f in zero:
            keys = R.CODE_RATES if f.startswith("viterbi") else labels
            res[f] = {"coset": table(coset[f], keys), "all_zero": table(zero[f], keys)}
            res[f + "_by_snr_rc"] = {"coset": by_snr(coset[f]), "all_zero": by_snr(zero[f])}
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_coset N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, one "
                    "point (cfo 0.02 and linewidth 1e-3, both free-running) behind the (1, 1) receiver, %d pilot bins of %d loaded, n_f "
                    "= %d per frame, W = %d word(s) of n = %d; Viterbi T = %s; LDPC %s with Z = %s, K = %s, max_iter %d; sym_rot %d, "
                    "llr_scale %g, %d rounds"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S, int(pil.sum()), int(alloc.sum()), n_f,
                       *R.ldpc_frame_words(n_f), " / ".join(str(R.code_steps(r, n_f)) for r in rates), " / ".join(labels),
                       " / ".join(str(R.ldpc_lift(J, L, R.ldpc_frame_words(n_f)[1])) for J, L, _ in ldpc),
                       " / ".join(str(int(x)) for x in co.ldpc_info_bits[0]), args.max_iter, co.sym_rot, R.LLR_SCALE, args.rounds),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": {"coset_all_6": R.rx_profile_coset_chunk_frames(st, k, S, m is not None, 1, False, 1, n_data, rates, True),
                             "coset_ldpc": R.rx_profile_coset_chunk_frames(st, k, S, m is not None, 1, False, 1, n_data, (), True)}},
            **res)), flush=True)


if __name__ == "__main__":
    main()
