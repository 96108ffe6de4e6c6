#!/usr/bin/env python3
"""Developer tool (GPU box): wofdm_rx_profile_harq beside wofdm_rx_profile_coset with the same point and LDPC codes, in ONE run --
the shape of tools/bench_rx_profile_coset.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.  Pair
0 is the raised-cosine pair, pair 1 a pair with linear edges.  The link point has a free-running carrier offset of 0.02 and a
linewidth of 1e-3 (the harsh point), the receiver is (1, 1) behind a comb on every eighth loaded bin; LDPC (4, 8), (4, 12),
(4, 16) at --max-iter iterations; --harq-rounds transmissions at most, Chase combining and plain ARQ.

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms).  The calls of a run are made in rounds
-- every variant once per round, --rounds rounds after a warm-up round --, so that a drift of the clocks meets every variant alike;
per variant the median, the smallest and the largest of its rounds are reported: the coset call with the three LDPC codes, and
the HARQ call with them, combined and not.  Both run the receive chain on every frame; the coset call decodes every frame's
words once, the HARQ call a group's words once per round it uses.  So the comparison is the decoders' share per decode: (call -
the tracking call's time) / decodes, the tracking call being the same chain without a decoder, the decodes the coset call's
words and the HARQ call's transmissions used.  By bytes on the way: the HARQ call's nine tracking fields are the coset call's.
Per pair and code, over the cells and by SNR for the raised-cosine pair: the ACKed share by round, the mean transmissions, the
residual and the undetected word error rates, the goodput per coded bit and per on-air sample.  One JSON line per run.  A
diagnostic route, not the hot path; the boxes switch clock states, so only figures of one run compare.

    python tools/bench_rx_profile_harq.py [--frames 2000] [--rounds 5] [--max-iter 20] [--harq-rounds 4]
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
    ap.add_argument("--harq-rounds", type=int, default=4)
    ap.add_argument("--variants", choices=("plain", "masked", "both"), default="both")
    args = ap.parse_args()
    n, k, S, n_ch, HR = 256, 4, 16, 4, args.harq_rounds
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
    n_f = n_c * (S - 2)                                                    # (the receiver has a postamble)
    ldpc = tuple((4, L, args.max_iter) for L in (8, 12, 16))
    labels = ["(%d, %d)" % c[:2] for c in ldpc]
    cells = w_tx.shape[0] * snr.size * n_ch
    frames = args.frames // HR * HR
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
        head = ([point], [tp], pil, sc)
        code = (R.LLR_SCALE, perm)
        variants = {
            "tracking": lambda f: R.rx_profile_tracking_gpu(*base, f, *head, **kw),
            "coset_ldpc_3": lambda f: R.rx_profile_coset_gpu(*base, f, *head, *code, (), ldpc, None, **kw),
            "harq_chase": lambda f: R.rx_profile_harq_gpu(*base, f, *head, *code, ldpc, None, HR, True, **kw),
            "harq_arq": lambda f: R.rx_profile_harq_gpu(*base, f, *head, *code, ldpc, None, HR, False, **kw),
        }
        ms, last = {v: [] for v in variants}, {}
        for call in variants.values():
            call(2 * HR)                                                   # warm-up
        for rnd in range(args.rounds + 1):
            for v, call in variants.items():
                last[v] = call(frames)
                if rnd > 0:
                    ms[v].append(R.rx_profile_kernel_ms())
        res = {}
        med = {v: float(np.median(ms[v])) for v in variants}
        for v in variants:
            a = np.asarray(ms[v])
            res[v + "_kernels_ms"] = {"median": round(med[v], 2), "min": round(float(a.min()), 2), "max": round(float(a.max()), 2)}
        co = last["coset_ldpc_3"]
        for v in variants:
            for a, b in zip(last[v][:9], co[:9]):
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), v
        decodes = {"coset_ldpc_3": float(co.ldpc_codewords[0]) * cells * len(ldpc)}
        for v in ("harq_chase", "harq_arq"):
            decodes[v] = float(R._harq_transmissions(last[v]).sum())
        res["decoders_us_per_decode"] = {v: round(1e3 * (med[v] - med["tracking"]) / d, 4) for v, d in decodes.items()}
        res["decodes"] = {v: int(d) for v, d in decodes.items()}
        res["iterations_per_decode"] = {"coset_ldpc_3": round(float(co.iterations.sum()) / decodes["coset_ldpc_3"], 3),
                                        **{v: round(float(last[v].iterations.sum()) / decodes[v], 3) for v in ("harq_chase", "harq_arq")}}
        res["decoders_us_per_iteration"] = {
            "coset_ldpc_3": round(1e3 * (med["coset_ldpc_3"] - med["tracking"]) / float(co.iterations.sum()), 5),
            **{v: round(1e3 * (med[v] - med["tracking"]) / float(last[v].iterations.sum()), 5) for v in ("harq_chase", "harq_arq")}}

        def table(a):                                                      # [pairs, n_snr, n_ch, codes] -> per pair and code
            a = np.nanmean(a, axis=(1, 2))
            return {nm: dict(zip(labels, np.round(a[i], 5).tolist())) for i, nm in enumerate(names)}

        def by_snr(a):                                                     # the raised-cosine pair, per SNR point
            return {str(float(s)): np.round(np.nanmean(a[0, i], axis=0), 5).tolist() for i, s in enumerate(snr)}
        res["single_shot_fer"] = table(R.coset_fer(co)[1][0])
        for v in ("harq_chase", "harq_arq"):
            p = last[v]
            views = {"mean_transmissions": R.harq_mean_transmissions(p)[0], "residual_fer": R.harq_residual_fer(p)[0],
                     "undetected": R.harq_undetected(p)[0], "goodput": R.harq_goodput(p)[0],
                     "bits_per_sample": R.harq_bits_per_sample(p, S, st.stride)[0]}
            res[v] = {f: table(a) for f, a in views.items()}
            res[v]["acked_by_round"] = {nm: {lb: np.round(np.nanmean(R.harq_acked(p)[0, i, :, :, j], axis=(0, 1)), 4).tolist()
                                             for j, lb in enumerate(labels)} for i, nm in enumerate(names)}
            res[v]["by_snr_rc"] = {f: by_snr(views[f]) for f in ("mean_transmissions", "residual_fer", "bits_per_sample")}
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_harq N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, R = %d, "
                    "one point (cfo 0.02 and linewidth 1e-3, both free-running) behind the (1, 1) receiver, %d pilot bins of %d loaded, "
                    "n_f = %d per frame, W = %d word(s) of n = %d; LDPC %s, K = %s, max_iter %d; sym_rot %d, llr_scale %g, %d rounds"
                    % (name, st.prefix_rm, st.stride, cells, frames, S, HR, int(pil.sum()), int(alloc.sum()), n_f,
                       *R.ldpc_frame_words(n_f), " / ".join(labels), " / ".join(str(int(x)) for x in co.ldpc_info_bits[0]),
                       args.max_iter, co.sym_rot, R.LLR_SCALE, args.rounds),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": {"harq": R.rx_profile_harq_chunk_frames(st, S, m is not None, 1, False, 1, HR),
                             "coset_ldpc": R.rx_profile_ldpc_chunk_frames(st, S, m is not None, 1, False, 1)}},
            **res)), flush=True)


if __name__ == "__main__":
    main()
