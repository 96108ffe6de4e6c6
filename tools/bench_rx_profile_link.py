#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_link beside the calls it combines, in ONE run -- the shape of
tools/bench_rx_profile_pn.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame (CPW, CP 32),
2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms), each call made twice and the
second taken:
  - the plain call, and each of the five single-impairment entry points with one point (track), beside a link call with that
    impairment alone on its one point: the ratio says what the link arm's per-point pass 1 and per-lane taps cost;
  - one link point with everything on (6 dB Rapp, a 185 Hz track, timing +2, cfo 0.02 tracked, linewidth 1e-3 tracked, a
    neighbour at 0 dB), four such points, and the cost per additional point, all over the plain call's time.
Every single-impairment link result is compared with its own entry point's by bytes on the way.  One JSON line per run.  A
diagnostic route, not the hot path; the boxes switch clock states, so only figures of one run compare.

    python tools/bench_rx_profile_link.py [--frames 2000]
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
from wofdm_amd import channels as CH  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    args = ap.parse_args()
    n, k, S, pairs, n_ch, fs = 256, 4, 16, 2, 4, 5e6
    st = W.make_structure("CPW", n, 32)
    B = st.stride
    h = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"][:n_ch].astype(np.complex64)
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    w_tx = np.stack([W.tx_rc_window(st)] * pairs).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st)] * pairs).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    tracks = np.stack([CH.gen_chan_track("vehicularA", h.shape[1], 185.0, fs, B, S + 2, np.random.RandomState(77 + c))
                       for c in range(n_ch)])[None].astype(np.complex64)
    L, rapp = R.LinkPoint, R.PaPoint(R.PA_RAPP, 6.0, 2.0)
    d = B // 3
    full = L(rapp, 0, 2, 0.02, 1, 1e-3, 1, (d, 0.0))
    four = [full, L(rapp, 0, -3, 0.02, 0, 1e-3, 0, (d, 0.0)), L(R.PaPoint(R.PA_RAPP, 3.0, 2.0), 0, 1, 0.01, 1, 1e-2, 1, (d, 10.0)),
            L(R.PaPoint(R.PA_CLIP, 4.0), 0, 0, 0.05, 1, 1e-3, 0, (2 * d, -10.0))]
    cells = pairs * snr.size * n_ch
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    base = (st, k, S, w_tx, w_rx, h, snr, 1, 0)
    for name, m in (("plain", None), ("masked", mask)):
        kw = dict(active=alloc, mask=m)
        ref = R.pa_ref_power(st, k, S, w_tx, 1, 0, 64, active=alloc, mask=m).astype(np.float32)
        side = dict(tracks=tracks, knot_step=B, aci_active=~alloc, ref_power=ref, **kw)

        def timed(call, frames=args.frames):
            call(8)                                                    # warm-up
            call(frames)
            out = call(frames)
            return out, R.rx_profile_kernel_ms()

        def link(points):
            return lambda f: R.rx_profile_link_gpu(*base, f, points, **side)
        plain, ms0 = timed(lambda f: R.rx_profile_gpu(*base, f, **kw))
        own = {
            "sync": (lambda f: R.rx_profile_sync_gpu(*base, f, [(2, 0.02, 1)], **kw), L(timing=2, cfo=0.02, cfo_tracked=1), 6),
            "pn": (lambda f: R.rx_profile_pn_gpu(*base, f, [(1e-3, 1)], **kw), L(linewidth=1e-3, cpe_tracked=1), 6),
            "pa": (lambda f: R.rx_profile_pa_gpu(*base, f, [rapp], ref, **kw), L(pa=rapp), 7),
            "doppler": (lambda f: R.rx_profile_doppler_gpu(st, k, S, w_tx, w_rx, tracks, B, snr, 1, 0, f, **kw), L(track=0), 6),
            "aci": (lambda f: R.rx_profile_aci_gpu(*base, f, ~alloc, d, 0.0, **kw), L(aci=(d, 0.0)), 3),
        }
        res = {"plain_call_kernels_s": ms0 * 1e-3}
        off, ms = timed(link([L()]))
        assert all(np.ascontiguousarray(a[0]).tobytes() == b.tobytes() for a, b in zip(off[:3], plain[:3]))
        res["link_all_off_kernels_s"] = ms * 1e-3
        res["link_all_off_over_plain"] = ms / ms0
        for arm, (call, point, nf) in own.items():
            a, ms_own = timed(call)
            b, ms_link = timed(link([point]))
            a = a[:nf] if arm == "aci" else [x[0] for x in a[:nf]]
            assert all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y[0]).tobytes() for x, y in zip(a, b[:nf])), arm
            res["%s_own_kernels_s" % arm] = ms_own * 1e-3
            res["%s_link_kernels_s" % arm] = ms_link * 1e-3
            res["%s_link_over_own" % arm] = ms_link / ms_own
        _, ms1 = timed(link([full]))
        _, ms4 = timed(link(four))
        res.update({"everything_on_one_point_kernels_s": ms1 * 1e-3, "everything_on_one_point_over_plain": ms1 / ms0,
                    "everything_on_four_points_kernels_s": ms4 * 1e-3, "everything_on_four_points_over_plain": ms4 / ms0,
                    "per_additional_point_over_plain": (ms4 - ms1) / 3.0 / ms0,
                    "frame_points_per_s_kernels_4_points": cells * args.frames * 4 / (ms4 * 1e-3)})
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_link N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames_4_points": R.rx_profile_link_chunk_frames(st, S, m is not None, 4, True),
            "chunk_frames_plain_call": R.rx_profile_chunk_frames(st, S, m is not None)}, **res)), flush=True)


if __name__ == "__main__":
    main()
