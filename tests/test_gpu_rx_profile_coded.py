"""``wofdm_rx_profile_coded`` on the GPU (wofdm_rxprof_coded_kernel<N> = the tracking kernel plus the soft-bit stores, and
wofdm_viterbi_kernel behind it), on the cases of tests/test_gpu_rx_profile_tracking.py with its comb and the four (cpe, post)
receivers behind a free-running carrier offset.  Three links, none of them across a discontinuity:

1. The exported soft bits against the fp64 mirror's z: |d_gpu - clip(llr_scale z_ref, +-127)| <= 0.5 + LLR_TOL (1 + min(|llr_scale
   z_ref|, 127)) w_s[n], w_s[n] = max_m |Hh_s[m]| / |Hh_s[n]| the tracking near rule's weight; d_gpu is exactly 0 where no decision
   is taken.  LLR_TOL began at 1e-3, the project's POW_TOL (z is quadratic in e, as err_power is), and is four times the largest
   excess measured; it may never reach 0.5 / 128.
2. The call against its own soft bits: code_errs equals ``viterbi_decode`` (numpy) of the exported soft bits and
   ``wofdm_viterbi_decode`` of them, exactly.
3. Identities by bytes: the tracking call's fields; code_errs with and without export, with one code or three, one point or two,
   over split frame ranges, on the N = 1024, S = 16 shape whose chunk ends inside a cell; ``coded_for_window_file``.

No test compares decoded counts of the fp32 chain with decoded counts of the fp64 chain: a decoder amplifies a one-LSB difference
arbitrarily.  Measured on an MI355X: profiles/rx_profile_coded.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC
import test_gpu_rx_profile_tracking as TT

pytestmark = pytest.mark.gpu

L, TP = R.LinkPoint, R.TrackingPoint
#: four times the largest excess measured on an MI355X, 8.59e-7 (profiles/rx_profile_coded.txt); the issue's start was POW_TOL = 1e-3
LLR_TOL = 3.4e-6
assert LLR_TOL < 0.5 / 128
FRAMES = 2
CODES = (0, 1, 2)
SCALES = (0.5,)


@functools.lru_cache(maxsize=None)
def case(name):
    """the tracking test's case with one link point, a free-running carrier offset, behind each of its receivers"""
    c = dict(TT.case(name))
    receivers = [TP(0, 0), TP(1, 0)] + ([TP(0, 1), TP(1, 1)] if c["S"] >= 3 else [])
    c["points"], c["tracking"] = [L(cfo=0.02, cfo_tracked=0)] * len(receivers), receivers
    n_c = c["k"] * int((c["on"] & ~c["pilots"]).sum())
    c["perm"] = R.default_interleaver(n_c)
    return c


def seed_of(name):
    return TT.base_seed(name) + 3


def run_gpu(c, seed, frame_offset, frames, points=None, tracking=None, codes=CODES, ref_frames=None, **kw):
    s = TT.sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_coded_gpu(*TT.head(c, seed, frame_offset, frames), c["points"] if points is None else points,
                                  c["tracking"] if tracking is None else tracking, c["pilots"], SCALES, R.LLR_SCALE, c["perm"], codes,
                                  **s, **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c = case(name)
    return run_gpu(c, seed_of(name), 0, FRAMES, export=True)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the mirror's profile with its soft bits, llr_scale z unrounded and the weights; computed once, not to be modified"""
    c = case(name)
    seed = seed_of(name)
    return R.rx_profile_coded_host(*TT.head(c, seed, 0, FRAMES), c["points"], c["tracking"], c["pilots"], SCALES, R.LLR_SCALE, c["perm"],
                                   (0,), with_soft=True, **TT.sides(c, seed, 0, FRAMES))


def errs_of_soft_bits(c, prof, decode):
    """(info_err, cw_err) as the call shapes them, from its exported soft bits through ``decode(soft [n_cw, n_c], rate, perm)``"""
    sb = prof.soft_bits
    rates, perm, pos, steps = R._code_prepare(c["st"], c["k"], c["active"], c["pilots"], prof.rates, c["perm"], R.LLR_SCALE)
    pairs, n_snr, n_ch, frames, n_pts, S1 = sb.shape[:6]
    stream = sb.reshape(sb.shape[:6] + (-1,))[..., pos]                  # [pairs, n_snr, n_ch, frames, points, S - 1, n_c]
    info, cw = np.zeros(prof.info_err.shape, np.uint64), np.zeros(prof.cw_err.shape, np.uint64)
    for j, r in enumerate(rates):
        bits, _ = decode(stream.reshape(-1, pos.size), r, perm)
        bits = bits.reshape(stream.shape[:6] + (-1,))
        for i, tp in enumerate(c["tracking"]):
            use = S1 - 1 if tp.post else S1
            b = bits[:, :, :, :, i, :use]
            info[i, :, :, :, j, :use] = b[..., :steps[j] - 6].sum(axis=(3, 5))
            cw[i, :, :, :, j, :use] = b.any(axis=-1).sum(axis=3)
    return info, cw


# ---- 1. the soft bits against the mirror ----

@pytest.mark.parametrize("name", TT.CASES)
def test_soft_bits_against_the_mirror(name):
    """Measured on an MI355X: profiles/rx_profile_coded.txt"""
    c = case(name)
    (ref, t, w), got = reference(name), gpu_profile(name)
    k = c["k"]
    d = got.soft_bits
    assert d.dtype == np.int8 and d.shape == ref.soft_bits.shape and (d[..., k:] == 0).all()
    data = np.tile(c["on"] & ~c["pilots"], (c["S"] - 1, 1))
    for i, tp in enumerate(c["tracking"]):
        taken = data.copy()
        if tp.post:
            taken[c["S"] - 2] = False
        di, ti, wi = d[:, :, :, :, i].astype(np.float64)[..., :k], t[:, :, :, :, i], w[:, :, :, :, i]
        assert (di[..., ~taken, :] == 0).all(), (name, i)                # exactly 0 wherever no decision is taken
        ok = ~np.isnan(ti)
        want = np.clip(np.where(ok, ti, 0.0), -127.0, 127.0)
        room = (1.0 + np.minimum(np.abs(want), 127.0)) * wi[..., None]
        diff = np.abs(di - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(taken[..., None] & ok, (diff - 0.5) / room, 0.0)
        moved = (di != ref.soft_bits[:, :, :, :, i].astype(np.float64)[..., :k])[..., taken, :].mean()
        clamp = (np.abs(ref.soft_bits[:, :, :, :, i][..., taken, :k].astype(np.int64)) == 127).mean()
        print("%s point %d (%d, %d): largest (|d - llr z| - 0.5) / ((1 + |llr z|) w) = %.2e; %.2f %% of the soft bits differ from "
              "the mirror's, %.1f %% clamp" % (name, i, tp.cpe, tp.post, ratio.max(), 100 * moved, 100 * clamp))
        assert (diff[..., taken, :] <= 0.5 + LLR_TOL * room[..., taken, :])[ok[..., taken, :]].all(), (name, i, ratio.max())
        assert (di[~ok] == 0).all()
    assert (np.abs(d.astype(np.int64)) <= 127).all() and (d != 0).any()


# ---- 2. the call against its own soft bits ----

@pytest.mark.parametrize("name", TT.CASES)
def test_code_errs_are_the_decoders_of_the_exported_soft_bits(name):
    c, got = case(name), gpu_profile(name)
    assert type(got) is R.RxProfileCoded and got.rates == CODES
    assert got.info_err.shape == (len(c["points"]), RC.PAIRS, RC.N_SNR, RC.N_CH, 3, c["S"] - 1)
    info, cw = errs_of_soft_bits(c, got, R.viterbi_decode)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw), name
    info, cw = errs_of_soft_bits(c, got, R.viterbi_decode_gpu)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw), name
    for i, tp in enumerate(c["tracking"]):
        assert int(got.codewords[i, -1]) == (0 if tp.post else FRAMES)
        if tp.post:
            assert (got.info_err[i, ..., -1] == 0).all() and (got.cw_err[i, ..., -1] == 0).all()
    assert (got.cw_err <= FRAMES).all() and (got.info_err <= FRAMES * got.info_bits[None, None, None, None, :, None]).all()
    print("%s: codeword errors per code %s of %d" % (name, got.cw_err.sum(axis=(0, 1, 2, 3, 5)), int(got.codewords.sum()) * 8))


# ---- 3. identities by bytes ----

@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", TT.OWN))
def test_identities_by_bytes(name):
    c, seed, got = case(name), seed_of(name), gpu_profile(name)
    trk = TT.run_gpu(c, seed, 0, FRAMES, c["points"], c["tracking"], scales=SCALES)
    assert TT.same_bits(got[:9], trk[:9]), name
    for f in ("scales", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(got, f), getattr(trk, f)), f
    plain = run_gpu(c, seed, 0, FRAMES)
    assert plain.soft_bits is None
    assert np.array_equal(plain.info_err, got.info_err) and np.array_equal(plain.cw_err, got.cw_err)
    assert TT.same_bits(plain[:9], got[:9])
    again = run_gpu(c, seed, 0, FRAMES, export=True)
    assert np.array_equal(again.soft_bits, got.soft_bits) and np.array_equal(again.info_err, got.info_err)
    one = run_gpu(c, seed, 0, FRAMES, codes=(1,))
    assert np.array_equal(one.info_err[..., 0, :], got.info_err[..., 1, :]) and np.array_equal(one.cw_err[..., 0, :], got.cw_err[..., 1, :])
    last = len(c["points"]) - 1
    alone = run_gpu(c, seed, 0, FRAMES, c["points"][last:], c["tracking"][last:])
    assert np.array_equal(alone.info_err[0], got.info_err[last]) and np.array_equal(alone.cw_err[0], got.cw_err[last])
    two = run_gpu(c, seed, 0, FRAMES, [c["points"][last], L(linewidth=0.11)], [c["tracking"][last], TP(1, 0)])
    assert np.array_equal(two.info_err[0], got.info_err[last]) and np.array_equal(two.cw_err[0], got.cw_err[last])


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed = case(name), seed_of(name)
    one = run_gpu(c, seed, 0, 8)
    a = run_gpu(c, seed, 0, 5, ref_frames=(0, 8))
    both = run_gpu(c, seed, 5, 3, ref_frames=(0, 8), out=a)
    for f in ("info_err", "cw_err", "codewords", "bit_err", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert one.cw_err.sum() > 0
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), codes=(0,), out=a)


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points: a chunk of the documented budget ends inside a cell; neither the split of the frame
    range nor another chunking (one point makes a frame smaller) changes code_errs -- no mirror here"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    act = CM.half_band_allocation(1024)
    pil = R.pilot_comb(act, 8)
    perm = R.default_interleaver(c["k"] * int((act & ~pil).sum()))
    pts, tps = [L(linewidth=0.01), L(cfo=0.01, cfo_tracked=0)], [TP(1, 1), TP(0, 1)]
    per_chunk = R.rx_profile_coded_chunk_frames(st, S, False, 2, False, 1)
    assert 100 < per_chunk < R.rx_profile_tracking_chunk_frames(st, S, False, 2, False, 1)
    frames = per_chunk // 2 + 19

    def run(f0, n, points=pts, tracking=tps, **kw):
        return W.rx_profile_coded_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, points, tracking, pil, SCALES,
                                      R.LLR_SCALE, perm, (0, 2), active=act, **kw)
    one = run(0, frames)
    assert (frames * 8) % per_chunk != 0 and frames % per_chunk != 0 and R.rx_profile_kernel_ms() > 0.0
    assert (one.cw_err[..., S - 2] == 0).all() and one.cw_err.sum() > 0 and int(one.codewords[0, 0]) == frames
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    assert np.array_equal(parts.info_err, one.info_err) and np.array_equal(parts.cw_err, one.cw_err)
    assert np.array_equal(parts.codewords, one.codewords)
    one_point = R.rx_profile_coded_chunk_frames(st, S, False, 1, False, 1)
    assert per_chunk < one_point and frames % one_point != 0
    alone = run(0, frames, points=pts[1:], tracking=tps[1:])
    assert np.array_equal(alone.info_err[0], one.info_err[1]) and np.array_equal(alone.cw_err[0], one.cw_err[1])
    trk = W.rx_profile_tracking_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, 0, frames, pts, tps, pil, SCALES, active=act)
    assert np.array_equal(trk.bit_err, one.bit_err) and np.array_equal(trk.sym_err, one.sym_err)


def test_coded_for_window_file_equals_the_direct_calls(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    pts, tps = [L(), L(cfo=0.02, cfo_tracked=0)], [TP(0, 0), TP(1, 1)]
    gpu = W.coded_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, SCALES, gpu=True, **kw)
    assert list(gpu) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    pil = R.pilot_comb(alloc, 4)
    perm = R.default_interleaver(4 * int((alloc & ~pil).sum()))
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want = W.rx_profile_coded_gpu(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, tps, pil, SCALES, R.LLR_SCALE, perm, (0, 1, 2),
                                      active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g = gpu[name][key]
            assert type(g) is R.RxProfileCoded and g.info_err.shape == (2, 2, 2, 3, 3)
            assert TT.same_bits(g[:9], [a[:, i] for a in want[:9]]), (name, key)
            assert np.array_equal(g.info_err, want.info_err[:, i]) and np.array_equal(g.cw_err, want.cw_err[:, i])
            assert np.array_equal(g.codewords, want.codewords) and np.array_equal(g.info_bits, want.info_bits)
            ber, cell = R.coded_ber(g)
            assert ber.shape == (2, 2, 2, 3, 3) and cell.shape == (2, 2, 2, 3) and np.isnan(ber[1, ..., -1]).all()
