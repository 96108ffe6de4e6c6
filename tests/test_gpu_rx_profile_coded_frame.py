"""``wofdm_rx_profile_coded_frame`` on the GPU (wofdm_rxprof_coded_kernel<N> as it is, and wofdm_viterbi_long_kernel behind it: one
codeword per point and frame over the point's data symbols), on the eight small shapes of tests/test_gpu_rx_profile_coded.py with
its comb, its link point, the four (cpe, post) receivers and three codes.  n256_cpw_half_masked has T = 5040, 6720 and 7560 -- beyond
the per-symbol decoder's 4608, and 5040 = 78 x 64 + 48 ends inside a block of the history --; the receivers with post have S_d = S -
2; n1024_wtx_half_masked has S = 2, one data symbol.

1. The call against its own soft bits: frame_errs equals ``viterbi_decode`` (numpy) of the exported soft bits gathered by
   ``frame_interleaver`` and ``wofdm_viterbi_decode_long`` of the same, exactly.
2. Identities by bytes: the tracking fields and the soft bits are ``wofdm_rx_profile_coded``'s; frame_errs with and without export,
   with one code or three, one point or two, over split frame ranges, on the N = 1024, S = 16 shape whose chunk ends inside a cell,
   from a repeated call; with S = 2, no post and sym_rot = 0 it is the per-symbol call's code_errs of symbol 1.
3. The soft bits against the fp64 mirror: by the half-LSB rule and ``LLR_TOL`` of tests/test_gpu_rx_profile_coded.py, imported.

S = 2 with post would be a point without a data symbol; the tracking receiver's own check (post needs S >= 3) refuses it before
anything is counted, as it does for every call built on it.  No test compares decoded counts of the fp32 chain with decoded counts
of the fp64 chain.  Measured on an MI355X: profiles/rx_profile_coded_frame.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC
import test_gpu_rx_profile_coded as TC
import test_gpu_rx_profile_tracking as TT

pytestmark = pytest.mark.gpu

L, TP = R.LinkPoint, R.TrackingPoint
FRAMES, CODES, SCALES, LLR_TOL = TC.FRAMES, TC.CODES, TC.SCALES, TC.LLR_TOL
LONG = "n256_cpw_half_masked"
ONE_SYMBOL = "n1024_wtx_half_masked"


def run_gpu(c, seed, frame_offset, frames, points=None, tracking=None, codes=CODES, sym_rot=None, ref_frames=None, **kw):
    s = TT.sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_coded_frame_gpu(*TT.head(c, seed, frame_offset, frames), c["points"] if points is None else points,
                                        c["tracking"] if tracking is None else tracking, c["pilots"], SCALES, R.LLR_SCALE, c["perm"],
                                        codes, sym_rot, **s, **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    return run_gpu(TC.case(name), TC.seed_of(name), 0, FRAMES, export=True)


def errs_of_soft_bits(c, prof, decode):
    """(info_err, cw_err) as the call shapes them, from its exported soft bits through ``decode(words [n_cw, n_f], rate)``"""
    sb = prof.soft_bits                                                 # [pairs, n_snr, n_ch, frames, points, S - 1, N, 8]
    pos = R._code_prepare(c["st"], c["k"], c["active"], c["pilots"], (2,), c["perm"], R.LLR_SCALE)[2]
    info, cw = np.zeros(prof.info_err.shape, np.uint64), np.zeros(prof.cw_err.shape, np.uint64)
    for i, tp in enumerate(c["tracking"]):
        words = R.frame_codewords(sb[:, :, :, :, i], tp.post, pos, c["perm"], prof.sym_rot)   # [pairs, n_snr, n_ch, frames, n_f]
        assert words.shape[-1] == pos.size * (c["S"] - 1 - tp.post)
        for j, r in enumerate(prof.rates):
            bits, _ = decode(words.reshape(-1, words.shape[-1]), r)
            bits = bits.reshape(words.shape[:4] + (-1,))
            assert bits.shape[-1] == prof.info_bits[i, j] + 6
            info[i, :, :, :, j] = bits[..., :bits.shape[-1] - 6].sum(axis=(3, 4))
            cw[i, :, :, :, j] = bits.any(axis=-1).sum(axis=3)
    return info, cw


# ---- 1. the call against its own soft bits ----

@pytest.mark.parametrize("name", TT.CASES)
def test_frame_errs_are_the_decoders_of_the_exported_soft_bits(name):
    c, got = TC.case(name), gpu_profile(name)
    S = c["S"]
    n_c = c["k"] * int((c["on"] & ~c["pilots"]).sum())
    assert type(got) is R.RxProfileCodedFrame and got.rates == CODES and got.sym_rot == (n_c // (S - 1)) % n_c
    assert got.info_err.shape == got.cw_err.shape == (len(c["points"]), RC.PAIRS, RC.N_SNR, RC.N_CH, 3)
    assert got.info_bits.tolist() == [[R.code_steps(r, n_c * (S - 1 - tp.post)) - 6 for r in CODES] for tp in c["tracking"]]
    if name == LONG:
        assert got.info_bits[0, 0] + 6 > _lib.CODE_MAX_STEPS and (got.info_bits[0, 0] + 6) % 64 != 0
    info, cw = errs_of_soft_bits(c, got, R.viterbi_decode)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw), name
    info, cw = errs_of_soft_bits(c, got, R.viterbi_decode_long_gpu)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw), name
    assert (got.codewords == FRAMES).all() and (got.cw_err <= FRAMES).all()
    assert (got.info_err <= FRAMES * got.info_bits[:, None, None, None, :]).all()
    print("%s: frame errors per code %s of %d, info-bit errors %s" % (name, got.cw_err.sum(axis=(0, 1, 2, 3)),
                                                                      int(got.codewords.sum()) * 8, got.info_err.sum(axis=(0, 1, 2, 3))))


# ---- 2. identities by bytes ----

@pytest.mark.parametrize("name", TT.CASES)
def test_tracking_fields_and_soft_bits_are_the_coded_calls(name):
    got, sym = gpu_profile(name), TC.gpu_profile(name)
    assert TT.same_bits(got[:9], sym[:9]), name
    for f in ("scales", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(got, f), getattr(sym, f)), f
    assert got.soft_bits.dtype == np.int8 and got.soft_bits.tobytes() == sym.soft_bits.tobytes()


@pytest.mark.parametrize("name", ("n64_wtx_plain", LONG, TT.OWN))
def test_identities_by_bytes(name):
    c, seed, got = TC.case(name), TC.seed_of(name), gpu_profile(name)
    plain = run_gpu(c, seed, 0, FRAMES)
    assert plain.soft_bits is None
    assert np.array_equal(plain.info_err, got.info_err) and np.array_equal(plain.cw_err, got.cw_err)
    assert TT.same_bits(plain[:9], got[:9])
    again = run_gpu(c, seed, 0, FRAMES, export=True)
    assert np.array_equal(again.soft_bits, got.soft_bits)
    assert np.array_equal(again.info_err, got.info_err) and np.array_equal(again.cw_err, got.cw_err)
    one = run_gpu(c, seed, 0, FRAMES, codes=(1,))
    assert np.array_equal(one.info_err[..., 0], got.info_err[..., 1]) and np.array_equal(one.cw_err[..., 0], got.cw_err[..., 1])
    last = len(c["points"]) - 1
    assert c["tracking"][last].post == 1                                # (alone, the S - 2 symbols' codeword is the launch's only length)
    alone = run_gpu(c, seed, 0, FRAMES, c["points"][last:], c["tracking"][last:], sym_rot=got.sym_rot)
    assert np.array_equal(alone.info_err[0], got.info_err[last]) and np.array_equal(alone.cw_err[0], got.cw_err[last])
    two = run_gpu(c, seed, 0, FRAMES, [c["points"][last], L(linewidth=0.11)], [c["tracking"][last], TP(1, 0)], sym_rot=got.sym_rot)
    assert np.array_equal(two.info_err[0], got.info_err[last]) and np.array_equal(two.cw_err[0], got.cw_err[last])
    # another rotation is another interleaver: the soft bits stay, the counts are its own decoders'
    other = run_gpu(c, seed, 0, FRAMES, sym_rot=1, export=True)
    assert other.sym_rot == 1 and np.array_equal(other.soft_bits, got.soft_bits)
    info, cw = errs_of_soft_bits(c, other, R.viterbi_decode_long_gpu)
    assert np.array_equal(other.info_err, info) and np.array_equal(other.cw_err, cw)


def test_split_frame_ranges_accumulate_to_one_call():
    c, seed = TC.case(LONG), TC.seed_of(LONG)
    one = run_gpu(c, seed, 0, 8)
    a = run_gpu(c, seed, 0, 5, ref_frames=(0, 8))
    both = run_gpu(c, seed, 5, 3, ref_frames=(0, 8), out=a)
    for f in ("info_err", "cw_err", "codewords", "bit_err", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert one.cw_err.sum() > 0 and (one.codewords == 8).all()
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), codes=(0,), out=a)
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), sym_rot=3, out=a)


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points: a chunk of the documented budget -- the history's term included -- ends inside a
    cell; neither the split of the frame range nor another chunking (one point makes a frame smaller) changes frame_errs -- no mirror
    here.  T = 12 544 and 18 816 over the 14 data symbols of the two points with post."""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    act = CM.half_band_allocation(1024)
    pil = R.pilot_comb(act, 8)
    n_data = int((act & ~pil).sum())
    perm = R.default_interleaver(c["k"] * n_data)
    pts, tps = [L(linewidth=0.01), L(cfo=0.01, cfo_tracked=0)], [TP(1, 1), TP(0, 1)]
    per_chunk = R.rx_profile_coded_frame_chunk_frames(st, c["k"], S, False, 2, False, 1, n_data, (0, 2), post=True)
    assert 100 < per_chunk < R.rx_profile_coded_chunk_frames(st, S, False, 2, False, 1)
    frames = per_chunk // 2 + 19

    def run(f0, n, points=pts, tracking=tps, **kw):
        return W.rx_profile_coded_frame_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, points, tracking, pil,
                                            SCALES, R.LLR_SCALE, perm, (0, 2), 128, active=act, **kw)
    one = run(0, frames)
    assert (frames * 8) % per_chunk != 0 and frames % per_chunk != 0 and R.rx_profile_kernel_ms() > 0.0
    assert one.cw_err.sum() > 0 and (one.codewords == frames).all()
    assert one.info_bits.tolist() == [[12544 - 6, 18816 - 6]] * 2
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    assert np.array_equal(parts.info_err, one.info_err) and np.array_equal(parts.cw_err, one.cw_err)
    assert np.array_equal(parts.codewords, one.codewords)
    one_point = R.rx_profile_coded_frame_chunk_frames(st, c["k"], S, False, 1, False, 1, n_data, (0, 2), post=True)
    assert per_chunk < one_point and frames % one_point != 0
    alone = run(0, frames, points=pts[1:], tracking=tps[1:])
    assert np.array_equal(alone.info_err[0], one.info_err[1]) and np.array_equal(alone.cw_err[0], one.cw_err[1])
    sym = W.rx_profile_coded_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, 0, frames, pts, tps, pil, SCALES, R.LLR_SCALE,
                                 perm, (0,), active=act)
    assert np.array_equal(sym.bit_err, one.bit_err) and np.array_equal(sym.sym_err, one.sym_err)


def test_one_data_symbol_without_rotation_is_the_per_symbol_call():
    c, seed = TC.case(ONE_SYMBOL), TC.seed_of(ONE_SYMBOL)
    assert c["S"] == 2 and all(tp.post == 0 for tp in c["tracking"])
    got, sym = run_gpu(c, seed, 0, FRAMES, sym_rot=0), TC.gpu_profile(ONE_SYMBOL)
    assert sym.info_err.shape[-1] == 1 and sym.cw_err.sum() > 0
    assert np.array_equal(got.info_err, sym.info_err[..., 0]) and np.array_equal(got.cw_err, sym.cw_err[..., 0])
    assert np.array_equal(got.info_bits, np.tile(sym.info_bits, (len(c["tracking"]), 1)))
    # ... and a postamble beside the one data symbol would leave none: refused before anything is counted, as the tracking call does
    with pytest.raises(ValueError):
        run_gpu(c, seed, 0, FRAMES, c["points"][:1], [TP(0, 1)], sym_rot=0)


# ---- 3. the soft bits against the mirror ----

@pytest.mark.parametrize("name", TT.CASES)
def test_soft_bits_against_the_mirror(name):
    """The rule and the figures of tests/test_gpu_rx_profile_coded.py: the soft bits are that call's bytes"""
    c = TC.case(name)
    (ref, t, w), got = TC.reference(name), gpu_profile(name)
    k = c["k"]
    d = got.soft_bits
    assert d.shape == ref.soft_bits.shape and (d[..., k:] == 0).all()
    data = np.tile(c["on"] & ~c["pilots"], (c["S"] - 1, 1))
    for i, tp in enumerate(c["tracking"]):
        taken = data.copy()
        if tp.post:
            taken[c["S"] - 2] = False
        di, ti, wi = d[:, :, :, :, i].astype(np.float64)[..., :k], t[:, :, :, :, i], w[:, :, :, :, i]
        assert (di[..., ~taken, :] == 0).all(), (name, i)
        ok = ~np.isnan(ti)
        want = np.clip(np.where(ok, ti, 0.0), -127.0, 127.0)
        room = (1.0 + np.minimum(np.abs(want), 127.0)) * wi[..., None]
        diff = np.abs(di - want)
        assert (diff[..., taken, :] <= 0.5 + LLR_TOL * room[..., taken, :])[ok[..., taken, :]].all(), (name, i)
        assert (di[~ok] == 0).all()


def test_coded_frame_for_window_file_equals_the_direct_calls(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    pts, tps = [L(), L(cfo=0.02, cfo_tracked=0)], [TP(0, 0), TP(1, 1)]
    gpu = W.coded_frame_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, SCALES, gpu=True, **kw)
    assert list(gpu) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    pil = R.pilot_comb(alloc, 4)
    perm = R.default_interleaver(4 * int((alloc & ~pil).sum()))
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want = W.rx_profile_coded_frame_gpu(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, tps, pil, SCALES, R.LLR_SCALE, perm, (0, 1, 2),
                                            active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g = gpu[name][key]
            assert type(g) is R.RxProfileCodedFrame and g.info_err.shape == (2, 2, 2, 3)
            assert TT.same_bits(g[:9], [a[:, i] for a in want[:9]]), (name, key)
            assert np.array_equal(g.info_err, want.info_err[:, i]) and np.array_equal(g.cw_err, want.cw_err[:, i])
            assert np.array_equal(g.codewords, want.codewords) and np.array_equal(g.info_bits, want.info_bits)
            assert R.coded_frame_ber(g).shape == R.coded_fer(g).shape == (2, 2, 2, 3)
