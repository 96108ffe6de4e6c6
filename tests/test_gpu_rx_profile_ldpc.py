"""``wofdm_rx_profile_ldpc`` on the GPU (wofdm_rxprof_coded_kernel<N> as it is, and wofdm_ldpc_kernel behind it: per point and
frame W codewords of a quasi-cyclic LDPC code over the point's data symbols), on the eight small shapes of
tests/test_gpu_rx_profile_coded.py -- 8 cells x 2 frames -- with its comb, its link point, the four (cpe, post) receivers and three
codes: (4, 8) with 30 iterations, (3, 6) with 5, which most words do not finish in, and (4, 12) with 64.

1. The call against its own soft bits: all four fields of ldpc_errs equal ``ldpc_decode`` (numpy) of the exported soft bits
   gathered by ``frame_interleaver`` and ``wofdm_ldpc_decode`` of the same, exactly.
2. Identities by bytes: the seven tracking outputs and the soft bits are ``wofdm_rx_profile_coded_frame``'s; ldpc_errs with and
   without export, with one code or three, one point or two, over split frame ranges, from a repeated call; and on N = 1024,
   64-QAM, S = 16 -- n_f = 37 632 with a postamble, W = 3 words of 12 544 -- with a chunk that ends inside a cell.

No test compares decoded counts of the fp32 chain with decoded counts of the fp64 chain.  Measured on an
MI355X: profiles/rx_profile_ldpc.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC
import test_gpu_rx_profile_coded as TC
import test_gpu_rx_profile_coded_frame as TCF
import test_gpu_rx_profile_tracking as TT

pytestmark = pytest.mark.gpu

L, TP = R.LinkPoint, R.TrackingPoint
FRAMES, SCALES = TC.FRAMES, TC.SCALES
CODES = ((4, 8, 30), (3, 6, 5), (4, 12, 64))
FIELDS = ("info_err", "cw_err", "unconverged", "iterations")


def run_gpu(c, seed, frame_offset, frames, points=None, tracking=None, codes=CODES, sym_rot=None, ref_frames=None, **kw):
    s = TT.sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_ldpc_gpu(*TT.head(c, seed, frame_offset, frames), c["points"] if points is None else points,
                                 c["tracking"] if tracking is None else tracking, c["pilots"], SCALES, R.LLR_SCALE, c["perm"],
                                 codes, sym_rot, **s, **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    return run_gpu(TC.case(name), TC.seed_of(name), 0, FRAMES, export=True)


def same_counts(a, b, ia=Ellipsis, ib=Ellipsis):
    return all(np.array_equal(getattr(a, f)[ia], getattr(b, f)[ib]) for f in FIELDS)


def errs_of_soft_bits(c, prof, decode):
    """the four counters as the call shapes them, from its exported soft bits through ``decode(words [n_cw, n], J, L, max_iter)``"""
    sb = prof.soft_bits                                                 # [pairs, n_snr, n_ch, frames, points, S - 1, N, 8]
    pos = R._code_prepare(c["st"], c["k"], c["active"], c["pilots"], (2,), c["perm"], R.LLR_SCALE)[2]
    out = np.zeros((4,) + prof.info_err.shape, np.uint64)
    for i, tp in enumerate(c["tracking"]):
        stream = R.frame_codewords(sb[:, :, :, :, i], tp.post, pos, c["perm"], prof.sym_rot)   # [pairs, n_snr, n_ch, frames, n_f]
        n_words, n = R.ldpc_frame_words(stream.shape[-1])
        assert prof.codewords[i] == n_words * stream.shape[3]
        words = stream[..., :n_words * n].reshape(-1, n)
        for j, (J, Lc, m) in enumerate(prof.codes):
            bits, iters, conv = decode(words, J, Lc, m)
            Z = R.ldpc_lift(J, Lc, n)
            assert prof.info_bits[i, j] == n - J * Z
            info = bits[:, J * Z:].reshape(stream.shape[:4] + (n_words, -1))
            per = (info.sum(axis=-1), info.any(axis=-1), ~conv.reshape(info.shape[:-1]), iters.reshape(info.shape[:-1]))
            for f, a in enumerate(per):
                out[f][i, :, :, :, j] = a.sum(axis=(3, 4))
    return out


# ---- 1. the call against its own soft bits ----

@pytest.mark.parametrize("name", TT.CASES)
def test_ldpc_errs_are_the_decoders_of_the_exported_soft_bits(name):
    c, got = TC.case(name), gpu_profile(name)
    n_c = c["k"] * int((c["on"] & ~c["pilots"]).sum())
    assert type(got) is R.RxProfileLdpc and got.codes == CODES and got.sym_rot == (n_c // (c["S"] - 1)) % n_c
    assert got.info_err.shape == (len(c["points"]), RC.PAIRS, RC.N_SNR, RC.N_CH, 3)
    want = errs_of_soft_bits(c, got, R.ldpc_decode)
    for f, a in zip(FIELDS, want):
        assert np.array_equal(getattr(got, f), a), (name, f)
    want = errs_of_soft_bits(c, got, R.ldpc_decode_gpu)
    for f, a in zip(FIELDS, want):
        assert np.array_equal(getattr(got, f), a), (name, f)
    words = got.codewords[:, None, None, None, None]
    assert (got.cw_err <= words).all() and (got.unconverged <= words).all() and (got.iterations >= words).all()
    assert (got.iterations <= words * np.array([m for _, _, m in CODES], np.uint64)).all()
    assert (got.info_err <= words * got.info_bits[:, None, None, None, :]).all()
    print("%s: per code, of %d words: in error %s, unconverged %s, iterations %s, info-bit errors %s"
          % (name, int(got.codewords.sum()) * 8, got.cw_err.sum(axis=(0, 1, 2, 3)), got.unconverged.sum(axis=(0, 1, 2, 3)),
             got.iterations.sum(axis=(0, 1, 2, 3)), got.info_err.sum(axis=(0, 1, 2, 3))))


def test_the_cases_hold_words_that_converge_and_words_that_do_not():
    conv = unconv = early = 0
    for name in TT.CASES[:4]:
        got = gpu_profile(name)
        words = int(got.codewords.sum()) * 8
        unconv += int(got.unconverged[..., 0].sum())
        conv += words - int(got.unconverged[..., 0].sum())
        early += int((got.iterations[..., 0] < 30 * got.codewords[:, None, None, None]).sum())
    assert conv > 0 and unconv > 0 and early > 0


# ---- 2. identities by bytes ----

@pytest.mark.parametrize("name", TT.CASES)
def test_tracking_fields_and_soft_bits_are_the_coded_frame_calls(name):
    got, frm = gpu_profile(name), TCF.gpu_profile(name)
    assert TT.same_bits(got[:9], frm[:9]), name
    for f in ("scales", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(got, f), getattr(frm, f)), f
    assert got.sym_rot == frm.sym_rot
    assert got.soft_bits.dtype == np.int8 and got.soft_bits.tobytes() == frm.soft_bits.tobytes()


@pytest.mark.parametrize("name", ("n64_wtx_plain", TCF.LONG, TT.OWN))
def test_identities_by_bytes(name):
    c, seed, got = TC.case(name), TC.seed_of(name), gpu_profile(name)
    plain = run_gpu(c, seed, 0, FRAMES)
    assert plain.soft_bits is None and same_counts(plain, got) and TT.same_bits(plain[:9], got[:9])
    again = run_gpu(c, seed, 0, FRAMES, export=True)
    assert np.array_equal(again.soft_bits, got.soft_bits) and same_counts(again, got)
    one = run_gpu(c, seed, 0, FRAMES, codes=CODES[1:2])
    assert same_counts(one, got, (Ellipsis, 0), (Ellipsis, 1))
    last = len(c["points"]) - 1
    assert c["tracking"][last].post == 1                                # (alone, the S - 2 symbols' word is the launch's only length)
    alone = run_gpu(c, seed, 0, FRAMES, c["points"][last:], c["tracking"][last:], sym_rot=got.sym_rot)
    assert same_counts(alone, got, 0, last)
    two = run_gpu(c, seed, 0, FRAMES, [c["points"][last], L(linewidth=0.11)], [c["tracking"][last], TP(1, 0)], sym_rot=got.sym_rot)
    assert same_counts(two, got, 0, last)
    # another rotation is another interleaver: the soft bits stay, the counts are its own decoder's
    other = run_gpu(c, seed, 0, FRAMES, sym_rot=1, export=True)
    assert other.sym_rot == 1 and np.array_equal(other.soft_bits, got.soft_bits)
    for f, a in zip(FIELDS, errs_of_soft_bits(c, other, R.ldpc_decode_gpu)):
        assert np.array_equal(getattr(other, f), a), f


def test_split_frame_ranges_accumulate_to_one_call():
    c, seed = TC.case(TCF.LONG), TC.seed_of(TCF.LONG)
    one = run_gpu(c, seed, 0, 8)
    a = run_gpu(c, seed, 0, 5, ref_frames=(0, 8))
    both = run_gpu(c, seed, 5, 3, ref_frames=(0, 8), out=a)
    for f in FIELDS + ("codewords", "bit_err", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (one.codewords == 8).all() and one.iterations.sum() > 0
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), codes=CODES[:1], out=a)
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), sym_rot=3, out=a)


def test_several_words_per_frame_and_chunks_that_end_inside_a_cell():
    """N = 1024, 64-QAM, S = 16, cp + cs = 64, two points with a postamble: n_f = 6 x 448 x 14 = 37 632 > 16384, W = 3 words of
    12 544; a chunk of the documented budget ends inside a cell; neither the split of the frame range nor another chunking (one point
    makes a frame smaller) changes ldpc_errs.  The first frames' words against the decoder alone on the exported soft bits."""
    st, S, k = W.make_structure("wtx", 1024, 56), 16, 6
    c = RC.make_case(st, k, S, "plain", 3001)
    act = CM.half_band_allocation(1024)
    pil = R.pilot_comb(act, 8)
    n_c = k * int((act & ~pil).sum())
    perm = R.default_interleaver(n_c)
    pts, tps = [L(linewidth=0.01), L(cfo=0.01, cfo_tracked=0)], [TP(1, 1), TP(0, 1)]
    codes = ((4, 8, 6), (4, 16, 10))
    assert n_c * (S - 2) == 37632 and R.ldpc_frame_words(n_c * (S - 2)) == (3, 12544)
    per_chunk = R.rx_profile_ldpc_chunk_frames(st, S, False, 2, False, 1)
    assert per_chunk == R.rx_profile_coded_chunk_frames(st, S, False, 2, False, 1) and per_chunk > 100
    frames = per_chunk // 2 + 19

    def run(f0, n, points=pts, tracking=tps, **kw):
        return W.rx_profile_ldpc_gpu(st, k, S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, points, tracking, pil, SCALES,
                                     R.LLR_SCALE, perm, codes, 128, active=act, **kw)
    one = run(0, frames)
    assert (frames * 8) % per_chunk != 0 and frames % per_chunk != 0 and R.rx_profile_kernel_ms() > 0.0
    assert (one.codewords == 3 * frames).all() and one.iterations.min() >= 3 * frames
    assert one.info_bits.tolist() == [[12544 - 4 * R.ldpc_lift(4, 8, 12544), 12544 - 4 * R.ldpc_lift(4, 16, 12544)]] * 2
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    assert same_counts(parts, one) and np.array_equal(parts.codewords, one.codewords)
    one_point = R.rx_profile_ldpc_chunk_frames(st, S, False, 1, False, 1)
    assert per_chunk < one_point and frames % one_point != 0
    alone = run(0, frames, points=pts[1:], tracking=tps[1:])
    assert same_counts(alone, one, 0, 1)
    few = run(0, 2, export=True)
    cc = dict(c, active=act, pilots=pil, perm=perm, tracking=tps)
    for f, a in zip(FIELDS, errs_of_soft_bits(cc, few, R.ldpc_decode_gpu)):
        assert np.array_equal(getattr(few, f), a), f
    for f, a in zip(FIELDS, errs_of_soft_bits(cc, few._replace(soft_bits=few.soft_bits[:1, :1]), R.ldpc_decode)):
        assert np.array_equal(getattr(few, f)[:, :1, :1], a[:, :1, :1]), f


def test_ldpc_for_window_file_equals_the_direct_calls(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    pts, tps = [L(), L(cfo=0.02, cfo_tracked=0)], [TP(0, 0), TP(1, 1)]
    codes = ((4, 8), (3, 6, 12))
    gpu = W.ldpc_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, SCALES, codes=codes, gpu=True, **kw)
    assert list(gpu) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    pil = R.pilot_comb(alloc, 4)
    perm = R.default_interleaver(4 * int((alloc & ~pil).sum()))
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want = W.rx_profile_ldpc_gpu(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, tps, pil, SCALES, R.LLR_SCALE, perm, codes,
                                     active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g = gpu[name][key]
            assert type(g) is R.RxProfileLdpc and g.info_err.shape == (2, 2, 2, 2)
            assert TT.same_bits(g[:9], [a[:, i] for a in want[:9]]), (name, key)
            assert same_counts(g, want, Ellipsis, (slice(None), i))
            assert np.array_equal(g.codewords, want.codewords) and np.array_equal(g.info_bits, want.info_bits)
            assert g.codes == ((4, 8, R.LDPC_MAX_ITER), (3, 6, 12))
            assert R.ldpc_ber(g).shape == R.ldpc_fer(g).shape == R.ldpc_mean_iterations(g).shape == (2, 2, 2, 2)
