"""``wofdm_rx_profile_coset`` on the GPU (wofdm_rxprof_coded_kernel<N> as it is; behind it wofdm_viterbi_coset_kernel and
wofdm_ldpc_coset_kernel, which draw the frame's information stream, encode it and decode against the transmitted word), on the
eight small shapes of tests/test_gpu_rx_profile_coded.py -- 8 cells x 2 frames -- with its comb, its link point, the four (cpe,
post) receivers, the Viterbi rates 1/2, 2/3, 3/4 and the LDPC codes (4, 8) x 30, (3, 6) x 5, (4, 12) x 64.

1. frame_errs against the call's own soft bits: gathered by ``frame_codewords``, flipped by ``coset_codewords``, decoded by
   ``viterbi_decode`` (numpy) and by ``wofdm_viterbi_decode_long``, the decoded bits compared with the stream -- exactly.
2. ldpc_errs likewise through ``ldpc_decode`` and ``wofdm_ldpc_decode`` -- exactly, all four fields.
3. By bytes, the seven tracking fields and the soft bits are ``wofdm_rx_profile_coded_frame``'s.
4. By bytes, the counters with and without export, with the Viterbi codes alone, the LDPC codes alone or both, one point or two,
   over split frame ranges, from a repeated call.
5. N = 1024, 64-QAM, S = 16 with a postamble: n_f = 37 632, W = 3, a chunk that ends inside a cell, against another chunking.
6. Two frames that straddle 2^32 under a seed whose high word is set.
7. Without any mirror decoder: a short channel at 30 and 36 dB, QPSK, where every exported soft bit is positive and the fp64 mirror's
   are all >= 4 in magnitude (both asserted): every error counter is 0 and the iterations equal the words.  A wrong word, flip or
   comparison would leave about half the bits in error.

No test compares decoded counts of the fp32 chain with decoded counts of the fp64 chain.  Measured on an
MI355X: profiles/rx_profile_coset.txt."""
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
RATES = (0, 1, 2)
CODES = ((4, 8, 30), (3, 6, 5), (4, 12, 64))
VIT = ("info_err", "cw_err")
LDPC = ("ldpc_info_err", "ldpc_cw_err", "unconverged", "iterations")


def run_gpu(c, seed, frame_offset, frames, points=None, tracking=None, codes=RATES, ldpc_codes=CODES, sym_rot=None, ref_frames=None, **kw):
    s = TT.sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_coset_gpu(*TT.head(c, seed, frame_offset, frames), c["points"] if points is None else points,
                                  c["tracking"] if tracking is None else tracking, c["pilots"], SCALES, R.LLR_SCALE, c["perm"],
                                  codes, ldpc_codes, sym_rot, **s, **kw)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    return run_gpu(TC.case(name), TC.seed_of(name), 0, FRAMES, export=True)


def same_counts(a, b, ia=Ellipsis, ib=Ellipsis, fields=VIT + LDPC):
    return all(np.array_equal(getattr(a, f)[ia], getattr(b, f)[ib]) for f in fields)


def words_of(c, prof, i, seed, frame_offset):
    """point i's frames as the decoders meet them: (soft [pairs, n_snr, n_ch, frames, n_f] int16, x [.., codes, n_f], x_ldpc [..,
    ldpc codes, n_f], the stream [.., n_f]) -- the exported soft bits gathered by ``frame_codewords``, the transmitted words of every
    (cell, frame) from ``coset_codewords``"""
    pos = R._code_prepare(c["st"], c["k"], c["active"], c["pilots"], (2,), c["perm"], R.LLR_SCALE)[2]
    soft = R.frame_codewords(prof.soft_bits[:, :, :, :, i], c["tracking"][i].post, pos, c["perm"], prof.sym_rot).astype(np.int16)
    lead, n_f = soft.shape[:4], soft.shape[-1]
    xv = np.zeros(lead + (len(prof.rates), n_f), np.uint8)
    xl = np.zeros(lead + (len(prof.ldpc_codes), n_f), np.uint8)
    stream = np.zeros(lead + (n_f,), np.uint8)
    for p, s, ch, f in np.ndindex(*lead):
        cell, frame = (p * lead[1] + s) * lead[2] + ch, frame_offset + f
        xv[p, s, ch, f], xl[p, s, ch, f] = R.coset_codewords(seed, cell, frame, n_f, prof.rates, prof.ldpc_codes)
        stream[p, s, ch, f] = R.coset_info(seed, cell, frame, n_f)
    return soft, xv, xl, stream


def viterbi_errs(c, prof, decode, seed, frame_offset=0):
    """(info_err, cw_err) as the call shapes them, through ``decode(words [n_cw, n_f], rate)`` on the flipped soft bits"""
    info, cw = np.zeros(prof.info_err.shape, np.uint64), np.zeros(prof.cw_err.shape, np.uint64)
    for i in range(len(c["tracking"])):
        soft, xv, _, stream = words_of(c, prof, i, seed, frame_offset)
        for j, r in enumerate(prof.rates):
            flipped = np.where(xv[..., j, :] != 0, -soft, soft).astype(np.int8)
            bits = decode(flipped.reshape(-1, soft.shape[-1]), r)[0].reshape(soft.shape[:4] + (-1,))
            T = bits.shape[-1]
            assert T == prof.info_bits[i, j] + 6
            wrong = bits ^ np.concatenate([stream[..., :T - 6], np.zeros(soft.shape[:4] + (6,), np.uint8)], axis=-1)
            info[i, :, :, :, j] = wrong[..., :T - 6].sum(axis=(3, 4))
            cw[i, :, :, :, j] = wrong.any(axis=-1).sum(axis=3)
    return info, cw


def ldpc_errs(c, prof, decode, seed, frame_offset=0):
    """the four LDPC counters as the call shapes them, through ``decode(words [n_cw, n], J, L, max_iter)`` on the flipped soft bits"""
    out = np.zeros((4,) + prof.ldpc_info_err.shape, np.uint64)
    for i in range(len(c["tracking"])):
        soft, _, xl, _ = words_of(c, prof, i, seed, frame_offset)
        n_words, n = R.ldpc_frame_words(soft.shape[-1])
        assert prof.ldpc_codewords[i] == n_words * soft.shape[3]
        for j, (J, Lc, m) in enumerate(prof.ldpc_codes):
            x = xl[..., j, :n_words * n]
            flipped = np.where(x != 0, -soft[..., :n_words * n], soft[..., :n_words * n]).astype(np.int8)
            bits, iters, conv = decode(flipped.reshape(-1, n), J, Lc, m)
            k0 = J * R.ldpc_lift(J, Lc, n)
            assert prof.ldpc_info_bits[i, j] == n - k0
            wrong = (bits ^ x.reshape(-1, n))[:, k0:].reshape(soft.shape[:4] + (n_words, -1))
            per = (wrong.sum(axis=-1), wrong.any(axis=-1), ~conv.reshape(wrong.shape[:-1]), iters.reshape(wrong.shape[:-1]))
            for f, a in enumerate(per):
                out[f][i, :, :, :, j] = a.sum(axis=(3, 4))
    return out


# ---- 1. and 2. the call against its own soft bits ----

@pytest.mark.parametrize("name", TT.CASES)
def test_frame_errs_are_the_decoders_of_the_flipped_soft_bits(name):
    c, got, seed = TC.case(name), gpu_profile(name), TC.seed_of(name)
    n_c = c["k"] * int((c["on"] & ~c["pilots"]).sum())
    assert type(got) is R.RxProfileCoset and got.rates == RATES and got.sym_rot == (n_c // (c["S"] - 1)) % n_c
    assert got.info_err.shape == got.cw_err.shape == (len(c["points"]), RC.PAIRS, RC.N_SNR, RC.N_CH, 3)
    assert got.info_bits.tolist() == [[R.code_steps(r, n_c * (c["S"] - 1 - tp.post)) - 6 for r in RATES] for tp in c["tracking"]]
    info, cw = viterbi_errs(c, got, R.viterbi_decode, seed)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw), name
    info, cw = viterbi_errs(c, got, R.viterbi_decode_long_gpu, seed)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw), name
    assert (got.codewords == FRAMES).all() and (got.cw_err <= FRAMES).all()
    assert (got.info_err <= FRAMES * got.info_bits[:, None, None, None, :]).all()
    frm = TCF.gpu_profile(name)
    print("%s: frame errors per code %s of %d (all-zero view %s), info-bit errors %s (all-zero view %s)"
          % (name, got.cw_err.sum(axis=(0, 1, 2, 3)), int(got.codewords.sum()) * 8, frm.cw_err.sum(axis=(0, 1, 2, 3)),
             got.info_err.sum(axis=(0, 1, 2, 3)), frm.info_err.sum(axis=(0, 1, 2, 3))))


@pytest.mark.parametrize("name", TT.CASES)
def test_ldpc_errs_are_the_decoders_of_the_flipped_soft_bits(name):
    c, got, seed = TC.case(name), gpu_profile(name), TC.seed_of(name)
    assert got.ldpc_codes == CODES and got.ldpc_info_err.shape == (len(c["points"]), RC.PAIRS, RC.N_SNR, RC.N_CH, 3)
    for decode in (R.ldpc_decode, R.ldpc_decode_gpu):
        for f, a in zip(LDPC, ldpc_errs(c, got, decode, seed)):
            assert np.array_equal(getattr(got, f), a), (name, f)
    words = got.ldpc_codewords[:, None, None, None, None]
    assert (got.ldpc_cw_err <= words).all() and (got.unconverged <= words).all() and (got.iterations >= words).all()
    assert (got.iterations <= words * np.array([m for _, _, m in CODES], np.uint64)).all()
    assert (got.ldpc_info_err <= words * got.ldpc_info_bits[:, None, None, None, :]).all()
    print("%s: per code, of %d words: in error %s, unconverged %s, iterations %s, info-bit errors %s"
          % (name, int(got.ldpc_codewords.sum()) * 8, got.ldpc_cw_err.sum(axis=(0, 1, 2, 3)), got.unconverged.sum(axis=(0, 1, 2, 3)),
             got.iterations.sum(axis=(0, 1, 2, 3)), got.ldpc_info_err.sum(axis=(0, 1, 2, 3))))


def test_the_cases_hold_words_in_error_and_words_without():
    wrong = right = 0
    for name in TT.CASES[:4]:
        got = gpu_profile(name)
        for err, words in ((got.cw_err, got.codewords), (got.ldpc_cw_err, got.ldpc_codewords)):
            wrong += int(err.sum())
            right += int(words.sum()) * 8 * 3 - int(err.sum())
    assert wrong > 0 and right > 0


# ---- 3. and 4. identities by bytes ----

@pytest.mark.parametrize("name", TT.CASES)
def test_tracking_fields_and_soft_bits_are_the_coded_frame_calls(name):
    got, frm = gpu_profile(name), TCF.gpu_profile(name)
    assert TT.same_bits(got[:9], frm[:9]), name
    for f in ("scales", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(got, f), getattr(frm, f)), f
    assert got.sym_rot == frm.sym_rot and np.array_equal(got.info_bits, frm.info_bits) and np.array_equal(got.codewords, frm.codewords)
    assert got.soft_bits.dtype == np.int8 and got.soft_bits.tobytes() == frm.soft_bits.tobytes()


@pytest.mark.parametrize("name", ("n64_wtx_plain", TCF.LONG, TT.OWN))
def test_identities_by_bytes(name):
    c, seed, got = TC.case(name), TC.seed_of(name), gpu_profile(name)
    plain = run_gpu(c, seed, 0, FRAMES)
    assert plain.soft_bits is None and same_counts(plain, got) and TT.same_bits(plain[:9], got[:9])
    again = run_gpu(c, seed, 0, FRAMES, export=True)
    assert np.array_equal(again.soft_bits, got.soft_bits) and same_counts(again, got)
    # one family alone, one code alone
    vit = run_gpu(c, seed, 0, FRAMES, ldpc_codes=())
    assert same_counts(vit, got, fields=VIT) and vit.ldpc_info_err.shape[-1] == 0 and vit.ldpc_codes == ()
    assert TT.same_bits(vit[:9], got[:9])
    ldpc = run_gpu(c, seed, 0, FRAMES, codes=())
    assert same_counts(ldpc, got, fields=LDPC) and ldpc.info_err.shape[-1] == 0 and ldpc.rates == ()
    one = run_gpu(c, seed, 0, FRAMES, codes=(1,), ldpc_codes=CODES[1:2])
    assert same_counts(one, got, (Ellipsis, 0), (Ellipsis, 1))
    # one point or two: the last receiver has a postamble, so alone its word length is the launch's only one
    last = len(c["points"]) - 1
    assert c["tracking"][last].post == 1
    alone = run_gpu(c, seed, 0, FRAMES, c["points"][last:], c["tracking"][last:], sym_rot=got.sym_rot)
    assert same_counts(alone, got, 0, last)
    two = run_gpu(c, seed, 0, FRAMES, [c["points"][last], L(linewidth=0.11)], [c["tracking"][last], TP(1, 0)], sym_rot=got.sym_rot)
    assert same_counts(two, got, 0, last)
    # every point of a call carries the same information: under another rotation the soft bits stay and the counts are its decoders'
    other = run_gpu(c, seed, 0, FRAMES, sym_rot=1, export=True, ldpc_codes=CODES[:1])
    assert other.sym_rot == 1 and np.array_equal(other.soft_bits, got.soft_bits)
    info, cw = viterbi_errs(c, other, R.viterbi_decode_long_gpu, seed)
    assert np.array_equal(other.info_err, info) and np.array_equal(other.cw_err, cw)
    for f, a in zip(LDPC, ldpc_errs(c, other, R.ldpc_decode_gpu, seed)):
        assert np.array_equal(getattr(other, f), a), f


def test_split_frame_ranges_accumulate_to_one_call():
    c, seed = TC.case(TCF.LONG), TC.seed_of(TCF.LONG)
    one = run_gpu(c, seed, 0, 8)
    a = run_gpu(c, seed, 0, 5, ref_frames=(0, 8))
    both = run_gpu(c, seed, 5, 3, ref_frames=(0, 8), out=a)
    for f in VIT + LDPC + ("codewords", "ldpc_codewords", "bit_err", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (one.codewords == 8).all() and one.cw_err.sum() > 0 and one.iterations.sum() > 0
    # the frames 5 ... 7 alone are those frames' words, not the first three's
    late, early = run_gpu(c, seed, 5, 3, ref_frames=(0, 8)), run_gpu(c, seed, 0, 3, ref_frames=(0, 8))
    assert not same_counts(late, early)
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), codes=(0,), out=a)
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), ldpc_codes=CODES[:1], out=a)
    with pytest.raises(ValueError):
        run_gpu(c, seed, 5, 3, ref_frames=(0, 8), sym_rot=3, out=a)


# ---- 5. several words per frame, chunks that end inside a cell ----

def test_several_words_per_frame_and_chunks_that_end_inside_a_cell():
    """N = 1024, 64-QAM, S = 16, cp + cs = 64, two points with a postamble: n_f = 6 x 448 x 14 = 37 632, T = 18 816 and 28 224, W =
    3 words of 12 544.  A chunk of the documented budget -- the history's term included -- ends inside a cell; neither the split of
    the frame range nor another chunking (one point makes a frame smaller; the LDPC codes alone drop the history) changes a counter.
    The first frames' words against the decoders alone on the exported soft bits."""
    st, S, k = W.make_structure("wtx", 1024, 56), 16, 6
    c = RC.make_case(st, k, S, "plain", 3001)
    act = CM.half_band_allocation(1024)
    pil = R.pilot_comb(act, 8)
    n_data = int((act & ~pil).sum())
    n_c = k * n_data
    perm = R.default_interleaver(n_c)
    pts, tps = [L(linewidth=0.01), L(cfo=0.01, cfo_tracked=0)], [TP(1, 1), TP(0, 1)]
    rates, codes = (0, 2), ((4, 8, 6), (4, 16, 10))
    assert n_c * (S - 2) == 37632 and R.ldpc_frame_words(n_c * (S - 2)) == (3, 12544)
    per_chunk = R.rx_profile_coset_chunk_frames(st, k, S, False, 2, False, 1, n_data, rates, post=True)
    assert per_chunk == R.rx_profile_coded_frame_chunk_frames(st, k, S, False, 2, False, 1, n_data, rates, post=True) and per_chunk > 100
    frames = per_chunk // 2 + 19

    def run(f0, n, points=pts, tracking=tps, codes_=rates, **kw):
        return W.rx_profile_coset_gpu(st, k, S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, points, tracking, pil, SCALES,
                                      R.LLR_SCALE, perm, codes_, codes, 128, active=act, **kw)
    one = run(0, frames)
    assert (frames * 8) % per_chunk != 0 and frames % per_chunk != 0 and R.rx_profile_kernel_ms() > 0.0
    assert (one.codewords == frames).all() and (one.ldpc_codewords == 3 * frames).all() and one.iterations.min() >= 3 * frames
    assert one.info_bits.tolist() == [[18816 - 6, 28224 - 6]] * 2 and one.cw_err.sum() > 0
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    assert same_counts(parts, one) and np.array_equal(parts.codewords, one.codewords)
    one_point = R.rx_profile_coset_chunk_frames(st, k, S, False, 1, False, 1, n_data, rates, post=True)
    assert per_chunk < one_point and frames % one_point != 0
    alone = run(0, frames, points=pts[1:], tracking=tps[1:])
    assert same_counts(alone, one, 0, 1)
    no_hist = R.rx_profile_coset_chunk_frames(st, k, S, False, 2, False, 1, n_data, (), post=True)
    assert no_hist == R.rx_profile_ldpc_chunk_frames(st, S, False, 2, False, 1) and per_chunk < no_hist and (frames * 8) % no_hist != 0
    ldpc = run(0, frames, codes_=())
    assert same_counts(ldpc, one, fields=LDPC)
    few = run(0, 2, export=True)
    cc = dict(c, active=act, pilots=pil, perm=perm, tracking=tps)
    info, cw = viterbi_errs(cc, few, R.viterbi_decode_long_gpu, 7000)
    assert np.array_equal(few.info_err, info) and np.array_equal(few.cw_err, cw)
    for f, a in zip(LDPC, ldpc_errs(cc, few, R.ldpc_decode_gpu, 7000)):
        assert np.array_equal(getattr(few, f), a), f


# ---- 6. keys beyond 32 bits ----

def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, the frames 2^32 - 1 and 2^32: the information stream's counter takes both words of the frame
    index and its key both words of the seed -- the mirror's words, drawn with the full values, are what the GPU decoded against;
    with the low words alone they are not"""
    c = TC.case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 1
    got = run_gpu(c, seed, f0, 2, export=True)
    info, cw = viterbi_errs(c, got, R.viterbi_decode_long_gpu, seed, f0)
    assert np.array_equal(got.info_err, info) and np.array_equal(got.cw_err, cw)
    for f, a in zip(LDPC, ldpc_errs(c, got, R.ldpc_decode_gpu, seed, f0)):
        assert np.array_equal(getattr(got, f), a), f
    assert got.cw_err.sum() > 0
    assert not np.array_equal(viterbi_errs(c, got, R.viterbi_decode_long_gpu, seed & 0xFFFFFFFF, f0)[0], got.info_err)
    assert not np.array_equal(viterbi_errs(c, got, R.viterbi_decode_long_gpu, seed, f0 - 2 ** 32)[0], got.info_err)


# ---- 7. without a mirror decoder ----

def test_a_clean_link_counts_nothing():
    st, k, S = W.make_structure("wtx", 64, 8), 2, 6
    c = RC.make_case(st, k, S, "half", 911)
    h = np.zeros_like(c["h"])
    h[:, 0], h[:, 1] = 1.0, (0.3, 0.3j)                                 # |H| >= 0.7 on every bin, the channel inside the prefix
    snr = np.array((30.0, 36.0), np.float32)
    pil = R.pilot_comb(np.asarray(c["active"]) != 0, 8)
    n_c = k * int(((np.asarray(c["active"]) != 0) & ~pil).sum())
    pts, tps = [L(), L()], [TP(0, 0), TP(1, 1)]
    args = (st, k, S, c["w_tx"], c["w_rx"], h, snr, 77, 0, FRAMES, pts, tps, pil, SCALES, R.LLR_SCALE, R.default_interleaver(n_c), RATES,
            ((3, 6, 30), (4, 8, 30)))
    got = W.rx_profile_coset_gpu(*args, active=c["active"], export=True)
    ref = R.rx_profile_coset_host(*args, active=c["active"], with_soft=True)[0]
    taken = np.tile((np.asarray(c["active"]) != 0) & ~pil, (S - 1, 1))
    for i, tp in enumerate(tps):
        use = taken.copy()
        if tp.post:
            use[S - 2] = False
        d, dref = got.soft_bits[:, :, :, :, i][..., use, :k], ref.soft_bits[:, :, :, :, i][..., use, :k]
        assert d.size == dref.size == 8 * FRAMES * use.sum() * k
        assert (d > 0).all() and (np.abs(dref.astype(np.int32)) >= 4).all(), (i, int(d.min()), int(np.abs(dref).min()))
    assert got.info_bits.min() > 100 and got.ldpc_info_bits.min() > 100
    for f in VIT + LDPC[:3]:
        assert not getattr(got, f).any(), f
    assert np.array_equal(got.iterations, np.broadcast_to(got.ldpc_codewords[:, None, None, None, None], got.iterations.shape))
    assert (got.codewords == FRAMES).all() and (got.ldpc_codewords == FRAMES).all()
    vit, ldpc = R.coset_ber(got)
    assert vit.shape == ldpc.shape[:-1] + (3,) and not vit.any() and not ldpc.any() and not any(a.any() for a in R.coset_fer(got))


def test_coset_for_window_file_equals_the_direct_calls(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    pts, tps = [L(), L(cfo=0.02, cfo_tracked=0)], [TP(0, 0), TP(1, 1)]
    codes = ((4, 8), (3, 6, 12))
    gpu = W.coset_for_window_file("wtx", 8, win, h, snr, pts, tps, 4, SCALES, ldpc_codes=codes, gpu=True, **kw)
    assert list(gpu) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    pil = R.pilot_comb(alloc, 4)
    perm = R.default_interleaver(4 * int((alloc & ~pil).sum()))
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want = W.rx_profile_coset_gpu(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, tps, pil, SCALES, R.LLR_SCALE, perm, RATES, codes,
                                      active=alloc, mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g = gpu[name][key]
            assert type(g) is R.RxProfileCoset and g.info_err.shape == (2, 2, 2, 3) and g.ldpc_info_err.shape == (2, 2, 2, 2)
            assert TT.same_bits(g[:9], [a[:, i] for a in want[:9]]), (name, key)
            assert same_counts(g, want, Ellipsis, (slice(None), i))
            assert np.array_equal(g.codewords, want.codewords) and np.array_equal(g.ldpc_info_bits, want.ldpc_info_bits)
            assert g.ldpc_codes == ((4, 8, R.LDPC_MAX_ITER), (3, 6, 12)) and g.rates == RATES
            assert [a.shape for a in R.coset_ber(g)] == [a.shape for a in R.coset_fer(g)] == [(2, 2, 2, 3), (2, 2, 2, 2)]
