"""``wofdm_rx_profile_harq`` on the GPU (wofdm_rxprof_coded_kernel<N> as it is; behind it wofdm_ldpc_harq_kernel, which draws the
words of a group's first frame, encodes them once and decodes round by round on the combined soft bits).

Shape: N = 64, 16-QAM, S = 6, 2 pairs x 2 SNR points x 2 channels, 8 frames per cell, the codes (3, 6) x 5 and (4, 8) x 30, two
points of which one has a postamble, R = 2 and 4.  The SNR points, 14 and 22 dB, are where the host route finds ACKs beside words
never ACKed at both R; the test asserts it on the GPU's counters.

1. harq_errs equals ``wofdm_ldpc_harq_decode`` (and the numpy mirror) on the call's own exported soft bits, gathered through the
   frame interleaver and flipped by ``coset_codewords`` of each group's FIRST frame -- all 13 fields, by bytes.
2. At R = 1 it is the documented mapping of ``wofdm_rx_profile_coset``'s LDPC counters.
3. The tracking fields and the soft bits are ``wofdm_rx_profile_coded_frame``'s bytes.
4. The counters with and without export, one point or two, one code or two, from a repeated call, over frame ranges split at a
   multiple of R.
5. N = 256 with frames just over ``rx_profile_harq_chunk_frames``: a chunk ends inside a cell, at a multiple of R = 3.
6. R = 3 from frame 2^32 - 1: the group straddles a frame index of 2^32; its words are those of frame 2^32 - 1 under the full
   64-bit index and seed."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC

pytestmark = pytest.mark.gpu

L, TP = R.LinkPoint, R.TrackingPoint
SCALES = (0.5,)
CODES = ((3, 6, 5), (4, 8, 30))
FRAMES, SEED = 8, 4711
FIELDS = ("acked", "unacked", "word_err", "undetected", "info_err", "iterations")


@functools.lru_cache(maxsize=None)
def case(n_fft=64, S=6):
    st = W.make_structure("CPW", n_fft, n_fft // 8)
    c = RC.make_case(st, 4, S, "plain", 43)
    pil = R.pilot_comb(np.ones(n_fft, bool), 8)
    n_c = 4 * int((~pil).sum())
    c.update(snr=np.array((14.0, 22.0), np.float32), pilots=pil, perm=R.default_interleaver(n_c), n_c=n_c,
             points=[L(), L(cfo=0.01, cfo_tracked=0)], tracking=[TP(0, 0), TP(1, 1)])
    return c


def run(rounds, combine=True, f0=0, frames=FRAMES, c=None, seed=SEED, points=None, tracking=None, codes=CODES, entry=None, cells=None, **kw):
    c = case() if c is None else c
    w_tx, w_rx, h, snr = c["w_tx"], c["w_rx"], c["h"], c["snr"]
    if cells == 1:
        w_tx, w_rx, h, snr = w_tx[:1], w_rx[:1], h[:1], np.array((10.0,), np.float32)   # (the host route: ACKs at round 3, failures)
    head = (c["st"], c["k"], c["S"], w_tx, w_rx, h, snr, seed, f0, frames, c["points"] if points is None else points,
            c["tracking"] if tracking is None else tracking, c["pilots"], SCALES, R.LLR_SCALE, c["perm"])
    side = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], **kw)
    if entry is not None:
        return entry(head, side)
    return W.rx_profile_harq_gpu(*head, codes, side.pop("sym_rot", None), rounds, combine, **side)


@functools.lru_cache(maxsize=None)
def gpu_profile(rounds, combine=True):
    return run(rounds, combine, export=True)


def same_counts(a, b, ia=Ellipsis, ib=Ellipsis, ca=None, cb=None):
    """the counters of a (points ia, code ca) are b's (points ib, code cb)"""
    def of(p, f, i, code):
        x = getattr(p, f)[i]
        return x if code is None else (x[..., code, :] if f == "acked" else x[..., code])
    return all(np.array_equal(of(a, f, ia, ca), of(b, f, ib, cb)) for f in FIELDS)


def counters(prof):
    return np.concatenate([prof.acked] + [getattr(prof, f)[..., None] for f in FIELDS[1:]], axis=-1)


def errs_of_soft_bits(prof, c, seed, f0, decode, tracking=None):
    """harq_errs [points, pairs, n_snr, n_ch, codes, 13] from the call's exported soft bits through ``decode(soft [n_cw, R, n], J, L,
    max_iter, combine)``: every group's rows gathered by ``frame_codewords`` and flipped by the words of the group's first frame"""
    tps = c["tracking"] if tracking is None else tracking
    rounds = prof.rounds
    pos = R._code_prepare(c["st"], c["k"], c["active"], c["pilots"], (2,), c["perm"], R.LLR_SCALE)[2]
    out = np.zeros(prof.unacked.shape + (_lib.HARQ_FIELDS,), np.uint64)
    for i, tp in enumerate(tps):
        soft = R.frame_codewords(prof.soft_bits[:, :, :, :, i], tp.post, pos, c["perm"], prof.sym_rot).astype(np.int16)
        lead, n_f = soft.shape[:3], soft.shape[-1]
        groups = soft.shape[3] // rounds
        n_words, n = R.ldpc_frame_words(n_f)
        assert prof.words[i] == n_words * groups and prof.word_bits[i] == n and prof.frame_words[i] == n_words
        for j, (J, Lc, m) in enumerate(prof.codes):
            d = np.zeros(lead + (groups, n_words, rounds, n), np.int8)
            x = np.zeros(lead + (groups, n_words, n), np.uint8)
            for p, s, ch, g in np.ndindex(*lead, groups):
                cell = (p * lead[1] + s) * lead[2] + ch
                xl = R.coset_codewords(seed, cell, f0 + g * rounds, n_f, (), ((J, Lc, m),))[1][0, :n_words * n]
                rows = soft[p, s, ch, g * rounds:(g + 1) * rounds, :n_words * n]
                d[p, s, ch, g] = np.where(xl != 0, -rows, rows).reshape(rounds, n_words, n).transpose(1, 0, 2)
                x[p, s, ch, g] = xl.reshape(n_words, n)
            bits, rnd, iters, conv = decode(d.reshape(-1, rounds, n), J, Lc, m, bool(prof.combine))
            k0 = J * R.ldpc_lift(J, Lc, n)
            assert prof.info_bits[i, j] == n - k0
            shape = lead + (groups * n_words,)
            wrong = (bits ^ x.reshape(-1, n))[:, k0:]
            bad, rnd, iters, conv = wrong.any(axis=1).reshape(shape), rnd.reshape(shape), iters.reshape(shape), conv.reshape(shape)
            for r in range(rounds):
                out[i, :, :, :, j, r] = (conv & (rnd == r + 1)).sum(axis=-1)
            out[i, :, :, :, j, 8] = (~conv).sum(axis=-1)
            out[i, :, :, :, j, 9] = bad.sum(axis=-1)
            out[i, :, :, :, j, 10] = (bad & conv).sum(axis=-1)
            out[i, :, :, :, j, 11] = wrong.sum(axis=1).reshape(shape).sum(axis=-1)
            out[i, :, :, :, j, 12] = iters.sum(axis=-1)
    return out


@pytest.mark.parametrize("combine", (True, False))
@pytest.mark.parametrize("rounds", (2, 4))
def test_harq_errs_are_the_decoder_on_the_flipped_soft_bits(rounds, combine):
    c, got = case(), gpu_profile(rounds, combine)
    assert type(got) is R.RxProfileHarq and got.rounds == rounds and got.combine == int(combine) and got.codes == CODES
    assert got.acked.shape == (2, RC.PAIRS, 2, RC.N_CH, 2, 8) and got.unacked.shape == (2, RC.PAIRS, 2, RC.N_CH, 2)
    assert got.words.tolist() == [FRAMES // rounds] * 2 and not got.acked[..., rounds:].any()
    print("R=%d combine=%d: ACKed per round %s, unACKed %s, undetected %s, iterations %s"
          % (rounds, combine, got.acked.sum(axis=(0, 1, 2, 3))[:, :rounds].tolist(), got.unacked.sum(axis=(0, 1, 2, 3)),
             got.undetected.sum(axis=(0, 1, 2, 3)), got.iterations.sum(axis=(0, 1, 2, 3))))
    assert np.array_equal(got.acked.sum(axis=-1) + got.unacked, np.broadcast_to(got.words[:, None, None, None, None], got.unacked.shape))
    assert (got.undetected <= got.word_err).all() and (got.word_err <= got.words[:, None, None, None, None]).all()
    for decode in (R.ldpc_harq_decode_gpu, R.ldpc_harq_decode):
        assert np.array_equal(counters(got), errs_of_soft_bits(got, c, SEED, 0, decode)), decode.__name__
    if combine:
        assert got.acked.sum() > 0 and got.unacked.sum() > 0           # both ACKs and failures at these SNR points


def test_combining_acks_words_that_plain_arq_does_not():
    chase, arq = gpu_profile(4, True), gpu_profile(4, False)
    assert chase.acked.sum() > arq.acked.sum() and np.array_equal(chase.acked[..., 0], arq.acked[..., 0])


def test_one_round_is_the_coset_calls_counters():
    got = run(1)
    cos = run(1, entry=lambda head, side: W.rx_profile_coset_gpu(*head, (), CODES, None, **side))
    words = cos.ldpc_codewords[:, None, None, None, None]
    assert (got.words == FRAMES).all() and np.array_equal(got.words, cos.ldpc_codewords)
    assert np.array_equal(got.acked[..., 0], words - cos.unconverged) and not got.acked[..., 1:].any()
    assert np.array_equal(got.unacked, cos.unconverged) and np.array_equal(got.word_err, cos.ldpc_cw_err)
    assert np.array_equal(got.info_err, cos.ldpc_info_err) and np.array_equal(got.iterations, cos.iterations)
    assert same_counts(run(1, combine=False), got)


def test_tracking_fields_and_soft_bits_are_the_coded_frame_calls():
    got = gpu_profile(4)
    frm = run(4, entry=lambda head, side: W.rx_profile_coded_frame_gpu(*head, (0,), got.sym_rot, export=True, **side))
    for a, b in zip(got[:9], frm[:9]):
        assert a.tobytes() == b.tobytes()
    for f in ("scales", "decisions", "decisions_sym"):
        assert np.array_equal(getattr(got, f), getattr(frm, f)), f
    assert got.soft_bits.dtype == np.int8 and got.soft_bits.tobytes() == frm.soft_bits.tobytes()
    assert gpu_profile(2).soft_bits.tobytes() == got.soft_bits.tobytes() and gpu_profile(4, False).soft_bits.tobytes() == got.soft_bits.tobytes()


@pytest.mark.parametrize("rounds", (2, 4))
def test_identities_by_bytes(rounds):
    c, got = case(), gpu_profile(rounds)
    plain = run(rounds)
    assert plain.soft_bits is None and same_counts(plain, got) and all(a.tobytes() == b.tobytes() for a, b in zip(plain[:9], got[:9]))
    again = run(rounds, export=True)
    assert np.array_equal(again.soft_bits, got.soft_bits) and same_counts(again, got)
    one = run(rounds, codes=CODES[1:])
    assert same_counts(one, got, ca=0, cb=1) and not same_counts(one, got, ca=0, cb=0)
    alone = run(rounds, points=c["points"][1:], tracking=c["tracking"][1:], sym_rot=got.sym_rot)
    assert same_counts(alone, got, 0, 1)
    # frame ranges split at a multiple of R add up; the later range's words are its own groups'
    a = run(rounds, f0=0, frames=FRAMES - rounds)
    both = run(rounds, f0=FRAMES - rounds, frames=rounds, out=a)
    assert same_counts(both, got) and np.array_equal(both.words, got.words) and np.array_equal(both.bit_err, got.bit_err)
    with pytest.raises(ValueError):
        run(rounds, f0=1, frames=rounds)
    with pytest.raises(ValueError):
        run(rounds, f0=0, frames=rounds + 1)
    with pytest.raises(ValueError):
        run(rounds, f0=FRAMES - rounds, frames=rounds, out=run(rounds, combine=False, frames=FRAMES - rounds))


def test_a_chunk_that_ends_inside_a_cell():
    """N = 256, S = 3, one cell, R = 3: the frames are one group more than a chunk holds, so the first chunk ends inside the cell
    -- at a multiple of R --; the call over all frames is the two ranges' sum, and a one-point call (another chunking) agrees"""
    c = case(256, 3)
    codes = ((4, 8, 10),)
    per_chunk = R.rx_profile_harq_chunk_frames(c["st"], 3, False, 2, False, 1, 3)
    base = R.rx_profile_ldpc_chunk_frames(c["st"], 3, False, 2, False, 1)
    assert per_chunk == base // 3 * 3 and 1000 < per_chunk < 65535 and per_chunk % 3 == 0
    frames = per_chunk + 3
    one = run(3, frames=frames, c=c, cells=1, codes=codes)
    assert R.rx_profile_kernel_ms() > 0.0 and (one.words == frames // 3).all()
    parts = run(3, f0=per_chunk, frames=3, c=c, cells=1, codes=codes, out=run(3, frames=per_chunk, c=c, cells=1, codes=codes))
    assert same_counts(parts, one) and np.array_equal(parts.words, one.words)
    assert one.acked.sum() > 0 and one.unacked.sum() > 0
    alone = run(3, frames=frames, c=c, cells=1, codes=codes, points=c["points"][1:], tracking=c["tracking"][1:], sym_rot=one.sym_rot)
    assert R.rx_profile_harq_chunk_frames(c["st"], 3, False, 1, False, 1, 3) > frames and same_counts(alone, one, 0, 1)


def test_a_group_that_straddles_a_frame_index_of_2_to_the_32():
    c, seed, f0 = case(), 0x9E3779B97F4A7C15, 2 ** 32 - 1
    assert f0 % 3 == 0
    got = run(3, f0=f0, frames=6, seed=seed, export=True)
    assert np.array_equal(counters(got), errs_of_soft_bits(got, c, seed, f0, R.ldpc_harq_decode_gpu))
    assert got.acked.sum() > 0
    # the words are the first frames' -- 2^32 - 1 and 2^32 + 2 -- under the full seed: not another frame's, not the low word's
    for other in ((seed & 0xFFFFFFFF, f0), (seed, f0 + 1), (seed, f0 - 3)):
        assert not np.array_equal(counters(got), errs_of_soft_bits(got, c, *other, R.ldpc_harq_decode_gpu)), other
