"""Retransmissions with soft combining without a GPU: the integer mirror ``ldpc_harq_decode`` against ``ldpc_decode`` round by
round, the host route ``rx_profile_harq_host`` against ``rx_profile_coset_host`` at one round, and the views on a hand-made
counter array.  include/wofdm.h has the scheme."""
import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC

J, L, N, MAX_ITER = 3, 6, 120, 8
#: the host route's SNR points (QPSK over the faded channels): words fail and words decode at both
SNR = np.array((4.0, 12.0), np.float32)


def noisy_rows(n_cw, rounds, n, seed, gain=12.0, mean=0.8):
    """transmissions of the all-zero word: rint(gain (mean + N(0, 1))) clamped to +-127, [n_cw, rounds, n] int8"""
    rs = np.random.RandomState(seed)
    return np.clip(np.rint(gain * (mean + rs.standard_normal((n_cw, rounds, n)))), -127, 127).astype(np.int8)


def test_the_symbols_exist():
    assert _lib.HARQ_MAX_ROUNDS == 8 and _lib.HARQ_FIELDS == 13
    for name in ("wofdm_ldpc_harq_decode", "wofdm_rx_profile_harq"):
        assert name in _lib.EXPORTS
    for name in ("ldpc_harq_decode", "ldpc_harq_decode_gpu", "rx_profile_harq_gpu", "rx_profile_harq_host", "rx_profile_harq_chunk_frames",
                 "RxProfileHarq", "harq_acked", "harq_mean_transmissions", "harq_residual_fer", "harq_undetected", "harq_goodput",
                 "harq_bits_per_sample", "harq_for_window_file"):
        assert hasattr(W, name), name


@pytest.mark.parametrize("combine", (True, False))
def test_one_round_is_ldpc_decode(combine):
    soft = noisy_rows(24, 1, N, 1, mean=1.2)
    bits, rnd, iters, conv = R.ldpc_harq_decode(soft, J, L, MAX_ITER, combine)
    b, it, cv = R.ldpc_decode(soft[:, 0], J, L, MAX_ITER)
    assert np.array_equal(bits, b) and np.array_equal(iters, it) and np.array_equal(conv, cv) and (rnd == 1).all()
    assert cv.any() and not cv.all()
    assert bits.dtype == np.uint8 and rnd.dtype == iters.dtype == np.int32 and conv.dtype == bool
    perm = np.random.RandomState(2).permutation(N)
    for a, b_ in zip(R.ldpc_harq_decode(soft, J, L, MAX_ITER, combine, perm)[::2], R.ldpc_decode(soft[:, 0], J, L, MAX_ITER, perm)[:2]):
        assert np.array_equal(a, b_)
    # a word of [rounds, n] is one word
    one = R.ldpc_harq_decode(soft[3], J, L, MAX_ITER, combine)
    assert one[0].shape == (1, N) and np.array_equal(one[0][0], bits[3])


def test_the_words_stop_at_every_round_and_some_never():
    soft = noisy_rows(48, 4, N, 6)
    bits, rnd, iters, conv = R.ldpc_harq_decode(soft, J, L, MAX_ITER)
    assert set(rnd[conv].tolist()) == {1, 2, 3, 4} and (~conv).any() and (rnd[~conv] == 4).all()
    # round by round by the definition: the clamped int32 sum of the rows so far, decoded afresh
    for w in range(soft.shape[0]):
        total = 0
        for r in range(4):
            q = np.clip(soft[w, :r + 1].astype(np.int32).sum(axis=0), -127, 127)
            b, it, cv = R.ldpc_decode(q[None], J, L, MAX_ITER)
            total += int(it[0])
            if cv[0] or r == 3:
                break
        assert (rnd[w], iters[w], bool(conv[w])) == (r + 1, total, bool(cv[0])) and np.array_equal(bits[w], b[0]), w
    # a word that never converges ran max_iter in every round
    assert (iters[~conv] == 4 * MAX_ITER).all()


@pytest.mark.parametrize("combine", (True, False))
def test_an_acked_word_ignores_its_later_rows(combine):
    soft = noisy_rows(48, 4, N, 6, mean=0.8 if combine else 1.0)
    ref = R.ldpc_harq_decode(soft, J, L, MAX_ITER, combine)
    junk = soft.copy()
    garbage = np.random.RandomState(9).randint(-128, 128, soft.shape).astype(np.int8)
    for w in range(soft.shape[0]):
        if ref[3][w]:
            junk[w, ref[1][w]:] = garbage[w, ref[1][w]:]
    assert (ref[3] & (ref[1] < 4)).sum() > 5 and not np.array_equal(junk, soft)
    for a, b in zip(R.ldpc_harq_decode(junk, J, L, MAX_ITER, combine), ref):
        assert np.array_equal(a, b)


def test_plain_arq_decodes_each_row_alone():
    soft = noisy_rows(48, 4, N, 5, mean=1.0)
    bits, rnd, iters, conv = R.ldpc_harq_decode(soft, J, L, MAX_ITER, combine=False)
    rows = [R.ldpc_decode(soft[:, r], J, L, MAX_ITER) for r in range(4)]
    assert len(set(rnd[conv].tolist())) >= 3 and (~conv).any()
    for w in range(soft.shape[0]):
        stop = rnd[w] - 1
        assert all(not rows[r][2][w] for r in range(stop)) and bool(rows[stop][2][w]) == bool(conv[w])
        assert np.array_equal(bits[w], rows[stop][0][w]) and iters[w] == sum(int(rows[r][1][w]) for r in range(stop + 1))
    # combining never needs more rounds on these words than it took the sum to converge
    assert not np.array_equal(R.ldpc_harq_decode(soft, J, L, MAX_ITER, combine=True)[1], rnd)


def test_sums_are_formed_wider_than_int8_and_clamp_at_127():
    n = N
    rs = np.random.RandomState(11)
    base = noisy_rows(6, 1, n, 12)[:, 0]
    # two rows of +127 where an int8 sum would wrap to -2: the sum must act as +127
    soft = np.stack([np.where(base > 0, 127, base), np.where(base > 0, 127, 0)], axis=1).astype(np.int8)
    want = np.clip(soft.astype(np.int32).sum(axis=1), -127, 127)
    assert (want == 127).any() and ((soft[:, 0].astype(np.int8) + soft[:, 1].astype(np.int8)).astype(np.int8) < 0).any()
    got = R.ldpc_harq_decode(soft, J, L, 64)
    first = R.ldpc_decode(soft[:, 0], J, L, 64)
    second = R.ldpc_decode(want.astype(np.int16), J, L, 64)
    for w in range(6):
        src = first if first[2][w] else second
        assert np.array_equal(got[0][w], src[0][w]) and got[1][w] == (1 if first[2][w] else 2)
    # rows that contain -128: alone they clamp to -127, two of them as well
    low = np.full((4, 2, n), -128, dtype=np.int8)
    low[:, :, ::3] = rs.randint(-128, 128, (4, 2, n))[:, :, ::3]
    for combine in (True, False):
        got = R.ldpc_harq_decode(low, J, L, MAX_ITER, combine)
        for w in range(4):
            q0 = np.clip(low[w, 0].astype(np.int32), -127, 127)
            q1 = np.clip(low[w].astype(np.int32).sum(axis=0) if combine else low[w, 1].astype(np.int32), -127, 127)
            a, b = R.ldpc_decode(q0[None], J, L, MAX_ITER), R.ldpc_decode(q1[None], J, L, MAX_ITER)
            src = a if a[2][0] else b
            assert np.array_equal(got[0][w], src[0][0]) and got[3][w] == src[2][0]
            assert q0.min() == -127 and q1.min() == -127


def test_the_mirror_checks_its_arguments():
    with pytest.raises(ValueError):
        R.ldpc_harq_decode(np.zeros((1, 9, N), np.int8), J, L)
    with pytest.raises(ValueError):
        R.ldpc_harq_decode(np.zeros((1, 2, N), np.int8), J, L, combine=2)
    with pytest.raises(ValueError):
        R.rx_profile_harq_chunk_frames(W.make_structure("CPW", 64, 8), 6, False, 1, False, 1, 0)


def _small_case():
    st = W.make_structure("CPW", 64, 8)
    c = RC.make_case(st, 2, 4, "plain", 41)
    pil = R.pilot_comb(np.ones(64, bool), 8)
    return st, c, pil


def test_one_round_maps_onto_the_coset_hosts_counters():
    st, c, pil = _small_case()
    codes = ((3, 6, 5), (4, 8, 30))
    pts, tps = [R.LinkPoint(), R.LinkPoint(cfo=0.01, cfo_tracked=0)], [R.TrackingPoint(0, 0), R.TrackingPoint(1, 1)]
    args = (st, 2, 4, c["w_tx"][:1], c["w_rx"][:1], c["h"], SNR, 5, 6, 3, pts, tps, pil, (0.5,), R.LLR_SCALE, None)
    cos = R.rx_profile_coset_host(*args, (), codes, None)
    got = R.rx_profile_harq_host(*args, codes, None, 1, True)
    assert type(got) is R.RxProfileHarq and got.rounds == 1 and got.combine == 1 and got.codes == codes
    words = cos.ldpc_codewords[:, None, None, None, None]
    assert np.array_equal(got.words, cos.ldpc_codewords) and np.array_equal(got.info_bits, cos.ldpc_info_bits)
    assert np.array_equal(got.acked[..., 0], words - cos.unconverged) and not got.acked[..., 1:].any()
    assert np.array_equal(got.unacked, cos.unconverged) and np.array_equal(got.word_err, cos.ldpc_cw_err)
    assert np.array_equal(got.info_err, cos.ldpc_info_err) and np.array_equal(got.iterations, cos.iterations)
    assert (got.undetected <= got.word_err).all() and got.unacked.sum() > 0 and got.acked.sum() > 0
    for a, b in zip(got[:9], cos[:9]):
        assert np.array_equal(a, b)
    # plain ARQ at one round is the same call
    arq = R.rx_profile_harq_host(*args, codes, None, 1, False)
    assert all(np.array_equal(getattr(arq, f), getattr(got, f)) for f in ("acked", "unacked", "word_err", "info_err", "iterations"))
    # groups: the frames and the first frame are multiples of the rounds
    with pytest.raises(ValueError):
        R.rx_profile_harq_host(*args[:8], 6, 3, *args[10:], codes, None, 2, True)
    with pytest.raises(ValueError):
        R.rx_profile_harq_host(*args[:8], 5, 2, *args[10:], codes, None, 2, True)


def test_two_rounds_combine_the_groups_frames():
    st, c, pil = _small_case()
    codes = ((3, 6, 5),)
    args = (st, 2, 4, c["w_tx"][:1], c["w_rx"][:1], c["h"][:1], SNR[1:], 5, 6, 4, None, None, pil, (0.5,), R.LLR_SCALE, None)
    two = R.rx_profile_harq_host(*args, codes, None, 2, True)
    one = R.rx_profile_harq_host(*args, codes, None, 1, True)
    assert (two.words == 2).all() and (one.words == 4).all()
    assert np.array_equal(two.acked.sum(axis=-1) + two.unacked, np.full(two.unacked.shape, 2, np.uint64))
    # a group's first transmission is the one-round call's frame: what it ACKs at round 1, that call ACKs among its frames
    assert (two.acked[..., 0] <= one.acked[..., 0]).all()
    for a, b in zip(two[:9], one[:9]):
        assert np.array_equal(a, b)


def hand_made():
    """two points x one cell x two codes, R = 4: 20 words each"""
    herr = np.zeros((2, 1, 1, 1, 2, 13), np.uint64)
    herr[0, ..., 0, :] = [10, 4, 2, 1, 0, 0, 0, 0, 3, 4, 1, 37, 500]
    herr[0, ..., 1, :] = [0, 0, 0, 0, 0, 0, 0, 0, 20, 20, 0, 900, 2400]
    herr[1, ..., 0, :] = [20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 20]
    herr[1, ..., 1, :] = [0, 0, 0, 20, 0, 0, 0, 0, 0, 0, 0, 0, 700]
    trk = [None] * len(R.RxProfileTracking._fields)
    K = np.array([[60, 40], [50, 30]], np.int64)
    return R._harq_result(trk, herr, K, np.array([2, 2], np.int64), np.array([120, 100], np.int64), 40, ((3, 6, 8), (4, 6, 8)), 4, 1,
                          0.25, 0, None)


def test_the_views_on_a_hand_made_counter_array():
    p = hand_made()
    assert p.words.tolist() == [20, 20] and p.acked.shape == (2, 1, 1, 1, 2, 8) and p.unacked.shape == (2, 1, 1, 1, 2)
    cdf = R.harq_acked(p)
    assert cdf.shape == (2, 1, 1, 1, 2, 4)
    assert np.allclose(cdf[0, 0, 0, 0, 0], [0.5, 0.7, 0.8, 0.85]) and np.allclose(cdf[0, 0, 0, 0, 1], 0.0)
    assert np.allclose(cdf[1, 0, 0, 0, 0], 1.0) and np.allclose(cdf[1, 0, 0, 0, 1], [0, 0, 0, 1])
    mt = R.harq_mean_transmissions(p)
    assert np.allclose(mt[:, 0, 0, 0], [[(10 + 8 + 6 + 4 + 12) / 20.0, 4.0], [1.0, 4.0]])
    assert np.allclose(R.harq_residual_fer(p)[:, 0, 0, 0], [[4 / 20.0, 1.0], [0.0, 0.0]])
    assert np.allclose(R.harq_undetected(p)[:, 0, 0, 0], [[1 / 20.0, 0.0], [0.0, 0.0]])
    gp = R.harq_goodput(p)
    assert np.allclose(gp[:, 0, 0, 0], [[60 * 16 / (120 * 40.0), 0.0], [50 * 20 / (100 * 20.0), 30 * 20 / (100 * 80.0)]])
    # per on-air sample: W n coded bits in S symbols of B samples
    bps = R.harq_bits_per_sample(p, 16, 80)
    assert np.allclose(bps[:, 0, 0, 0], gp[:, 0, 0, 0] * np.array([[240.0], [200.0]]) / (16 * 80))
    # a point that carries no word: NaN, not a division by zero
    q = p._replace(words=np.array([20, 0], np.uint64), acked=p.acked * np.array([1, 0], np.uint64).reshape(2, 1, 1, 1, 1, 1),
                   unacked=p.unacked * np.array([1, 0], np.uint64).reshape(2, 1, 1, 1, 1))
    assert np.isnan(R.harq_goodput(q)[1]).all() and np.isnan(R.harq_mean_transmissions(q)[1]).all() and np.isfinite(R.harq_goodput(q)[0]).all()


def test_chunk_frames_is_the_ldpc_calls_rounded_down():
    st = W.make_structure("CPW", 256, 32)
    base = R.rx_profile_ldpc_chunk_frames(st, 16, False, 2, False, 1)
    for rounds in range(1, 9):
        got = R.rx_profile_harq_chunk_frames(st, 16, False, 2, False, 1, rounds)
        assert got == base // rounds * rounds and got % rounds == 0 and 0 < got <= base
    big = W.make_structure("wtx", 1024, 56)
    assert R.rx_profile_harq_chunk_frames(big, 64, True, 16, True, 16, 8) % 8 == 0
