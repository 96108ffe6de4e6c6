"""``wofdm_ldpc_harq_decode`` (wofdm_ldpc_harq_kernel with no word to flip by) bit for bit against the integer mirror
``ldpc_harq_decode``: the decisions, the stop round, the iterations over all rounds and the ACK of every word.

Codes and lengths: (3, 6) n = 45 -- Z = 11, a partly filled wave --; (3, 6) n = 120; (4, 8) n = 700 -- Z = 89 --; (6, 24) n = 16 384, two
words -- Z above the 256 threads, the LDS maximum.  Rounds 1, 2, 4 and 8, Chase combining and plain ARQ, a non-identity perm.

The inputs are transmissions of the all-zero word, rint(12 (m_w + N(0, 1))) clamped to +-127, the mean m_w rising from word to word
so that the words need different numbers of rounds.  Every case asserts ON THE MIRROR'S RESULT what its inputs reach (``FULL``: a
stop at every round 1 ... R and words never ACKed; the others: ACKed words beside unACKed ones or beside later ACKs), so that no comparison
passes on words that all stop alike."""
import functools

import numpy as np
import pytest

from wofdm_amd import rx_profile as R

pytestmark = pytest.mark.gpu

#: name: (J, L, n, max_iter, words, seed)
CODES = {"n45": (3, 6, 45, 8, 64, 2), "n120": (3, 6, 120, 8, 64, 1), "n700": (4, 8, 700, 10, 32, 4)}
ROUNDS = (1, 2, 4, 8)
#: the means' range per rule: combining gains with every round, plain ARQ draws each round anew
MEANS = {True: (0.25, 1.5), False: (0.75, 1.1)}
ARQ_N700 = (0.9, 1.5)                    # (the longer code's waterfall is steeper: a wider range for its words to differ)
#: the cases whose mirror stops at every round 1 ... R, for each R of ROUNDS, and leaves words unACKed
FULL = {("n45", True), ("n120", True), ("n700", True), ("n120", False)}


def rows(n_cw, rounds, n, seed, lo, hi, gain=12.0):
    rs = np.random.RandomState(seed)
    mean = np.linspace(lo, hi, n_cw)[:, None, None]
    return np.clip(np.rint(gain * (mean + rs.standard_normal((n_cw, rounds, n)))), -127, 127).astype(np.int8)


@functools.lru_cache(maxsize=None)
def reference(name, rounds, combine):
    """(soft, the mirror's (bits, round, iters, converged)); computed once, not to be modified"""
    J, L, n, max_iter, n_cw, seed = CODES[name]
    soft = rows(n_cw, rounds, n, seed, *(ARQ_N700 if (name, combine) == ("n700", False) else MEANS[combine]))
    return soft, R.ldpc_harq_decode(soft, J, L, max_iter, combine)


def same(got, ref):
    return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, ref))


@pytest.mark.parametrize("combine", (True, False))
@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("name", sorted(CODES))
def test_the_decoder_is_the_mirror(name, rounds, combine):
    J, L, n, max_iter = CODES[name][:4]
    soft, ref = reference(name, rounds, combine)
    _, rnd, iters, conv = ref
    stops = set(rnd[conv].tolist())
    print("%s R=%d combine=%d: ACKed per round %s, unACKed %d" % (name, rounds, combine, np.bincount(rnd[conv], minlength=rounds + 1)[1:],
                                                                   (~conv).sum()))
    if (name, combine) in FULL:
        assert stops == set(range(1, rounds + 1)) and (~conv).any()
    else:
        assert conv.any() and ((~conv).any() or len(stops) > 1)
    assert same(R.ldpc_harq_decode_gpu(soft, J, L, max_iter, combine), ref)
    assert (iters[~conv] == rounds * max_iter).all() and (rnd[~conv] == rounds).all()


@pytest.mark.parametrize("combine", (True, False))
def test_a_non_identity_perm(combine):
    J, L, n, max_iter = CODES["n120"][:4]
    soft, ref = reference("n120", 4, combine)
    perm = np.random.RandomState(3).permutation(n)
    scattered = np.zeros_like(soft)
    scattered[:, :, perm] = soft                                       # variable c is read at perm[c]
    assert same(R.ldpc_harq_decode_gpu(scattered, J, L, max_iter, combine, perm), ref)
    assert same(R.ldpc_harq_decode(scattered, J, L, max_iter, combine, perm), ref)
    assert not same(R.ldpc_harq_decode_gpu(scattered, J, L, max_iter, combine), ref)


def test_the_largest_code_two_words():
    """(6, 24) over 16 384 positions: Z = 691 above the workgroup's 256 threads, the decoder's LDS at its maximum; one word is
    ACKed in an early round, the other runs all four"""
    soft = rows(2, 4, 16384, 7, 0.45, 1.3)
    for combine in (True, False):
        ref = R.ldpc_harq_decode(soft, 6, 24, 6, combine)
        assert same(R.ldpc_harq_decode_gpu(soft, 6, 24, 6, combine), ref)
        if combine:
            assert ref[3].tolist() == [False, True] and ref[1][0] == 4 and ref[1][1] < 4 and ref[2][0] == 24
    assert R.ldpc_lift(6, 24, 16384) == 691


def test_runs_at_the_ends_of_the_range_reach_the_clamp():
    """rows of +127 / +127 whose int8 sum would wrap, and rows that contain -128: the sums are int32 and clamp to +-127"""
    J, L, n, max_iter = CODES["n120"][:4]
    base = rows(24, 4, n, 12, 0.3, 1.2)
    hot = base.copy()
    hot[:, :, 10:50] = np.where(base[:, :, 10:50] > 0, 127, -128)
    hot[:, 1::2, 60:70] = -128
    hot[:, :, 70:80] = 127
    assert (hot == -128).any() and (hot.astype(np.int32).sum(axis=1) > 254).any() and (hot.astype(np.int32).sum(axis=1) < -256).any()
    for combine in (True, False):
        for rounds in (1, 2, 4):
            ref = R.ldpc_harq_decode(hot[:, :rounds], J, L, max_iter, combine)
            assert same(R.ldpc_harq_decode_gpu(hot[:, :rounds], J, L, max_iter, combine), ref), (combine, rounds)
    ref = R.ldpc_harq_decode(hot, J, L, max_iter, True)
    assert ref[3].any() and not ref[3].all()
    # one round of in-range rows is wofdm_ldpc_decode
    one = R.ldpc_harq_decode_gpu(base[:, :1], J, L, max_iter)
    b, it, cv = R.ldpc_decode_gpu(base[:, 0], J, L, max_iter)
    assert np.array_equal(one[0], b) and np.array_equal(one[2], it) and np.array_equal(one[3], cv) and (one[1] == 1).all()
