"""The information stream and the coset view without a GPU: ``wofdm_coset_info`` (host only) against ``rx_profile.coset_info`` and
against the stream's definition written out on ``_stream``; stream 4 against streams 0 ... 3; both encoder mirrors through their
decoder mirrors; and the effect the coset view exists to show.

The effect.  A soft word s, as the all-zero view sees it, reaches a decoder in the coset view as d' = x ? -s : s, x the transmitted
word of a random information word u.  A decoder that treated 0 and 1 alike would decode d' to (what it decodes s to) XOR u, so
both views would count the same errors.  Ours break ties and zeros towards 0: the Viterbi survivor is p0 unless p1 is STRICTLY
smaller, the min-sum decoder takes t = 0 as positive and decides x = (Q < 0).
  * On s = 0 (every metric tied, every Q zero) both decoders return the all-zero word in either view: the all-zero view counts
    nothing, the coset view counts the weight of u.  On +-1 words (ties, no zero) and on the words of a low-SNR cell at llr_scale
    0.25 (a third of the soft bits 0) the views differ as well, the all-zero view being the flattering one.
  * On words without zeros and without ties the two views count the same.  The Viterbi words are noisy ones, checked by a forward
    pass written out here (``tie_on_the_path``: c0 = c1 at a state of the decoded path -- the metrics do not depend on how a tie is
    broken, and the traceback reads no other decision).  In the min-sum decoder t = Q - R is zero now and then on any noisy
    word, so the LDPC words are built to have none: another codeword's strong soft bits (|d| >= 101) with a few weak errors (|d| <=
    5), no two of them in one check -- every t is then a soft bit itself or >= 101 - 3 in magnitude, and one iteration ends it.
    Their count is the other codeword's weight on the information bits, in both views."""
import ctypes as C

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import rx_profile as R

SEEDS = (1, 0x9E3779B97F4A7C15, 0xFFFFFFFF00000001)
FRAMES = (0, 5, 2 ** 32 - 1, 2 ** 32, 0x123456789A)
CELLS = (0, 7, 70001, 2 ** 28 - 1)
N_BITS = (1, 127, 128, 129, 4097)


def lib_info(seed, cell, frame, n_bits):
    bits = np.full(max(n_bits, 1) + 3, 9, np.uint8)
    rc = _lib.load().wofdm_coset_info(C.c_uint64(seed), C.c_uint32(cell), C.c_uint64(frame), n_bits, bits.ctypes.data)
    assert rc == 0 and (bits[n_bits:] == 9).all()
    return bits[:n_bits]


def stream_by_definition(seed, cell, frame, n_bits):
    """bit i is bit i mod 32 of word (i mod 128) div 32 of block i div 128 of Philox stream 4"""
    blocks = R._stream(seed, 4, cell, frame, (n_bits + 127) // 128)      # [blocks, 4]
    return np.array([(int(blocks[i // 128, (i % 128) // 32]) >> (i % 32)) & 1 for i in range(n_bits)], np.uint8)


def test_the_symbols_exist():
    assert R.STREAM_INFO == _lib.STREAM_INFO == 4 and "wofdm_coset_info" in _lib.EXPORTS
    for name in ("coset_info", "coset_codewords", "coset_ber", "coset_fer", "conv_encode_gpu", "ldpc_encode_gpu",
                 "rx_profile_coset_gpu", "rx_profile_coset_host", "frame_profile_coset", "RxProfileCoset", "coset_for_window_file"):
        assert hasattr(W, name), name


@pytest.mark.parametrize("seed", SEEDS)
def test_the_library_draws_the_mirrors_stream(seed):
    for frame in FRAMES:
        for cell in CELLS:
            for n_bits in N_BITS if (frame, cell) == (FRAMES[3], CELLS[2]) else N_BITS[2:4]:
                got = lib_info(seed, cell, frame, n_bits)
                assert np.array_equal(got, R.coset_info(seed, cell, frame, n_bits)), (seed, cell, frame, n_bits)
                assert np.array_equal(got, stream_by_definition(seed, cell, frame, n_bits))
    # a prefix is a prefix, and both halves of the seed and of the frame index enter
    long = lib_info(seed, 70001, 2 ** 32, 4097)
    assert 1800 < int(long.sum()) < 2300
    for n_bits in N_BITS:
        assert np.array_equal(lib_info(seed, 70001, 2 ** 32, n_bits), long[:n_bits])
    assert not np.array_equal(lib_info(seed ^ (1 << 40), 70001, 2 ** 32, 4097), long)
    assert not np.array_equal(lib_info(seed, 70001, 0, 4097), long)
    assert not np.array_equal(lib_info(seed, 70001 - 65536, 2 ** 32, 4097), long)


def test_the_host_call_checks_its_arguments():
    lib = _lib.load()
    bits = np.full(8, 9, np.uint8)
    assert lib.wofdm_coset_info(1, 0, 0, 8, None) == -1
    assert lib.wofdm_coset_info(1, 0, 0, -1, bits.ctypes.data) == -1
    assert lib.wofdm_coset_info(1, 2 ** 28, 0, 8, bits.ctypes.data) == -1 and (bits == 9).all()
    assert lib.wofdm_coset_info(1, 0, 0, 0, bits.ctypes.data) == 0 and (bits == 9).all()


def test_stream_4_is_none_of_the_other_streams():
    for seed, cell, frame in ((1, 0, 0), (SEEDS[1], 70001, 2 ** 32)):
        info = R._stream(seed, R.STREAM_INFO, cell, frame, 8)
        for other in (R.STREAM_BITS, R.STREAM_NOISE, R.STREAM_ACI, R.STREAM_PN):
            assert not (R._stream(seed, other, cell, frame, 8) == info).all(axis=1).any(), other
    # ... and it depends neither on the point nor on the code: nothing but (seed, cell, frame) enters
    xv, xl = R.coset_codewords(3, 5, 9, 900, (0, 2), ((4, 8), (3, 6)))
    assert np.array_equal(R.coset_codewords(3, 5, 9, 900, (2,), ((3, 6),))[0][0], xv[1])
    assert np.array_equal(R.coset_codewords(3, 5, 9, 900, (), ((3, 6),))[1][0], xl[1])


# ---- the transmitted words ----

@pytest.mark.parametrize("rate", (0, 1, 2))
@pytest.mark.parametrize("n_c", (56, 57, 64, 1350))
def test_the_viterbi_mirror_returns_an_encoded_word(rate, n_c):
    T = R.code_steps(rate, n_c)
    u = np.random.RandomState(n_c + rate).randint(0, 2, size=(3, T - 6)).astype(np.uint8)
    x = np.zeros((3, n_c), np.uint8)
    word = R.conv_encode(u, rate)
    x[:, :word.shape[1]] = word
    bits, metric = R.viterbi_decode((127 * (1 - 2 * x.astype(np.int32))).astype(np.int8), rate)
    assert np.array_equal(bits[:, :T - 6], u) and (bits[:, T - 6:] == 0).all()
    assert (metric == -127 * word.sum(axis=1, dtype=np.int64)).all()


@pytest.mark.parametrize("J,L,n", ((3, 6, 64), (4, 8, 488), (6, 24, 1000), (4, 16, 4096)))
def test_the_ldpc_mirror_returns_an_encoded_word_in_one_iteration(J, L, n):
    Z = R.ldpc_lift(J, L, n)
    u = np.random.RandomState(n).randint(0, 2, size=(3, n - J * Z)).astype(np.uint8)
    x = R.ldpc_encode(u, J, L, n)
    bits, iters, conv = R.ldpc_decode((127 * (1 - 2 * x.astype(np.int32))).astype(np.int8), J, L, 30)
    assert np.array_equal(bits, x) and np.array_equal(bits[:, J * Z:], u) and (iters == 1).all() and conv.all()


def test_coset_codewords_are_the_mirrors_of_the_stream():
    seed, cell, frame, n_f = 11, 3, 2 ** 32 + 1, 40000                   # W = 3 LDPC words of 13333, one position left over
    stream = R.coset_info(seed, cell, frame, n_f)
    xv, xl = R.coset_codewords(seed, cell, frame, n_f, (0, 1, 2), ((4, 8), (4, 16, 20)))
    assert xv.shape == (3, n_f) and xl.shape == (2, n_f) and xv.dtype == xl.dtype == np.uint8
    for i, r in enumerate((0, 1, 2)):
        word = R.conv_encode(stream[:R.code_steps(r, n_f) - 6], r)
        assert np.array_equal(xv[i, :word.size], word) and (xv[i, word.size:] == 0).all()
    assert R.ldpc_frame_words(n_f) == (3, 13333)
    for i, (J, L) in enumerate(((4, 8), (4, 16))):
        Z, edges = R.ldpc_edges(J, L, 13333)
        for w in range(3):
            x = xl[i, w * 13333:(w + 1) * 13333]
            K = 13333 - J * Z
            assert np.array_equal(x[J * Z:], stream[w * 13333:w * 13333 + K])
            full = np.concatenate([x, np.zeros(L * Z - 13333, np.uint8)])
            assert all((full[e].sum(axis=0) % 2 == 0).all() for e in edges)
        assert (xl[i, 3 * 13333:] == 0).all()
    with pytest.raises(ValueError):
        R.coset_codewords(seed, cell, frame, n_f, (), ())


# ---- the two views ----

def viterbi_views(s, u, rate):
    """(info-bit errors of the all-zero view, of the coset view) of soft words s [n_cw, n_c] behind information words u"""
    T = R.code_steps(rate, s.shape[1])
    x = np.zeros(s.shape, np.uint8)
    word = R.conv_encode(u, rate)
    x[:, :word.shape[1]] = word
    zero = R.viterbi_decode(s, rate)[0]
    coset = R.viterbi_decode(np.where(x != 0, -s.astype(np.int16), s).astype(np.int8), rate)[0]
    return int(zero[:, :T - 6].sum()), int((coset[:, :T - 6] ^ u).sum())


def ldpc_views(s, u, J, L, max_iter=30):
    n = s.shape[1]
    k0 = J * R.ldpc_lift(J, L, n)
    x = R.ldpc_encode(u, J, L, n)
    zero = R.ldpc_decode(s, J, L, max_iter)
    coset = R.ldpc_decode(np.where(x != 0, -s.astype(np.int16), s).astype(np.int8), J, L, max_iter)
    return ((int(zero[0][:, k0:].sum()), int(zero[1].sum())),
            (int((coset[0][:, k0:] ^ u).sum()), int(coset[1].sum())))


def tie_on_the_path(s, rate):
    """whether ``viterbi_decode``'s traceback of the soft word s [n_c] passes a state whose two predecessors had equal metrics"""
    s = np.asarray(s, np.int64)
    T = R.code_steps(rate, s.size)
    ca, cb, _ = R._kept_index(rate, T)
    ext = np.concatenate([s, [0]])
    st = np.arange(64)
    p0 = (st << 1) & 63
    r0 = ((st >> 5) << 6) | p0
    a0, b0 = R._parity(r0 & 0o133), R._parity(r0 & 0o171)
    m = np.full(64, 1 << 30, np.int64)
    m[0] = 0
    tie, dec = np.zeros((T, 64), bool), np.zeros((T, 64), np.int64)
    for t in range(T):
        da, db = ext[ca[t]], ext[cb[t]]
        c0 = m[p0] + a0 * da + b0 * db
        c1 = m[p0 | 1] + (1 - a0) * da + (1 - b0) * db
        tie[t], dec[t] = c0 == c1, c1 < c0
        m = np.minimum(c0, c1)
    state = 0
    for t in range(T - 1, -1, -1):
        if tie[t, state]:
            return True
        state = ((state << 1) & 63) | dec[t, state]
    return False


def flipped(s, u, rate):
    x = np.zeros(s.shape, np.uint8)
    word = R.conv_encode(u, rate)
    x[:, :word.shape[1]] = word
    return np.where(x != 0, -s.astype(np.int16), s).astype(np.int8)


@pytest.mark.parametrize("rate", (0, 1, 2))
def test_zeros_and_ties_fall_towards_the_all_zero_word_viterbi(rate):
    n_c = 600
    T = R.code_steps(rate, n_c)
    rs = np.random.RandomState(40 + rate)
    u = rs.randint(0, 2, size=(4, T - 6)).astype(np.uint8)
    # every soft bit 0: the decoder returns the all-zero word in either view
    zero, coset = viterbi_views(np.zeros((4, n_c), np.int8), u, rate)
    assert zero == 0 and coset == int(u.sum()) > 0
    # a stretch of zeros inside a clean word (as the all-zero view sees it: every soft bit positive)
    s = np.full((4, n_c), 40, np.int8)
    s[:, 200:400] = 0
    zero, coset = viterbi_views(s, u, rate)
    assert zero == 0 and coset > 0
    # exact ties without a zero: every soft bit +-1
    s = rs.choice(np.array([-1, 1], np.int8), size=(4, n_c))
    zero, coset = viterbi_views(s, u, rate)
    print("rate %d, +-1 words: info-bit errors in the all-zero view %d, in the coset view %d" % (rate, zero, coset))
    assert all(tie_on_the_path(w, rate) for w in s) and zero != coset


@pytest.mark.parametrize("rate", (0, 1, 2))
def test_without_zeros_or_ties_the_views_agree_viterbi(rate):
    n_c = 600
    T = R.code_steps(rate, n_c)
    rs = np.random.RandomState(50 + rate)
    u = rs.randint(0, 2, size=(48, T - 6)).astype(np.uint8)
    # noisy all-zero words (the all-zero view's input), weak to strong, the soft bits odd and from a wide range; of 48 candidates
    # those whose decoded path meets no tie in either view -- chosen by that property alone, before anything is counted
    s = np.clip(2.0 * np.rint(rs.normal(np.linspace(3.0, 15.0, 48), 17.0, size=(n_c, 48)).T) + 1.0, -127, 127).astype(np.int8)
    assert (s != 0).all()
    keep = [i for i, (a, b) in enumerate(zip(s, flipped(s, u, rate))) if not tie_on_the_path(a, rate) and not tie_on_the_path(b, rate)]
    assert len(keep) >= 8, len(keep)
    s, u = s[keep], u[keep]
    zero, coset = viterbi_views(s, u, rate)
    print("rate %d, noisy words: info-bit errors in the all-zero view %d, in the coset view %d" % (rate, zero, coset))
    assert zero == coset > 0


@pytest.mark.parametrize("J,L,n", ((3, 6, 64), (4, 8, 488)))
def test_zeros_fall_towards_the_all_zero_word_ldpc(J, L, n):
    K = n - J * R.ldpc_lift(J, L, n)
    rs = np.random.RandomState(60 + n)
    u = rs.randint(0, 2, size=(4, K)).astype(np.uint8)
    (zero, zit), (coset, cit) = ldpc_views(np.zeros((4, n), np.int8), u, J, L)
    assert zero == 0 and zit == 4 and coset == int(u.sum()) > 0           # (the all-zero word has an even syndrome: one iteration)
    # a low-SNR cell at a small llr_scale: a third of the soft bits are exactly 0
    s = np.rint(rs.normal(0.5, 0.8, size=(4, n))).astype(np.int8)
    assert 0.2 < (s == 0).mean() < 0.5
    (zero, _), (coset, _) = ldpc_views(s, u, J, L)
    print("(%d, %d, %d), low-SNR words: info-bit errors in the all-zero view %d, in the coset view %d" % (J, L, n, zero, coset))
    assert zero < coset


@pytest.mark.parametrize("J,L,n", ((3, 6, 64), (4, 8, 488), (4, 12, 1000)))
def test_without_zeros_the_views_agree_ldpc(J, L, n):
    Z = R.ldpc_lift(J, L, n)
    K = n - J * Z
    rs = np.random.RandomState(70 + n)
    u, other = rs.randint(0, 2, size=(2, 5, K)).astype(np.uint8)
    c2 = R.ldpc_encode(other, J, L, n)
    # what the all-zero view sees when the channel delivers ANOTHER codeword, strongly, with three weak errors in one block
    # column (no check joins two variables of a block column)
    s = (1 - 2 * c2.astype(np.int16)) * (2 * rs.randint(50, 64, size=c2.shape) + 1)
    for w in range(5):
        at = J * Z + rs.choice(Z, size=3, replace=False)
        s[w, at] = -np.sign(s[w, at]) * np.array([1, 3, 5])
    s = s.astype(np.int8)
    assert (np.abs(s) >= 101).sum() == 5 * (n - 3)
    for max_iter in (1, 30):
        zero, coset = ldpc_views(s, u, J, L, max_iter)
        assert zero == coset == (int(other.sum()), 5), (max_iter, zero, coset)


