"""``wofdm_ldpc_decode`` on the GPU (wofdm_ldpc_kernel: one workgroup per codeword, Q and R in LDS, a layer's checks strided over
the threads, the stop decision one workgroup-wide OR) against the integer numpy mirror ``rx_profile.ldpc_decode``: bits, iters and
converged are equal EXACTLY -- both are pure integer arithmetic.  The shapes (J, L, n) and why each is there:
    (3, 6, 64)      Z = 11    two shortened positions
    (4, 8, 488)     Z = 61    nothing shortened, Z under a wave
    (4, 8, 504)     Z = 67    Z over a wave
    (6, 24, 1000)   Z = 53    five whole block columns shortened
    (4, 8, 2000)    Z = 251   Z under 256 threads
    (4, 16, 4096)   Z = 257   Z over 256 threads
    (4, 8, 6272)    Z = 787   the benchmark's word
    (4, 8, 16384)   Z = 2053  the largest
n_cw is 1, 5 and 257 (1 and 3 at the largest).  The words of a shape are one matrix whose rows cycle through the inputs: noisy
codewords of RANDOM info words (BPSK over AWGN, soft = clip(rint(4 LLR), +-127)) at three noise levels -- clean (9 dB), the
waterfall, hopeless (-3 dB) --, draws from [-3, 7] (ties and zeros everywhere) and the full int8 range with -128; the first five
rows hold one of each, and n_cw = 1 runs on each of them.  Behind them mostly clean and waterfall rows, so that the mirror -- run
ONCE per shape to 64 iterations, its state after 1 and 30 kept -- stays quick.  With a permutation the same words sit behind it, so
the expected result is the same.  max_iter is 1, 30 and 64.  ``test_the_case_list_exercises_the_stop_rule`` asserts from the mirror
alone that the cases hold a word that stops early, one that converges exactly at max_iter, and one that never converges."""
import functools

import numpy as np
import pytest

from wofdm_amd import rx_profile as R

pytestmark = pytest.mark.gpu

#: (J, L, n, Z, Eb/N0 of the waterfall rows in dB)
SHAPES = ((3, 6, 64, 11, 5.0), (4, 8, 488, 61, 3.5), (4, 8, 504, 67, 3.5), (6, 24, 1000, 53, 4.5), (4, 8, 2000, 251, 3.0),
          (4, 16, 4096, 257, 3.5), (4, 8, 6272, 787, 2.5), (4, 8, 16384, 2053, 2.25))
MAX_ITERS = (1, 30, 64)
KINDS = ("clean", "waterfall", "hopeless", "ties", "full")


def n_cws(n):
    return (1, 5, 257) if n < 16384 else (1, 3)


def kind_of_row(r):
    if r < 5:
        return KINDS[r]
    if r % 32 in (7, 15, 23):
        return KINDS[2 + (r % 32) // 8]
    return KINDS[r & 1]


@functools.lru_cache(maxsize=None)
def reference(J, L, n):
    """(words [rows, n] int8 as the decoder reads them, info-bit count K, {max_iter: (bits, iters, converged)} of the mirror);
    computed once per shape, not to be modified"""
    Z, ebn0 = next((s[3], s[4]) for s in SHAPES if s[:3] == (J, L, n))
    K = n - J * Z
    rs = np.random.RandomState(100 * J + L + n)
    rows = max(max(n_cws(n)), 5)
    code = R.ldpc_encode(rs.randint(0, 2, size=(rows, K)), J, L, n)
    words = np.zeros((rows, n), dtype=np.int8)
    for r in range(rows):
        kind = kind_of_row(r)
        if kind == "ties":
            words[r] = rs.randint(-3, 8, size=n)
        elif kind == "full":
            words[r] = rs.randint(-128, 128, size=n)
            words[r, rs.randint(0, n, size=3)] = -128
        else:
            db = {"clean": 9.0, "waterfall": ebn0, "hopeless": -3.0}[kind]
            var = 1.0 / (2.0 * (K / n) * 10.0 ** (db / 10.0))
            y = 1.0 - 2.0 * code[r] + np.sqrt(var) * rs.standard_normal(n)
            words[r] = np.clip(np.rint(4.0 * 2.0 * y / var), -127, 127)
    return words, K, R.ldpc_decode_at(words, J, L, MAX_ITERS)


def batches(n):
    """the row ranges of the GPU calls: every one of the five inputs alone, then the n_cw beyond 1"""
    out = [(r, r + 1) for r in range(5)]
    for m in n_cws(n)[1:]:
        out.append((0, m))
        if m < 5:
            out.append((5 - m, 5))
    return out


@pytest.mark.parametrize("with_perm", (False, True))
@pytest.mark.parametrize("J,L,n,Z,ebn0", SHAPES)
def test_bits_iters_and_converged_equal_the_mirrors(J, L, n, Z, ebn0, with_perm):
    assert R.ldpc_lift(J, L, n) == Z
    words, K, ref = reference(J, L, n)
    assert (words == -128).any()
    perm, soft = None, words
    if with_perm:
        perm = np.random.RandomState(n).permutation(n).astype(np.int32)
        soft = np.zeros_like(words)
        soft[:, perm] = words                                           # variable c is read at soft[:, perm[c]]
    assert ref[64][0][:, J * Z:].any(axis=1).sum() > 0                  # (random info words: not only zeros come out)
    for max_iter in MAX_ITERS:
        bits, iters, conv = ref[max_iter]
        for a, b in batches(n):
            got_bits, got_iters, got_conv = R.ldpc_decode_gpu(soft[a:b], J, L, max_iter, perm)
            assert got_bits.shape == (b - a, n) and got_bits.dtype == np.uint8
            assert np.array_equal(got_iters, iters[a:b]), (J, L, n, max_iter, a, b, got_iters, iters[a:b])
            assert np.array_equal(got_conv, conv[a:b]), (J, L, n, max_iter, a, b)
            assert np.array_equal(got_bits, bits[a:b]), (J, L, n, max_iter, a, b)


def test_the_case_list_exercises_the_stop_rule():
    """from the mirror alone, on the shapes whose mirror is cheapest: a decoder that ignored the stop rule could not pass"""
    early = exact = never = between = False
    for J, L, n, Z, _ in SHAPES[:5]:
        _, _, ref = reference(J, L, n)
        for max_iter in MAX_ITERS:
            _, iters, conv = ref[max_iter]
            assert (iters >= 1).all() and (iters <= max_iter).all() and (iters[~conv] == max_iter).all()
            early |= bool((conv & (iters < max_iter)).any())
            exact |= bool((conv & (iters == max_iter)).any())
            never |= bool((~conv).any()) and max_iter == 64
            between |= bool((conv & (iters > 1) & (iters < 30)).any())
    assert early and exact and never and between


def test_iters_and_converged_may_be_null():
    from wofdm_amd import _lib
    J, L, n = 4, 8, 488
    words, _, ref = reference(J, L, n)
    soft = np.ascontiguousarray(words[:5])
    bits = np.zeros((5, n), dtype=np.uint8)
    _lib.check(_lib.load().wofdm_ldpc_decode(0, J, L, 30, n, None, 5, soft.ctypes.data, bits.ctypes.data, None, None))
    assert np.array_equal(bits, ref[30][0][:5])
