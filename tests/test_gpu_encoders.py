"""``wofdm_conv_encode`` and ``wofdm_ldpc_encode`` on the GPU against the numpy mirrors ``rx_profile.conv_encode`` and
``rx_profile.ldpc_encode``, bit for bit.

wofdm_conv_encode_kernel takes one trellis step per lane and stores a step's kept outputs at their closed-form positions: n_c = 56,
57 and 64 are the header's examples (57 and 64 leave positions over at some rates; T = 28 ... 48 is less than one workgroup of 256
steps), 6144 is several workgroups with a partial last one, 37 632 the longest frame of the receive-profile tests (T = 28 224 at
rate 3/4); all three rates, n_cw = 1, 5 and 257.  The left-over positions must come back 0 from a buffer the library allocates, so
the information words are random and the output is compared whole.

wofdm_ldpc_encode_kernel holds a word as bits in LDS and back-substitutes a block row at a time; the shapes are those of
tests/test_gpu_ldpc.py (shortened positions, Z under and over a wave, under and over 256 threads, whole block columns shortened,
the largest word).  Beside the mirror, and independently of its encoder, every check of ``ldpc_edges`` has even parity on the GPU's
word."""
import numpy as np
import pytest

from wofdm_amd import rx_profile as R

import test_gpu_ldpc as TL

pytestmark = pytest.mark.gpu

N_CS = (56, 57, 64, 6144, 37632)
N_CWS = (1, 5, 257)


@pytest.mark.parametrize("rate", (0, 1, 2))
@pytest.mark.parametrize("n_c", N_CS)
def test_conv_encode_equals_the_mirror(n_c, rate):
    T = R.code_steps(rate, n_c)
    info = np.random.RandomState(7 * n_c + rate).randint(0, 2, size=(max(N_CWS), T - 6)).astype(np.uint8)
    word = R.conv_encode(info, rate)
    want = np.zeros((max(N_CWS), n_c), np.uint8)
    want[:, :word.shape[1]] = word
    assert n_c - 3 <= word.shape[1] <= n_c and want.any()
    for n_cw in N_CWS:
        got = R.conv_encode_gpu(info[-n_cw:], rate, n_c)
        assert got.shape == (n_cw, n_c) and got.dtype == np.uint8
        assert np.array_equal(got, want[-n_cw:]), (n_c, rate, n_cw)


def test_conv_encode_reads_bit_0_of_a_byte_and_takes_the_shortest_word():
    info = np.random.RandomState(3).randint(0, 256, size=(5, 26)).astype(np.uint8)
    assert np.array_equal(R.conv_encode_gpu(info, 0, 64), R.conv_encode(info & 1, 0))
    for rate, n_c in ((0, 14), (1, 11), (2, 10)):                        # T = 7: one information bit
        assert R.code_steps(rate, n_c) == 7
        for bit in (0, 1):
            got = R.conv_encode_gpu(np.array([[bit]], np.uint8), rate, n_c)
            word = R.conv_encode(np.array([[bit]]), rate)
            assert np.array_equal(got[:, :word.shape[1]], word) and (got[:, word.shape[1]:] == 0).all()
    with pytest.raises(ValueError):
        R.conv_encode_gpu(info, 0, 66)


@pytest.mark.parametrize("J,L,n,Z,ebn0", TL.SHAPES)
def test_ldpc_encode_equals_the_mirror_and_every_check_is_even(J, L, n, Z, ebn0):
    assert R.ldpc_lift(J, L, n) == Z
    K = n - J * Z
    info = np.random.RandomState(n + J).randint(0, 2, size=(max(TL.n_cws(n)), K)).astype(np.uint8)
    want = R.ldpc_encode(info, J, L, n)
    _, edges = R.ldpc_edges(J, L, n)
    for n_cw in TL.n_cws(n):
        got = R.ldpc_encode_gpu(info[-n_cw:], J, L, n)
        assert got.shape == (n_cw, n) and got.dtype == np.uint8 and got.max() == 1
        assert np.array_equal(got[:, J * Z:], info[-n_cw:])
        full = np.concatenate([got, np.zeros((n_cw, L * Z - n), np.uint8)], axis=1)
        for i, e in enumerate(edges):
            assert (full[:, e].sum(axis=1) % 2 == 0).all(), (J, L, n, n_cw, i)
        assert np.array_equal(got, want[-n_cw:]), (J, L, n, n_cw)


def test_ldpc_encode_reads_bit_0_of_a_byte():
    J, L, n = 4, 8, 504
    info = np.random.RandomState(5).randint(0, 256, size=(3, n - J * R.ldpc_lift(J, L, n))).astype(np.uint8)
    assert np.array_equal(R.ldpc_encode_gpu(info, J, L, n), R.ldpc_encode(info & 1, J, L, n))
    with pytest.raises(ValueError):
        R.ldpc_encode_gpu(info[:, 1:], J, L, n)
