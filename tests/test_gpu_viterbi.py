"""``wofdm_viterbi_decode`` on the GPU (wofdm_viterbi_kernel: one wave per codeword, one state per lane) against the integer numpy
mirror ``rx_profile.viterbi_decode``: bits and metric are equal EXACTLY -- both are pure integer arithmetic with the same tie rule.
(rate, n_c) cover a short word, the lengths around a puncturing period (56 / 57, 64 / 65) and the longest word the library takes
(n_c = 6144: T = 3072 and 4608); n_cw one wave, a few, and more than one round of the machine's workgroups; soft values from noisy
codewords of random info words, from [-3, 7] (ties everywhere) and from the full int8 range with -128; with and without ``perm``."""
import functools

import numpy as np
import pytest

from wofdm_amd import rx_profile as R

pytestmark = pytest.mark.gpu

SHAPES = ((0, 26), (1, 56), (1, 57), (2, 64), (2, 65), (0, 6144), (2, 6144))
N_CW = (1, 5, 257)


def draw(kind, rate, n_c, n_cw, rs):
    if kind == "noisy":
        steps = R.code_steps(rate, n_c)
        coded = R.conv_encode(rs.randint(0, 2, size=(n_cw, steps - 6)), rate)
        x = np.zeros((n_cw, n_c))
        x[:, :coded.shape[1]] = 24.0 * (1 - 2 * coded.astype(np.float64))
        return np.clip(np.rint(x + 28.0 * rs.standard_normal(x.shape)), -127, 127).astype(np.int8)
    if kind == "ties":
        return rs.randint(-3, 8, size=(n_cw, n_c)).astype(np.int8)
    return rs.randint(-128, 128, size=(n_cw, n_c)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def reference(rate, n_c, kind, with_perm):
    """(soft, perm, the mirror's bits and metric) for the largest n_cw, of which the smaller take the first words; computed once,
    not to be modified"""
    rs = np.random.RandomState(1000 * rate + n_c + 7 * ("noisy", "ties", "full").index(kind))
    n_cw = max(N_CW)
    soft = draw(kind, rate, n_c, n_cw, rs)
    perm = R.default_interleaver(n_c) if with_perm else None
    if with_perm and kind == "noisy":                                   # the codeword sits behind the interleaver
        placed = np.zeros_like(soft)
        placed[:, perm] = soft
        soft = placed
    bits, metric = R.viterbi_decode(soft, rate, perm)
    return soft, perm, bits, metric


@pytest.mark.parametrize("with_perm", (False, True))
@pytest.mark.parametrize("kind", ("noisy", "ties", "full"))
@pytest.mark.parametrize("rate,n_c", SHAPES)
def test_bits_and_metric_equal_the_mirrors(rate, n_c, kind, with_perm):
    soft, perm, bits, metric = reference(rate, n_c, kind, with_perm)
    if kind == "noisy":
        assert 0 < (bits.any(axis=1)).sum()                             # (random info words: the decoder decodes, not only zeros)
    if kind == "full":
        assert (soft == -128).any()
    for n_cw in N_CW:
        got_bits, got_metric = R.viterbi_decode_gpu(soft[:n_cw], rate, perm)
        assert got_bits.shape == (n_cw, R.code_steps(rate, n_c)) and got_bits.dtype == np.uint8
        assert np.array_equal(got_metric, metric[:n_cw]), (rate, n_c, kind, n_cw)
        assert np.array_equal(got_bits, bits[:n_cw]), (rate, n_c, kind, n_cw)


def test_noisy_words_decode_to_what_was_sent():
    rs = np.random.RandomState(5)
    info = rs.randint(0, 2, size=(257, 42 - 6))
    coded = R.conv_encode(info, 2)
    soft = np.zeros((257, 56), dtype=np.int8)
    soft[:, :coded.shape[1]] = 40 * (1 - 2 * coded.astype(np.int8))
    bits, metric = R.viterbi_decode_gpu(soft, 2)
    assert np.array_equal(bits[:, :36], info) and (bits[:, 36:] == 0).all()
    assert np.array_equal(metric, -40 * coded.sum(axis=1).astype(np.int64))
