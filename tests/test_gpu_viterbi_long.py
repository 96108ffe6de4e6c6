"""``wofdm_viterbi_decode_long`` on the GPU (wofdm_viterbi_long_kernel: one wave per codeword, one state per lane, the survivor
history streamed to device memory in blocks of 64 steps) against the integer numpy mirror ``rx_profile.viterbi_decode`` and,
wherever T <= 4608, against ``wofdm_viterbi_decode`` (wofdm_viterbi_kernel): bits and metric are equal EXACTLY -- all three are pure
integer arithmetic with the same start and tie rule.  (rate, n_c) sit at the block boundaries of the history (T = 63, 64, 65, 128,
129), at the shortest word (T = 7), at the existing decoder's limit (4608) and beyond it (4609, 4611, 13333); n_cw one wave, a few,
and more than one round of the machine's workgroups (257; at T = 13333 the mirror's decision array, steps x n_cw x 64 bytes, keeps
it to 1 and 5); soft values from noisy codewords of random info words, from [-3, 7] (ties everywhere) and from the full int8 range
with -128; with and without ``perm``."""
import functools

import numpy as np
import pytest

from wofdm_amd import _lib
from wofdm_amd import rx_profile as R

import test_gpu_viterbi as TV

pytestmark = pytest.mark.gpu

#: (rate, n_c, T)
SHAPES = ((0, 14, 7), (0, 126, 63), (0, 128, 64), (0, 130, 65), (0, 256, 128), (0, 258, 129), (1, 57, 38), (2, 65, 48),
          (2, 6144, 4608), (0, 9218, 4609), (2, 6149, 4611), (1, 20000, 13333))


def n_cws(steps):
    return (1, 5, 257) if steps <= 4611 else (1, 5)


@functools.lru_cache(maxsize=None)
def reference(rate, n_c, kind, with_perm):
    """(soft, perm, the mirror's bits and metric) for the largest n_cw, of which the smaller take the first words; computed once,
    not to be modified"""
    rs = np.random.RandomState(2000 * rate + n_c + 7 * ("noisy", "ties", "full").index(kind))
    n_cw = max(n_cws(R.code_steps(rate, n_c)))
    soft = TV.draw(kind, rate, n_c, n_cw, rs)
    perm = R.default_interleaver(n_c) if with_perm else None
    if with_perm and kind == "noisy":                                   # the codeword sits behind the interleaver
        placed = np.zeros_like(soft)
        placed[:, perm] = soft
        soft = placed
    bits, metric = R.viterbi_decode(soft, rate, perm)
    return soft, perm, bits, metric


@pytest.mark.parametrize("with_perm", (False, True))
@pytest.mark.parametrize("kind", ("noisy", "ties", "full"))
@pytest.mark.parametrize("rate,n_c,steps", SHAPES)
def test_bits_and_metric_equal_the_mirrors_and_the_lds_decoders(rate, n_c, steps, kind, with_perm):
    assert R.code_steps(rate, n_c) == steps
    soft, perm, bits, metric = reference(rate, n_c, kind, with_perm)
    if kind == "noisy":
        assert 0 < (bits.any(axis=1)).sum()                             # (random info words: the decoder decodes, not only zeros)
    if kind == "full":
        assert (soft == -128).any()
    for n_cw in n_cws(steps):
        got_bits, got_metric = R.viterbi_decode_long_gpu(soft[:n_cw], rate, perm)
        assert got_bits.shape == (n_cw, steps) and got_bits.dtype == np.uint8
        assert np.array_equal(got_metric, metric[:n_cw]), (rate, n_c, kind, n_cw)
        assert np.array_equal(got_bits, bits[:n_cw]), (rate, n_c, kind, n_cw)
        if steps <= _lib.CODE_MAX_STEPS:
            old_bits, old_metric = R.viterbi_decode_gpu(soft[:n_cw], rate, perm)
            assert np.array_equal(got_metric, old_metric) and np.array_equal(got_bits, old_bits), (rate, n_c, kind, n_cw)
        else:
            with pytest.raises(RuntimeError):
                R.viterbi_decode_gpu(soft[:1], rate, perm)


def test_the_metric_of_a_constant_word_stays_far_inside_int32():
    rate, n_c = 1, 20000
    soft = np.full((2, n_c), -128, dtype=np.int8)
    bits, metric = R.viterbi_decode(soft, rate)
    got_bits, got_metric = R.viterbi_decode_long_gpu(soft, rate)
    assert np.array_equal(got_metric, metric) and np.array_equal(got_bits, bits)
    # every kept output is -128: a path pays -128 per hypothesised one, at most all n_c of them
    assert (-128 * n_c <= got_metric).all() and (got_metric < -128 * n_c // 4).all() and 128 * n_c < 1 << 22


def test_noisy_long_words_decode_to_what_was_sent():
    rs = np.random.RandomState(6)
    rate, n_c = 2, 6149
    steps = R.code_steps(rate, n_c)
    info = rs.randint(0, 2, size=(5, steps - 6))
    coded = R.conv_encode(info, rate)
    soft = np.zeros((5, n_c), dtype=np.int8)
    soft[:, :coded.shape[1]] = 40 * (1 - 2 * coded.astype(np.int8))
    bits, metric = R.viterbi_decode_long_gpu(soft, rate)
    assert np.array_equal(bits[:, :steps - 6], info) and (bits[:, steps - 6:] == 0).all()
    assert np.array_equal(metric, -40 * coded.sum(axis=1).astype(np.int64))
