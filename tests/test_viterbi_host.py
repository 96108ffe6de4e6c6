"""The K = 7, 133 / 171 code and its integer decoder without a GPU (include/wofdm.h, ``rx_profile.viterbi_decode``): the mirror's
final metric is the exhaustive minimum over all 2^(T - 6) terminated words at T = 14 for the three rates, on soft values drawn from
[-3, 7] so that ties are plentiful; the decoded word re-encodes to that metric and ends in the zero tail; a noise-free round trip
through a non-identity interleaver; ``code_steps`` on the header's values; the minimum weight over at most 8 info bits is 10."""
import itertools

import numpy as np
import pytest

from wofdm_amd import rx_profile as R

#: n_c that gives T = 14 per rate: 2 T; 3 (T / 2); 4 (T / 3) + 3 for T mod 3 = 2
N_C_T14 = {0: 28, 1: 21, 2: 19}


def path_metric(soft, coded):
    """the sum of d over the kept outputs whose coded bit is 1"""
    return (soft[..., :coded.shape[-1]].astype(np.int64) * coded).sum(axis=-1)


@pytest.mark.parametrize("rate", (0, 1, 2))
def test_final_metric_is_the_exhaustive_minimum(rate):
    n_c = N_C_T14[rate]
    assert R.code_steps(rate, n_c) == 14
    words = np.array(list(itertools.product((0, 1), repeat=8)), dtype=np.uint8)
    coded = R.conv_encode(words, rate)                                  # [256, kept]
    assert coded.shape[1] <= n_c < coded.shape[1] + 2
    rs = np.random.RandomState(40 + rate)
    soft = rs.randint(-3, 8, size=(200, n_c)).astype(np.int8)
    bits, metric = R.viterbi_decode(soft, rate)
    every = (soft[:, None, :coded.shape[1]].astype(np.int64) * coded[None]).sum(axis=-1)     # [200, 256]
    best = every.min(axis=1)
    tied = ((every == best[:, None]).sum(axis=1) > 1).mean()
    print("rate %s: %.0f %% of the words have tied minima" % (R.CODE_RATES[rate], 100 * tied))
    assert tied > 0.02
    assert np.array_equal(metric, best)
    assert bits.shape == (200, 14) and (bits[:, 8:] == 0).all()
    assert np.array_equal(path_metric(soft, R.conv_encode(bits[:, :8], rate)), best)


@pytest.mark.parametrize("rate", (0, 1, 2))
def test_noise_free_round_trip_through_an_interleaver(rate):
    n_c = 57
    steps = R.code_steps(rate, n_c)
    rs = np.random.RandomState(7 + rate)
    info = rs.randint(0, 2, size=(9, steps - 6))
    coded = R.conv_encode(info, rate)
    perm = R.default_interleaver(n_c)
    assert not np.array_equal(perm, np.arange(n_c)) and np.array_equal(np.sort(perm), np.arange(n_c))
    stream = np.zeros((9, n_c), dtype=np.int8)
    stream[:, :coded.shape[1]] = 20 * (1 - 2 * coded.astype(np.int8))
    soft = np.zeros_like(stream)
    soft[:, perm] = stream                                              # coded-stream index c reads position perm[c]
    bits, metric = R.viterbi_decode(soft, rate, perm)
    assert np.array_equal(bits[:, :steps - 6], info) and (bits[:, steps - 6:] == 0).all()
    assert np.array_equal(metric, -20 * coded.sum(axis=1).astype(np.int64))
    wrong, _ = R.viterbi_decode(soft, rate)
    assert not np.array_equal(wrong[:, :steps - 6], info)
    with pytest.raises(ValueError):
        R.viterbi_decode(soft, rate, np.zeros(n_c, dtype=np.int32))


def test_code_steps():
    for n_c, want in ((56, (28, 37, 42)), (57, (28, 38, 42)), (64, (32, 42, 48)), (6144, (3072, 4096, 4608))):
        assert tuple(R.code_steps(r, n_c) for r in (0, 1, 2)) == want
    for rate in (0, 1, 2):
        for n_c in range(0, 40):
            steps = R.code_steps(rate, n_c)
            assert R._kept_index(rate, steps)[2] <= n_c < R._kept_index(rate, steps + 1)[2]
    with pytest.raises(ValueError):
        R.code_steps(3, 10)


def test_free_distance_is_ten():
    words = np.array(list(itertools.product((0, 1), repeat=8)), dtype=np.uint8)[1:]
    weight = R.conv_encode(words, 0).sum(axis=1)
    assert weight.min() == 10
