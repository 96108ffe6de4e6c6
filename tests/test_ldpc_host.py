"""The quasi-cyclic LDPC code and its integer mirror without a GPU: ``ldpc_lift`` gives the lift table of the issue from the
definition (and the library's host function the same); the dense check matrix has no 4-cycle over a sweep with Z <= 120;
``ldpc_encode`` of random info words has a zero syndrome, (6, 24, 1000) with its 272 shortened positions included; a clean +-127
word decodes in one iteration and an all-zero soft word gives all-zero bits, converged, in one iteration; the coding-gain case --
(4, 8) at n = 6272 and Eb/N0 = 2.5 dB, BPSK over AWGN, soft = clip(rint(4 LLR), +-127), a fixed seed chosen on the CPU -- where the
LDPC mirror decodes every frame's information bits and ``viterbi_decode`` at rate 1/2 leaves info-bit errors on the same soft
bits; and ``rx_profile_ldpc_host`` carries the tracking mirror's fields."""
import numpy as np
import pytest

from wofdm_amd import _lib
from wofdm_amd import rx_profile as R

import doppler_cases as DC

LIFTS = {(4, 8, 448): 59, (4, 8, 488): 61, (4, 8, 504): 67, (4, 16, 976): 61, (6, 24, 1000): 53, (4, 16, 4096): 257,
         (4, 8, 6272): 787, (4, 12, 6272): 523, (4, 16, 6272): 397, (3, 6, 16384): 2731, (4, 8, 16384): 2053}


def is_prime(z):
    return z >= 2 and all(z % d for d in range(2, int(z ** 0.5) + 1))


def order_of_two(z):
    k, p = 1, 2 % z
    while p != 1:
        k, p = k + 1, (2 * p) % z
    return k


@pytest.mark.parametrize("key", sorted(LIFTS))
def test_the_lift_table(key):
    J, L, n = key
    Z = R.ldpc_lift(J, L, n)
    assert Z == LIFTS[key]
    assert _lib.load().wofdm_ldpc_lift(J, L, n) == Z                   # (host only: no device is touched)
    # ... from the definition: the smallest prime at or above max(L, ceil(n / L)) whose order of 2 is at least L
    lo = max(L, -(-n // L))
    assert is_prime(Z) and order_of_two(Z) >= L and Z >= lo
    assert not any(is_prime(z) and order_of_two(z) >= L for z in range(lo, Z))


def test_the_lift_refuses_what_the_header_says():
    for J, L, n in ((2, 8, 100), (7, 12, 100), (4, 4, 100), (4, 25, 100), (4, 8, 0), (4, 8, 1), (6, 7, 6), (3, 4, 15)):
        with pytest.raises(ValueError):
            R.ldpc_lift(J, L, n)
        assert _lib.load().wofdm_ldpc_lift(J, L, n) == -1, (J, L, n)       # WOFDM_E_INVALID
    assert R.ldpc_lift(3, 4, 16) == 5 and R.ldpc_lift(3, 6, 64) == 11   # (K = 1; s = 2)


def dense(J, L, n):
    Z, idx = R.ldpc_edges(J, L, n)
    H = np.zeros((J * Z, L * Z), dtype=np.int64)
    for i in range(J):
        assert idx[i].shape == (L - i, Z)
        for e in range(L - i):
            assert (idx[i][e] // Z == i + e).all()                     # block (i, j) is zero for j < i, one circulant otherwise
            H[i * Z + np.arange(Z), idx[i][e]] += 1
    return Z, H


@pytest.mark.parametrize("J", (3, 4, 5, 6))
def test_no_four_cycle_on_the_dense_matrix(J):
    seen = 0
    for L in sorted({J + 1, J + 2, 8, 12, 16, 24} - set(range(J + 1))):
        for n in (1, 200, 1000):
            try:
                Z = R.ldpc_lift(J, L, n)
            except ValueError:                                          # (K < 1)
                Z = 121
            if Z > 120:
                continue
            Z, H = dense(J, L, n)
            assert H.max() == 1
            assert (H.sum(axis=1) == np.repeat(L - np.arange(J), Z)).all()      # row i has degree L - i
            both = H @ H.T                                              # two checks share at most one variable
            np.fill_diagonal(both, 0)
            assert both.max() <= 1, (J, L, n)
            seen += 1
    assert seen >= 4


@pytest.mark.parametrize("J,L,n", ((6, 24, 1000), (4, 8, 488), (3, 6, 64), (4, 16, 976), (4, 8, 6272)))
def test_encoded_words_have_a_zero_syndrome_and_decode_in_one_iteration(J, L, n):
    rs = np.random.RandomState(n)
    Z, idx = R.ldpc_edges(J, L, n)
    K = n - J * Z
    if (J, L, n) == (6, 24, 1000):
        assert L * Z - n == 272 and K == 682
    info = rs.randint(0, 2, size=(4, K))
    word = R.ldpc_encode(info, J, L, n)
    assert word.shape == (4, n) and np.array_equal(word[:, J * Z:], info)
    full = np.zeros((4, L * Z), dtype=np.int64)
    full[:, :n] = word                                                  # the shortened positions are zeros
    for i in range(J):
        assert not (full[:, idx[i]].sum(axis=1) & 1).any()
    assert word[:, :J * Z].any()                                        # (the parity part is not trivially zero)
    bits, iters, conv = R.ldpc_decode((127 * (1 - 2 * word.astype(np.int64))).astype(np.int8), J, L, 30)
    assert np.array_equal(bits, word) and (iters == 1).all() and conv.all()
    bits, iters, conv = R.ldpc_decode(np.zeros((2, n), dtype=np.int8), J, L, 30)
    assert not bits.any() and (iters == 1).all() and conv.all()
    with pytest.raises(ValueError):
        R.ldpc_encode(info[:, :-1], J, L, n)


def test_decode_at_is_decode_at_every_stop_and_perm_reads_behind_the_permutation():
    J, L, n = 4, 8, 504
    rs = np.random.RandomState(5)
    soft = rs.randint(-20, 40, size=(6, n)).astype(np.int8)
    soft[:, :3] = -128
    at = R.ldpc_decode_at(soft, J, L, (1, 4, 9))
    for m in (1, 4, 9):
        for a, b in zip(at[m], R.ldpc_decode(soft, J, L, m)):
            assert np.array_equal(a, b)
        assert (at[m][1][~at[m][2]] == m).all()
    perm = rs.permutation(n)
    placed = np.zeros_like(soft)
    placed[:, perm] = soft
    for a, b in zip(R.ldpc_decode(placed, J, L, 9, perm), at[9]):
        assert np.array_equal(a, b)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            R.ldpc_decode(soft, J, L, bad)


def test_the_ldpc_code_decodes_where_the_convolutional_code_leaves_errors():
    """(4, 8) at n = 6272, K = 3124, against the K = 7 code at rate 1/2 with 3130 info bits on the SAME soft bits (the random-coset
    view: the LDPC codeword's signs are taken out, so that the Viterbi decoder's all-zero word is the transmitted one)"""
    J, L, n, frames = 4, 8, 6272, 4
    rs = np.random.RandomState(0)
    Z = R.ldpc_lift(J, L, n)
    K = n - J * Z
    assert (Z, K) == (787, 3124) and R.code_steps(0, n) - 6 == 3130
    word = R.ldpc_encode(rs.randint(0, 2, size=(frames, K)), J, L, n)
    var = 1.0 / (2.0 * (K / n) * 10.0 ** 0.25)
    y = 1.0 - 2.0 * word + np.sqrt(var) * rs.standard_normal((frames, n))
    soft = np.clip(np.rint(4.0 * 2.0 * y / var), -127, 127).astype(np.int8)
    bits, iters, _ = R.ldpc_decode(soft, J, L, 30)
    assert np.array_equal(bits[:, J * Z:], word[:, J * Z:])            # every frame's information bits
    assert 2 <= iters.min()
    coset = (soft.astype(np.int64) * (1 - 2 * word.astype(np.int64))).astype(np.int8)
    vbits, _ = R.viterbi_decode(coset, 0)
    assert vbits[:, :-6].sum() > 0


def test_the_host_profile_carries_the_tracking_mirrors_fields():
    c = dict(DC.case("n64_wtx_plain"))
    on = np.ones(64, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    pil, S = R.pilot_comb(on, 8), c["S"]
    L, TP = R.LinkPoint, R.TrackingPoint
    pts, tps = [L(cfo=0.02, cfo_tracked=0)] * 2, [TP(1, 1), TP(1, 0)]
    head = (c["st"], c["k"], S, c["w_tx"][:1], c["w_rx"][:1], c["h"][:1], c["snr"][:1], 5, 0, 2, pts, tps, pil, (0.5,))
    side = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    n_c = c["k"] * int((on & ~pil).sum())
    codes = ((3, 6, 7), (4, 8))
    prof = R.rx_profile_ldpc_host(*head, R.LLR_SCALE, R.default_interleaver(n_c), codes, None, with_soft=True, **side)[0]
    trk = R.rx_profile_tracking_host(*head, **side)
    assert type(prof) is R.RxProfileLdpc
    for f in R.RxProfileTracking._fields:
        assert np.array_equal(getattr(prof, f), getattr(trk, f)), f
    assert prof.sym_rot == n_c // (S - 1) and prof.codes == ((3, 6, 7), (4, 8, R.LDPC_MAX_ITER)) and list(prof.codewords) == [2, 2]
    ns = [n_c * (S - 1 - q.post) for q in tps]
    assert prof.info_bits.tolist() == [[n - J * R.ldpc_lift(J, Lc, n) for J, Lc, _ in prof.codes] for n in ns]
    assert prof.info_err.shape == prof.cw_err.shape == prof.unconverged.shape == prof.iterations.shape == (2, 1, 1, 1, 2)
    assert (prof.cw_err <= 2).all() and (prof.unconverged <= 2).all() and (prof.iterations >= 2).all()
    # the counts are the integer decoder's on the mirror's own soft bits, gathered through the frame interleaver
    pos = (8 * np.flatnonzero(on & ~pil)[:, None] + np.arange(c["k"])[None, :]).reshape(-1)
    for i, q in enumerate(tps):
        words = R.frame_codewords(prof.soft_bits[0, 0, 0, :, i], q.post, pos, R.default_interleaver(n_c), prof.sym_rot)
        assert words.shape == (2, ns[i]) and R.ldpc_frame_words(ns[i]) == (1, ns[i])
        for jc, (J, Lc, m) in enumerate(prof.codes):
            bits, iters, conv = R.ldpc_decode(words, J, Lc, m)
            info = bits[:, J * R.ldpc_lift(J, Lc, ns[i]):]
            assert [prof.info_err[i, 0, 0, 0, jc], prof.cw_err[i, 0, 0, 0, jc], prof.unconverged[i, 0, 0, 0, jc],
                    prof.iterations[i, 0, 0, 0, jc]] == [info.sum(), info.any(axis=1).sum(), (~conv).sum(), iters.sum()]
    assert np.array_equal(R.ldpc_fer(prof), prof.cw_err / 2.0)
    assert np.array_equal(R.ldpc_mean_iterations(prof), prof.iterations / 2.0)
    assert np.array_equal(R.ldpc_ber(prof), prof.info_err / (2.0 * prof.info_bits[:, None, None, None, :]))
    assert R.ldpc_frame_words(16384) == (1, 16384) and R.ldpc_frame_words(16385) == (2, 8192) and R.ldpc_frame_words(40000) == (3, 13333)
