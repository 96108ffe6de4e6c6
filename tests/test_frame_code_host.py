"""The frame-spanning code without a GPU: ``frame_interleaver`` is a bijection onto (symbol, position) and with one symbol and no
rotation the interleaver within a symbol itself; a noise-free codeword placed through it survives the erasure of a whole symbol --
the first or the last -- at every rate, where the same symbols coded one by one lose the erased symbol's codeword entirely (time
diversity, deterministic); and the fp64 mirror ``rx_profile_coded_frame_host`` has the tracking mirror's fields and, on one data
symbol without rotation, the per-symbol mirror's counts."""
import numpy as np
import pytest

from wofdm_amd import rx_profile as R

import doppler_cases as DC

L, TP = R.LinkPoint, R.TrackingPoint

SHAPES = ((56, 1), (56, 2), (56, 5), (48, 4), (336, 15))
DIVERSITY = ((56, 5), (48, 4), (336, 15), (448, 14))


@pytest.mark.parametrize("with_perm", (False, True))
@pytest.mark.parametrize("n_c,s_d", SHAPES)
def test_frame_interleaver_is_a_bijection(n_c, s_d, with_perm):
    perm = R.default_interleaver(n_c) if with_perm else None
    for rot in (0, 1, n_c // s_d, n_c - 1):
        j, at = R.frame_interleaver(n_c, s_d, rot, perm)
        assert j.shape == at.shape == (n_c * s_d,)
        assert np.array_equal(j, np.arange(n_c * s_d) % s_d)           # consecutive coded bits, consecutive symbols
        assert np.array_equal(np.sort(j * n_c + at), np.arange(n_c * s_d))
        for s in range(s_d):                                           # per symbol a bijection of its positions
            assert np.array_equal(np.sort(at[j == s]), np.arange(n_c))
        # the definition, index by index
        p = np.arange(n_c) if perm is None else perm
        for c in (0, 1, s_d, n_c * s_d - 1, (n_c * s_d) // 2):
            assert at[c] == p[(c // s_d + (c % s_d) * rot) % n_c], (c, rot)
        if rot % n_c != 0 and s_d > 1 and perm is None:
            assert (at[1:][j[1:] != 0] != at[:-1][j[1:] != 0]).all()   # ... and another place of the band
    assert R.default_sym_rot(n_c, s_d) == n_c // s_d


def test_one_symbol_without_rotation_is_perm_itself():
    for n_c in (56, 57, 448):
        perm = R.default_interleaver(n_c)
        j, at = R.frame_interleaver(n_c, 1, 0, perm)
        assert (j == 0).all() and np.array_equal(at, perm)
        assert np.array_equal(R.frame_interleaver(n_c, 1, 0)[1], np.arange(n_c))
    assert np.array_equal(R.frame_interleaver(56, 3, 56 + 18)[1], R.frame_interleaver(56, 3, 18)[1])   # (modulo n_c)
    for bad in (dict(n_c=56, s_d=0, sym_rot=0), dict(n_c=0, s_d=2, sym_rot=0), dict(n_c=56, s_d=2, sym_rot=-1)):
        with pytest.raises(ValueError):
            R.frame_interleaver(**bad)


@pytest.mark.parametrize("n_c,s_d", DIVERSITY)
def test_a_frame_codeword_survives_an_erased_symbol_and_per_symbol_codewords_do_not(n_c, s_d):
    rs = np.random.RandomState(n_c + s_d)
    perm, rot = R.default_interleaver(n_c), n_c // s_d
    j, at = R.frame_interleaver(n_c, s_d, rot, perm)
    for rate in (0, 1, 2):
        steps = R.code_steps(rate, n_c * s_d)
        info = rs.randint(0, 2, size=steps - 6)
        coded = R.conv_encode(info, rate)
        word = np.zeros(n_c * s_d, dtype=np.int8)
        word[:coded.size] = 40 * (1 - 2 * coded.astype(np.int8))
        syms = np.zeros((s_d, n_c), dtype=np.int8)
        syms[j, at] = word
        # the same symbols, one codeword each
        steps1 = R.code_steps(rate, n_c)
        info1 = rs.randint(0, 2, size=(s_d, steps1 - 6))
        coded1 = R.conv_encode(info1, rate)
        syms1 = np.zeros((s_d, n_c), dtype=np.int8)
        syms1[:, perm[:coded1.shape[1]]] = 40 * (1 - 2 * coded1.astype(np.int8))
        for erased in (0, s_d - 1):
            got = syms.copy()
            got[erased] = 0
            bits, _ = R.viterbi_decode(got[j, at][None], rate)
            assert np.array_equal(bits[0, :steps - 6], info) and (bits[0, steps - 6:] == 0).all(), (rate, erased)
            got1 = syms1.copy()
            got1[erased] = 0
            bits1, metric1 = R.viterbi_decode(got1, rate, perm)
            keep = np.arange(s_d) != erased
            assert np.array_equal(bits1[keep, :steps1 - 6], info1[keep])
            # (nothing of the erased symbol's word is left: metric 0, and the decoder's answer is the all-zero word)
            assert metric1[erased] == 0 and not bits1[erased].any() and info1[erased].any(), (rate, erased)


def _small(S=None):
    c = dict(DC.case("n64_wtx_plain"))
    on = np.ones(64, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    return c, R.pilot_comb(on, 8), c["S"] if S is None else S


def test_the_mirrors_tracking_fields_are_the_tracking_mirrors():
    c, pil, S = _small()
    pts, tps = [L(cfo=0.02, cfo_tracked=0)] * 2, [TP(1, 1), TP(1, 0)]
    head = (c["st"], c["k"], S, c["w_tx"][:1], c["w_rx"][:1], c["h"][:1], c["snr"][:1], 5, 0, 2, pts, tps, pil, (0.5,))
    side = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    n_c = c["k"] * int((~pil if c["active"] is None else (np.asarray(c["active"]) != 0) & ~pil).sum())
    prof = R.rx_profile_coded_frame_host(*head, R.LLR_SCALE, R.default_interleaver(n_c), (0, 2), None, with_soft=True, **side)[0]
    trk = R.rx_profile_tracking_host(*head, **side)
    assert type(prof) is R.RxProfileCodedFrame
    for f in R.RxProfileTracking._fields:
        assert np.array_equal(getattr(prof, f), getattr(trk, f)), f
    assert prof.sym_rot == n_c // (S - 1) and prof.rates == (0, 2) and list(prof.codewords) == [2, 2]
    assert prof.info_bits.tolist() == [[R.code_steps(r, n_c * (S - 1 - q.post)) - 6 for r in (0, 2)] for q in tps]
    assert prof.info_err.shape == prof.cw_err.shape == (2, 1, 1, 1, 2) and (prof.cw_err <= 2).all()
    # the counts are the integer decoder's on the mirror's own soft bits, gathered through the frame interleaver
    pos = (8 * np.flatnonzero(~pil if c["active"] is None else (np.asarray(c["active"]) != 0) & ~pil)[:, None]
           + np.arange(c["k"])[None, :]).reshape(-1)
    for i, q in enumerate(tps):
        words = R.frame_codewords(prof.soft_bits[0, 0, 0, :, i], q.post, pos, R.default_interleaver(n_c), prof.sym_rot)
        assert words.shape == (2, n_c * (S - 1 - q.post))
        for jc, r in enumerate((0, 2)):
            bits, _ = R.viterbi_decode(words, r)
            assert prof.info_err[i, 0, 0, 0, jc] == bits[:, :-6].sum() and prof.cw_err[i, 0, 0, 0, jc] == bits.any(axis=1).sum()
    ber, fer = R.coded_frame_ber(prof), R.coded_fer(prof)
    assert ber.shape == fer.shape == prof.info_err.shape
    assert np.array_equal(fer, prof.cw_err / 2.0)
    assert np.array_equal(ber, prof.info_err / (2.0 * prof.info_bits[:, None, None, None, :]))


def test_one_data_symbol_without_rotation_is_the_per_symbol_mirror():
    c, pil, S = _small(S=2)
    n_c = c["k"] * int((~pil if c["active"] is None else (np.asarray(c["active"]) != 0) & ~pil).sum())
    # (an SNR at which the decoder errs: the counts are not all zero)
    head = (c["st"], c["k"], S, c["w_tx"][:1], c["w_rx"][:1], c["h"][:1], np.asarray([3.0], np.float32), 5, 0, 4,
            [L(cfo=0.02, cfo_tracked=0), L()], [TP(1, 0), TP(0, 0)], pil, (0.5,), R.LLR_SCALE, R.default_interleaver(n_c), (0, 1, 2))
    side = dict(active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])
    frm = R.rx_profile_coded_frame_host(*head, 0, **side)
    sym = R.rx_profile_coded_host(*head, **side)
    assert sym.info_err.shape[-1] == 1 and sym.info_err.any()
    assert np.array_equal(frm.info_err, sym.info_err[..., 0]) and np.array_equal(frm.cw_err, sym.cw_err[..., 0])
    for f in R.RxProfileTracking._fields:
        assert np.array_equal(getattr(frm, f), getattr(sym, f)), f
