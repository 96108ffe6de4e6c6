"""``wofdm_rx_profile_aci`` on the GPU (two passes through the Tx chain of wofdm_rx_profile, wofdm_rxprof_aci_kernel<N>,
wofdm_rxprof_reduce_kernel<N>) against the fp64 host route ``rx_profile_aci_host``: the same frames, the same neighbour,
from the same Philox streams (the mirror itself is tied to the CPU oracle in tests/test_rx_profile_aci_host.py).

Rules: those of rx_profile_cases.check_profile, with the mirror in the oracle's place -- per cell sum_n |sym_gpu - sym_ref| <=
near and sum_n |bit_gpu - bit_ref| <= k near, unloaded bins exactly 0, |err_power - ref| <= POW_TOL (ref[n] + mean_n ref).
The seed of a case is the first from its base seed on, of 32, for which the mirror alone has at most 1 % near decisions
(``RC.pick_seed``'s cap, decided on the CPU).  No case needed another SNR pair than ``RC.SNR_DB``'s.

Measured on an MI355X: profiles/rx_profile_aci.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC

pytestmark = pytest.mark.gpu


def thirds(n):
    """victim on the lower third of the bins, neighbour on the upper third (bin n - 1 is bin 0's neighbour), the middle free"""
    v, a = np.zeros(n, bool), np.zeros(n, bool)
    v[:n // 3] = True
    a[n - n // 3:] = True
    return v, a


#: name -> (n_fft, system, cp, k, S, allocation, masked, delay (callable of B), level_db, rolled aci_h, nbt)
CASES = {
    "n64_wtx_half_d1": (64, "wtx", 8, 2, 4, "half", False, lambda B: 1, 0.0, False, 1),
    "n128_wrx_thirds_dBm1": (128, "wrx", 16, 2, 9, "thirds", False, lambda B: B - 1, 0.0, False, 1),
    "n256_cpw_half_masked_dhalf": (256, "CPW", 32, 6, 16, "half", True, lambda B: B // 2, 0.0, True, 1),
    "n512_wola_half_d0": (512, "WOLA", 64, 4, 3, "half", False, lambda B: 0, 0.0, False, 1),
    "n1024_wtx_half_masked_d7": (1024, "wtx", 128, 4, 2, "half", True, lambda B: 7, 0.0, False, 1),
    "n128_cpw_half_nbt0": (128, "CPW", 32, 4, 4, "half", False, lambda B: 33, 0.0, True, 0),
    "n64_cpw_half_m20dB": (64, "CPW", 32, 4, 5, "half", False, lambda B: 21, -20.0, False, 1),
    "n64_wrx_half_masked_p10dB": (64, "wrx", 8, 2, 6, "half", True, lambda B: 40, 10.0, True, 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    n, system, cp, k, S, alloc, masked, delay, level, rolled, nbt = CASES[name]
    st = W.make_structure(system, n, cp)
    c = RC.make_case(st, k, S, "masked" if masked else "plain", 4000 + n + len(name), nbt)
    if alloc == "half":
        c["active"] = CM.half_band_allocation(n)
        c["aci_active"] = ~c["active"]
    else:
        c["active"], c["aci_active"] = thirds(n)
    c["delay"], c["level"] = int(delay(st.stride)), level
    c["aci_h"] = np.roll(c["h"], 1, axis=0) if rolled else None
    assert 0 <= c["delay"] < st.stride
    return c


def host(c, seed, frame_offset, frames):
    """the mirror's profile as the dict check_profile reads"""
    prof, near = R.rx_profile_aci_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset,
                                       frames, c["aci_active"], c["delay"], c["level"], c["aci_h"], active=c["active"],
                                       mask=c["mask"], noise_before_truncate=c["nbt"], with_near=True)
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    return dict(bit=prof.bit_err.astype(np.int64), sym=prof.sym_err.astype(np.int64), pow=prof.err_power, near=near,
                decisions=cells * frames * (c["S"] - 1) * int(np.count_nonzero(c["active"])))


def pick_seed(c, base_seed, frame_offset=0, frames=RC.FRAMES, tries=32):
    """first seed from base_seed on whose MIRROR profile has at most 1 % near decisions (RC.pick_seed's cap)"""
    for seed in range(base_seed, base_seed + tries):
        ref = host(c, seed, frame_offset, frames)
        if ref["near"].sum() <= 0.01 * ref["decisions"]:
            return seed, ref
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (base_seed, base_seed + tries))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    seed, ref = pick_seed(c, 100 * (1 + list(CASES).index(name)))
    return c, seed, ref


def run_gpu(c, seed, frame_offset, frames, **kw):
    args = dict(aci_active=c["aci_active"], aci_delay=c["delay"], aci_level_db=c["level"], aci_h=c["aci_h"])
    args.update(kw)
    return W.rx_profile_aci_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], **args)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c, seed, _ = reference(name)
    return run_gpu(c, seed, 0, RC.FRAMES)


def tag_of(name, c):
    return "%s S=%d k=%d B=%d delay=%d level=%g" % (name, c["S"], c["k"], c["st"].stride, c["delay"], c["level"])


@pytest.mark.parametrize("name", list(CASES))
def test_profile_against_the_mirror(name):
    c, seed, ref = reference(name)
    prof = gpu_profile(name)
    RC.check_profile(prof, ref, c, tag_of(name, c))
    assert np.array_equal(prof.decisions, np.where(c["active"], RC.FRAMES * (c["S"] - 1), 0))
    # the neighbour is on the air: the same frames without it give another result, on every cell (no ordering is asserted:
    # the sums are led by a few faded bins, whose pilots the neighbour moves as well)
    alone = RC.run_gpu(c, seed, 0, RC.FRAMES)
    assert (np.abs(alone.err_power - prof.err_power).max(axis=-1) > 0).all()


@pytest.mark.parametrize("name", ("n64_wtx_half_d1", "n256_cpw_half_masked_dhalf"))
def test_an_empty_neighbour_allocation_is_the_plain_call(name):
    c, seed, _ = reference(name)
    a = run_gpu(c, seed, 0, RC.FRAMES, aci_active=np.zeros(c["st"].n_fft, bool))
    b = RC.run_gpu(c, seed, 0, RC.FRAMES)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a.err_power.tobytes() == b.err_power.tobytes()


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked_dhalf"
    c, seed, _ = reference(name)
    one = gpu_profile(name)
    a = run_gpu(c, seed, 0, 5)
    both = run_gpu(c, seed, 5, 3, out=a)
    assert np.array_equal(both.bit_err, one.bit_err) and np.array_equal(both.sym_err, one.sym_err)
    assert np.array_equal(both.decisions, one.decisions)
    assert (both.bit_err >= a.bit_err).all() and both.bit_err.sum() > a.bit_err.sum()
    assert RC.pow_ratio(both.err_power, one.err_power) < 1e-12              # fp64 sums of the same fp32 frame sums


def test_repeated_calls_are_identical():
    for name in ("n512_wola_half_d0", "n64_wrx_half_masked_p10dB"):
        c, seed, _ = reference(name)
        a, b = gpu_profile(name), run_gpu(c, seed, 0, RC.FRAMES)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert a.err_power.tobytes() == b.err_power.tobytes()


def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32, in stream 2 as well"""
    c = dict(case("n128_cpw_half_nbt0"))
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    ref = host(c, seed, f0, 8)
    assert ref["near"].sum() <= 0.01 * ref["decisions"]
    prof = run_gpu(c, seed, f0, 8)
    RC.check_profile(prof, ref, c, "keys beyond 32 bits")
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    assert not np.array_equal(run_gpu(c, seed & 0xFFFFFFFF, f0, 8).bit_err, prof.bit_err)
    high, low = run_gpu(c, seed, 2 ** 32, 5), run_gpu(c, seed, 0, 5)
    assert not np.array_equal(high.bit_err, low.bit_err) and not np.array_equal(high.err_power, low.err_power)
    assert np.array_equal(run_gpu(c, seed, f0, 3).bit_err + high.bit_err, prof.bit_err)


def test_aci_for_window_file_equals_its_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr, delays = channels[:2], [8.0, 16.0], (0, 37)
    gpu = W.aci_for_window_file("wtx", 8, win, h, snr, delays, -3.0, gpu=True, **kw)
    hst = W.aci_for_window_file("wtx", 8, win, h, snr, delays, -3.0, gpu=False, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for d in delays:
        for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
            want, near = R.rx_profile_aci_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, ~alloc, d, -3.0, active=alloc, mask=mask,
                                               with_near=True)
            for i, name in enumerate(("opt", "rc")):
                assert list(gpu[name]) == list(hst[name]) == list(delays)
                g, hh = gpu[name][d][key], hst[name][d][key]
                assert np.array_equal(hh.bit_err, want.bit_err[i]) and np.array_equal(hh.err_power, want.err_power[i])
                assert g.bit_err.shape == (2, 2, 64) and np.array_equal(g.decisions, hh.decisions)
                ds = np.abs(g.sym_err.astype(np.int64) - hh.sym_err.astype(np.int64)).sum(axis=-1)
                db = np.abs(g.bit_err.astype(np.int64) - hh.bit_err.astype(np.int64)).sum(axis=-1)
                assert (ds <= near[i]).all() and (db <= 4 * near[i]).all(), (name, d, key, ds, db, near[i])
                assert (g.bit_err[..., ~alloc] == 0).all() and (g.err_power[..., ~alloc] == 0).all()
                assert RC.pow_ratio(g.err_power, hh.err_power) <= RC.POW_TOL


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64: a chunk of the documented budget ends inside a cell; the split changes no integer
    counter"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    c.update(active=CM.half_band_allocation(1024), aci_active=~CM.half_band_allocation(1024), delay=501, level=0.0, aci_h=None)
    B, Tv = st.stride, st.frame_len(S)
    per_chunk = R.rx_profile_aci_chunk_frames(st, S, False)
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + (S + 1) * 1024 + Tv + (Tv + B) + 1024))
    assert 250 < per_chunk < R.rx_profile_chunk_frames(st, S, False)
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit
    one = run_gpu(c, 7000, 0, frames)
    assert int(one.decisions.max()) == frames * (S - 1)
    parts = run_gpu(c, 7000, frames - 7, 7, out=run_gpu(c, 7000, 0, frames - 7))
    assert np.array_equal(parts.bit_err, one.bit_err) and np.array_equal(parts.sym_err, one.sym_err)
    assert RC.pow_ratio(parts.err_power, one.err_power) < 1e-12
    assert R.rx_profile_kernel_ms() > 0.0
