"""``wofdm_rx_profile`` on the GPU (the Tx chain of wofdm_tx_papr with one job per (cell, frame), wofdm_rxprof_kernel<N>,
wofdm_rxprof_reduce_kernel<N>) against the CPU oracle: ``oracle.frame`` on ``oracle.gen_labels`` / ``gen_noise`` of (seed,
cell, frame), its ``labels_rx`` and ``Xhat`` reduced per bin (tests/rx_profile_cases.py) -- and, summed over the bins,
against the production frame kernels on the same cfg, seed and frame range.

Rules (rx_profile_cases.check_profile): per cell sum_n |sym_gpu - sym_ref| <= near and sum_n |bit_gpu - bit_ref| <= k near,
near = decisions whose fp64 Xhat lies within 1e-4 max(1, |Xhat|) max|Y0| / |Y0[n]| of a slicer threshold (at most 1 % of
the decisions by the choice of seed, an oracle-only property); unloaded bins exactly 0; |err_power - ref| <= POW_TOL (ref[n]
+ mean_n ref).  Against Plan.launch: the bins add up to counts[..., 0] within 2 k near and to counts[..., 2] within 2 near
(both kernels may tip a near decision, each its own way), the implied totals equal counts[..., 1] and counts[..., 3].

Measured on an MI355X: profiles/rx_profile.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def gpu_profile(n_fft, system, variant, nbt=1, cp=None):
    c, seed, _ = RC.reference(n_fft, system, variant, nbt, cp)
    return RC.run_gpu(c, seed, 0, RC.FRAMES)


def tag_of(n_fft, system, variant, c):
    return "N=%d %s %s S=%d k=%d B=%d" % (n_fft, system, variant, c["S"], c["k"], c["st"].stride)


@pytest.mark.parametrize("variant", RC.VARIANTS)
@pytest.mark.parametrize("system", RC.SYSTEMS)
@pytest.mark.parametrize("n_fft", RC.NS)
def test_profile_against_the_oracle(n_fft, system, variant):
    c, seed, ref = RC.reference(n_fft, system, variant)
    RC.check_profile(gpu_profile(n_fft, system, variant), ref, c, tag_of(n_fft, system, variant, c))


@pytest.mark.parametrize("n_fft,system,variant", ((64, "wtx", "masked"), (128, "CPW", "half"), (256, "CPW", "half_masked"),
                                                  (512, "wrx", "plain"), (1024, "wtx", "half")))
def test_noise_measured_over_the_truncated_signal(n_fft, system, variant):
    """noise_before_truncate = 0: Ps and Pn over S B samples"""
    c, seed, ref = RC.reference(n_fft, system, variant, 0)
    prof = gpu_profile(n_fft, system, variant, 0)
    RC.check_profile(prof, ref, c, tag_of(n_fft, system, variant, c) + " nbt=0")
    other = gpu_profile(n_fft, system, variant, 1)
    assert not np.array_equal(prof.err_power, other.err_power)


# every case at N <= 512 whose geometry the frame kernels take (cp + cs - tail_tx <= 64); wrx at N = 512 exceeds that at the
# matrix's CP 64 (stride - N = 69) and runs at CP 32 here (37, an odd stride), checked against the oracle as well
PLAN_CASES = [(n, s, v, None) for n in (64, 128, 256, 512) for s in RC.SYSTEMS for v in RC.VARIANTS
              if W.make_structure(s, n, RC.shape_of(n, s)[0]).stride - n <= 64] + [(512, "wrx", v, 32) for v in RC.VARIANTS]


@pytest.mark.parametrize("n_fft,system,variant,cp", PLAN_CASES)
def test_bins_add_up_to_the_production_counters(n_fft, system, variant, cp):
    c, seed, ref = RC.reference(n_fft, system, variant, 1, cp)
    prof = gpu_profile(n_fft, system, variant, 1, cp)
    if cp is not None:
        RC.check_profile(prof, ref, c, tag_of(n_fft, system, variant, c) + " cp=%d" % cp)
    st, k = c["st"], c["k"]
    cfg = W.make_cfg(st, k, c["S"], c["h"].shape[1], RC.N_CH, RC.N_SNR, RC.PAIRS, seed=seed)
    with W.Plan(cfg, c["w_tx"], c["w_rx"], c["h"], c["snr"]) as plan:
        if c["active"] is not None:
            plan.set_allocation(c["active"])
        if c["mask"] is not None:
            plan.set_tx_mask(c["mask"])
        counts = plan.run(0, RC.FRAMES).astype(np.int64)
        kid = plan.kernel_id()
    near = ref["near"]
    db = np.abs(prof.bit_err.sum(axis=-1).astype(np.int64) - counts[..., 0])
    ds = np.abs(prof.sym_err.sum(axis=-1).astype(np.int64) - counts[..., 2])
    print("%s: frame kernel %s, bit diff %s, sym diff %s, near %s" % (tag_of(n_fft, system, variant, c), kid, db.ravel(),
                                                                      ds.ravel(), near.ravel()))
    assert (db <= 2 * k * near).all() and (ds <= 2 * near).all()
    assert (counts[..., 3] == int(prof.decisions.sum())).all() and (counts[..., 1] == k * int(prof.decisions.sum())).all()


def test_split_frame_ranges_accumulate_to_one_call():
    c, seed, ref = RC.reference(256, "wtx", "half_masked")
    one = gpu_profile(256, "wtx", "half_masked")
    a = RC.run_gpu(c, seed, 0, 5)
    both = RC.run_gpu(c, seed, 5, 3, out=a)
    assert np.array_equal(both.bit_err, one.bit_err) and np.array_equal(both.sym_err, one.sym_err)
    assert np.array_equal(both.decisions, one.decisions)
    assert (both.bit_err >= a.bit_err).all() and both.bit_err.sum() > a.bit_err.sum()
    assert RC.pow_ratio(both.err_power, one.err_power) < 1e-12              # fp64 sums of the same fp32 frame sums


def test_repeated_calls_are_identical():
    for args in ((512, "CPW", "masked"), (64, "wrx", "half")):
        c, seed, _ = RC.reference(*args)
        a, b = gpu_profile(*args), RC.run_gpu(c, seed, 0, RC.FRAMES)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert a.err_power.tobytes() == b.err_power.tobytes()


def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32"""
    cp, S, k = RC.shape_of(128, "wtx")
    c = RC.make_case(W.make_structure("wtx", 128, cp), k, S, "plain", 77)
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    ref = RC.oracle_profile(c, seed, f0, 8)
    assert ref["near"].sum() <= 0.01 * ref["decisions"]
    prof = RC.run_gpu(c, seed, f0, 8)
    RC.check_profile(prof, ref, c, "keys beyond 32 bits")
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    assert not np.array_equal(RC.run_gpu(c, seed & 0xFFFFFFFF, f0, 8).bit_err, prof.bit_err)
    high, low = RC.run_gpu(c, seed, 2 ** 32, 5), RC.run_gpu(c, seed, 0, 5)
    assert not np.array_equal(high.bit_err, low.bit_err) and not np.array_equal(high.err_power, low.err_power)
    assert np.array_equal(RC.run_gpu(c, seed, f0, 3, ).bit_err + high.bit_err, prof.bit_err)


def test_a_frame_above_the_lds_limit_of_the_frame_kernels():
    """N = 1024, S = 16, cp + cs = 64: wofdm_plan_create refuses the frame, the profile runs it"""
    c, seed, ref = RC.reference_over_the_frame_limit()
    st = c["st"]
    cfg = W.make_cfg(st, c["k"], c["S"], c["h"].shape[1], RC.N_CH, RC.N_SNR, RC.PAIRS, seed=seed)
    with pytest.raises(_lib.WofdmError) as ei:
        W.Plan(cfg, c["w_tx"], c["w_rx"], c["h"], c["snr"])
    assert ei.value.code == -2 and "LDS" in str(ei.value)
    RC.check_profile(RC.run_gpu(c, seed, 0, RC.FRAMES), ref, c, "N=1024 S=16 cp+cs=64")


def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16: a chunk of the documented budget ends inside cell 1; the split changes no integer counter"""
    c, seed, _ = RC.reference_over_the_frame_limit()
    st, S = c["st"], c["S"]
    per_chunk = R.rx_profile_chunk_frames(st, S, False)
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (8 * (S * 1024 + st.frame_len(S) + 1024)) and 500 < per_chunk < 2000
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit
    one = RC.run_gpu(c, seed, 0, frames)
    assert int(one.decisions.max()) == frames * (S - 1)
    parts = RC.run_gpu(c, seed, frames - 7, 7, out=RC.run_gpu(c, seed, 0, frames - 7))
    assert np.array_equal(parts.bit_err, one.bit_err) and np.array_equal(parts.sym_err, one.sym_err)
    assert RC.pow_ratio(parts.err_power, one.err_power) < 1e-12
    assert R.rx_profile_kernel_ms() > 0.0


def test_profile_for_window_file_equals_its_host_route(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr = channels[:2], [8.0, 16.0]
    gpu = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=True, **kw)
    host = W.profile_for_window_file("wtx", 8, win, h, snr, gpu=False, **kw)
    assert list(gpu) == list(host) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        want, near = R.rx_profile_host(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, active=alloc, mask=mask, with_near=True)
        for i, name in enumerate(("opt", "rc")):
            g, hh = gpu[name][key], host[name][key]
            assert np.array_equal(hh.bit_err, want.bit_err[i]) and np.array_equal(hh.err_power, want.err_power[i])
            assert g.bit_err.shape == (2, 2, 64) and np.array_equal(g.decisions, hh.decisions)
            ds = np.abs(g.sym_err.astype(np.int64) - hh.sym_err.astype(np.int64)).sum(axis=-1)
            db = np.abs(g.bit_err.astype(np.int64) - hh.bit_err.astype(np.int64)).sum(axis=-1)
            assert (ds <= near[i]).all() and (db <= 4 * near[i]).all(), (name, key, ds, db, near[i])
            assert (g.bit_err[..., ~alloc] == 0).all() and (g.err_power[..., ~alloc] == 0).all()
            assert RC.pow_ratio(g.err_power, hh.err_power) <= RC.POW_TOL
