"""The receive profile and the frame kernels on the GPU at the documented limits of their geometry (tests/edge_geometry_cases.py:
tail_rx = 64, a window that folds a quarter to all of the symbol, cp = cs = n_fft, 2 tail_tx near P, circ_shift up to 48, 1 ... 21
taps, CPwtx and CPwrx), where no other GPU test goes.

a. ``wofdm_rx_profile`` on all eleven cases against the CPU oracle under ``rx_profile_cases.check_profile``, unchanged: per cell
   sum_n |sym_gpu - sym_ref| <= near and sum_n |bit_gpu - bit_ref| <= k near, unloaded bins exactly 0, |err_power - ref| <= POW_TOL
   (ref[n] + mean_n ref) with POW_TOL = 1e-3; a second call returns the same bytes.
b. The seven cases ``wofdm_plan_create`` takes through ``Plan.run``: counts[..., 1] and counts[..., 3] exact, |counts[..., 0] -
   oracle| <= k near and |counts[..., 2] - oracle| <= near per cell, the kernel ``kernel_cases.expected_kernel_id`` names, status OK;
   again with the plan options dft_valu and fir_valu (within 2 k near and 2 near of the default: each kernel may tip a near decision
   its own way; an option the geometry does not support is reported and left out); the profile's bins add up to the default plan's
   counters under tests/test_gpu_rx_profile.py's rule.
c. The four other cases are refused by ``W.Plan`` with WOFDM_E_UNSUPPORTED, and the profile runs them (a).
d. ``wofdm_rx_profile_link`` on three cases with two composed points (everything on, the first window before the frame at one, a
   neighbour delay of B - 1) against ``rx_profile_link_host`` under tests/test_gpu_rx_profile_link.py's ``check_points``; an all-off
   point behind them in the same call returns the bytes of ``wofdm_rx_profile``.  On fold_all_n64 ``wofdm_rx_profile_tracking`` with
   the receiver (1, 1) on the same points against ``rx_profile_tracking_host`` under tests/test_gpu_rx_profile_tracking.py's
   ``check_tracking``.

Every near count is the reference's own (at most 1 % of the decisions by the choice of seed, asserted on the CPU in
tests/test_edge_geometry_host.py).  Measured on an MI355X: profiles/edge_geometry.txt."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import rx_profile as R

import edge_geometry_cases as EC
import kernel_cases as KC
import rx_profile_cases as RC
import test_gpu_rx_profile_link as TL
import test_gpu_rx_profile_tracking as TT

pytestmark = pytest.mark.gpu

L = R.LinkPoint


@functools.lru_cache(maxsize=None)
def gpu_profile(name, seed):
    return RC.run_gpu(EC.case(name), seed, 0, RC.FRAMES)


def tag_of(name, c, seed):
    st = c["st"]
    return "%s N=%d %s S=%d k=%d B=%d P=%d gamma=%d kappa=%d taps=%d seed=%d" % (
        name, st.n_fft, st.system, c["S"], c["k"], st.stride, st.sym_len, st.prefix_rm, st.circ_shift, c["h"].shape[1], seed)


# ---- a. the receive profile against the oracle ----

@pytest.mark.parametrize("name", list(EC.CASES))
def test_profile_against_the_oracle(name):
    c, seed, ref = EC.reference(name)
    prof = gpu_profile(name, seed)
    RC.check_profile(prof, ref, c, tag_of(name, c, seed))
    assert np.array_equal(prof.decisions, np.where(np.ones(c["st"].n_fft, bool) if c["active"] is None else c["active"],
                                                   RC.FRAMES * (c["S"] - 1), 0))
    again = RC.run_gpu(c, seed, 0, RC.FRAMES)
    assert TL.same_bits(prof, again)


# ---- b. the frame kernels against the oracle ----

def run_plan(c, seed, opts):
    """(counts, kernel id) of the case's frames through a plan with the options `opts`; None where the geometry does not support one"""
    st = c["st"]
    cfg = W.make_cfg(st, c["k"], c["S"], c["h"].shape[1], RC.N_CH, RC.N_SNR, RC.PAIRS, noise_before_truncate=bool(c["nbt"]), seed=seed)
    with W.Plan(cfg, c["w_tx"], c["w_rx"], c["h"], c["snr"]) as plan:
        try:
            for key, val in opts.items():
                plan.set_option(key, val)
            if c["active"] is not None:
                plan.set_allocation(c["active"])
            if c["mask"] is not None:
                plan.set_tx_mask(c["mask"])
        except _lib.WofdmError as e:
            if not opts or e.code != -2:
                raise
            return None
        counts = plan.run(0, RC.FRAMES).astype(np.int64)
        plan.status()
        return counts, plan.kernel_id()


@pytest.mark.parametrize("name", EC.PLAN_CASES)
def test_frame_kernels_against_the_oracle(name):
    c, seed, ref = EC.reference(name)
    st, k, near, tag = c["st"], c["k"], ref["near"], tag_of(name, c, seed)
    want = ref["counts"].astype(np.int64)
    counts, kid = run_plan(c, seed, {})
    db, ds = np.abs(counts[..., 0] - want[..., 0]), np.abs(counts[..., 2] - want[..., 2])
    print("%s: frame kernel %s, bit diff %s, sym diff %s, near %s" % (tag, kid, db.ravel(), ds.ravel(), near.ravel()))
    assert np.array_equal(counts[..., 1], want[..., 1]) and np.array_equal(counts[..., 3], want[..., 3])
    assert (db <= k * near).all() and (ds <= near).all()
    assert kid == KC.expected_kernel_id(st, c["S"], None, EC.plan_var(c))
    # the matrix-pipe and the VALU forms
    for opts in ({"dft_valu": 1}, {"fir_valu": 1}):
        res = run_plan(c, seed, opts)
        if res is None:
            print("%s: %s is not supported for this geometry (WOFDM_E_UNSUPPORTED): arm left out" % (tag, opts))
            continue
        other, oid = res
        db, ds = np.abs(other[..., 0] - counts[..., 0]), np.abs(other[..., 2] - counts[..., 2])
        print("%s: %s: frame kernel %s, against the default: bit diff %s, sym diff %s" % (tag, opts, oid, db.ravel(), ds.ravel()))
        assert oid == KC.expected_kernel_id(st, c["S"], opts, EC.plan_var(c))
        assert np.array_equal(other[..., 1], want[..., 1]) and np.array_equal(other[..., 3], want[..., 3])
        assert (db <= 2 * k * near).all() and (ds <= 2 * near).all()
    # the profile's bins add up to the default plan's counters (test_bins_add_up_to_the_production_counters' rule)
    prof = gpu_profile(name, seed)
    db = np.abs(prof.bit_err.sum(axis=-1).astype(np.int64) - counts[..., 0])
    ds = np.abs(prof.sym_err.sum(axis=-1).astype(np.int64) - counts[..., 2])
    print("%s: profile bins against the plan: bit diff %s, sym diff %s" % (tag, db.ravel(), ds.ravel()))
    assert (db <= 2 * k * near).all() and (ds <= 2 * near).all()
    assert (counts[..., 3] == int(prof.decisions.sum())).all() and (counts[..., 1] == k * int(prof.decisions.sum())).all()


# ---- c. the geometries the frame kernels refuse ----

@pytest.mark.parametrize("name", EC.REFUSED_CASES)
def test_the_plan_refuses_what_the_profile_runs(name):
    c, seed, ref = EC.reference(name)
    cfg = W.make_cfg(c["st"], c["k"], c["S"], c["h"].shape[1], RC.N_CH, RC.N_SNR, RC.PAIRS, noise_before_truncate=bool(c["nbt"]),
                     seed=seed)
    with pytest.raises(_lib.WofdmError) as ei:
        W.Plan(cfg, c["w_tx"], c["w_rx"], c["h"], c["snr"])
    print("%s: %s" % (name, ei.value))
    assert ei.value.code == -2
    prof = gpu_profile(name, seed)
    assert (prof.bit_err.sum(axis=-1) > 0).all() and int(prof.decisions.sum()) * 8 == ref["decisions"]


# ---- d. the combined chain ----

@pytest.mark.parametrize("name", list(EC.LINK_CASES))
def test_composed_points_against_the_mirror(name):
    c, seed, ref, near = EC.link_reference(name)
    st, nc = c["st"], len(c["points"])
    allp = W.rx_profile_link_gpu(*EC.head(c, seed), c["points"] + [L()], **EC.link_sides(c, seed))
    prof = R.RxProfileLink(*(a[:nc] for a in allp[:-1]), allp.decisions)
    tag = tag_of(name, c, seed) + " link"
    print("%s: near shares per point %s" % (tag, np.round(near.sum(axis=(1, 2, 3)) / TL.decisions_of(c, RC.FRAMES), 4)))
    TL.check_points(prof, ref, near, c, RC.FRAMES, tag)
    # the all-off point is wofdm_rx_profile, by bytes
    plain = gpu_profile(name, seed)
    assert TL.same_bits([a[nc] for a in allp[:3]], plain[:3]) and np.array_equal(allp.decisions, plain.decisions)
    for i in range(nc):
        assert (np.abs(allp.err_power[i] - allp.err_power[nc]).max(axis=-1) > 0).all(), i


def test_tracking_where_the_whole_window_folds():
    c, seed, ref, near = EC.tracking_reference()
    prof = W.rx_profile_tracking_gpu(*EC.head(c, seed), c["points"], c["tracking"], c["pilots"], EC.TRACKING_SCALES,
                                     **EC.link_sides(c, seed))
    TT.check_tracking(prof, ref, near, c, tag_of(c["name"], c, seed) + " tracking")
