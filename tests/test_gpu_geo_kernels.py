"""The kernels with a built geometry (wofdm_geo_table in csrc/wofdm_kernel.h, template parameter GEO of wofdm_frames_kernel)
against the kernels that read the same geometry at run time.

A built geometry changes where the structure lengths come from -- constants instead of scalar loads -- and nothing else: the same
statements on the same operands.  So a default plan (kernel_geo() > 0) and the same plan under the option generic_geometry
(kernel_geo() == 0) must give the same counters BIT FOR BIT, in all four counters of every cell; no tolerance in cases 1, 2 and 4.
Case 3 holds the built kernels against the oracle directly, by the rule of
tests/test_gpu_parity.py::test_every_spilling_production_kernel.

Shapes: 12 SNR points x 8 Veh-A channels = 96 cells with 1, 5 and 37 frames per cell (tests/test_gpu_work_split.py): with 37 a
workgroup's run crosses cells and there are more items than workgroups."""
import numpy as np
import pytest

import kernel_cases as KC
import wofdm_amd as W
from oracle import oracle as O
from test_geo_table import header_names

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
N_SNR, N_CH = 12, 8
N_FFT, CP, S, TAPS = 256, 32, 16, 21
STRUCTURES = header_names()                                            # ids 1 ... of wofdm_geo_table, as the header names them
FRAMES = (1, 5, 37)
CARRY = 2 ** 32 - 3                                                     # frame offset: three frames below the 32-bit carry
#: the benchmark's row (layout 10) and a row of the other layout (11)
C2, L11 = ("wtx", 4), ("wrx", 4)

_generic = {}                                                           # (system, k, off, F) -> counters of the generic plan


def _plan(channels, system, k, generic=False):
    st = W.make_structure(system, N_FFT, CP)
    snrs = np.linspace(-5, 50, N_SNR).astype(np.float32)
    cfg = W.make_cfg(st, k, S, TAPS, N_CH, N_SNR, 1, seed=SEED)
    plan = W.Plan(cfg, W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32),
                  channels[:N_CH].astype(np.complex64), snrs)
    if generic:
        plan.set_option("generic_geometry", 1)
    return plan


def _generic_counts(channels, monkeypatch, system, k, off, F):
    """The generic plan's counters, as the library ships (no split override); computed once, shared, never written to."""
    key = (system, k, off, F)
    if key not in _generic:
        monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
        monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
        with _plan(channels, system, k, generic=True) as plan:
            assert plan.kernel_geo() == 0
            got = plan.run(off, F)
        got.setflags(write=False)
        _generic[key] = got
    return _generic[key]


def _check_totals(got, k, F):
    assert np.array_equal(got[..., 1], np.full(got.shape[:-1], F * 15 * N_FFT * k))
    assert np.array_equal(got[..., 3], np.full(got.shape[:-1], F * 15 * N_FFT))


# ------------------------------------------------------------------------------------------------------------------
# 1. specialised against generic, every row and k
@pytest.mark.parametrize("k", [2, 4, 6])
@pytest.mark.parametrize("system", STRUCTURES)
def test_built_geometry_equals_run_time_geometry(channels, monkeypatch, system, k):
    monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
    monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
    st = W.make_structure(system, N_FFT, CP)
    cases = [(0, F) for F in FRAMES] + ([(CARRY, 37)] if (system, k) in (C2, L11) else [])
    with _plan(channels, system, k) as plan, _plan(channels, system, k, generic=True) as gen:
        assert plan.kernel_geo() == STRUCTURES.index(system) + 1 and gen.kernel_geo() == 0
        assert plan.kernel_id() == gen.kernel_id() == KC.expected_kernel_id(st, S, {}, 0)
        # a row's admission: the occupancy the runtime reports for its kernel (registers and LDS together) is the generic kernel's, three
        pi, gi = plan.info(), gen.info()
        print("%s k %d: workgroups per CU %d (generic %d), LDS %d bytes" % (system, k, pi["workgroups_per_cu"], gi["workgroups_per_cu"],
                                                                         pi["lds_bytes"]))
        assert pi["workgroups_per_cu"] == gi["workgroups_per_cu"] == 3
        assert pi["lds_bytes"] == gi["lds_bytes"] and pi["waves_per_workgroup"] == gi["waves_per_workgroup"]
        for off, F in cases:
            got = plan.run(off, F)
            want = _generic.setdefault((system, k, off, F), gen.run(off, F))
            print("%s k %d offset %d F %d: layout %d, bit errors %d / %d" % (system, k, off, F, plan.kernel_id()[0],
                                                                          got[..., 0].sum(), want[..., 0].sum()))
            assert np.array_equal(got, want)
            _check_totals(got, k, F)
            assert got[..., 0].sum() > 0
    want37, carry = _generic[(system, k, 0, 37)], _generic.get((system, k, CARRY, 37))
    assert carry is None or not np.array_equal(carry[..., 0], want37[..., 0])      # (other frames, other errors)


def test_both_layouts_are_among_the_rows():
    ids = {KC.expected_kernel_id(W.make_structure(s, N_FFT, CP), S, {}, 0)[0] for s in STRUCTURES}
    assert ids == {10, 11}
    for system, k in (C2, L11):
        assert KC.expected_kernel_id(W.make_structure(system, N_FFT, CP), S, {}, 0)[0] == (10 if (system, k) == C2 else 11)


# ------------------------------------------------------------------------------------------------------------------
# 2. the specialised kernel with a tail handed out in chunks
@pytest.mark.parametrize("system,k", [C2, L11])
def test_built_geometry_with_a_tail(channels, monkeypatch, system, k):
    F = 37
    want = _generic_counts(channels, monkeypatch, system, k, 0, F)
    monkeypatch.setenv("WOFDM_SPLIT_ALPHA", "0.5")
    monkeypatch.setenv("WOFDM_SPLIT_CHUNK", "3")
    with _plan(channels, system, k) as plan:
        assert plan.kernel_geo() > 0
        assert N_SNR * N_CH * F > plan.info()["workgroups"]             # more items than workgroups: the launch has a tail
        got = plan.run(0, F)
    assert np.array_equal(got, want)
    _check_totals(got, k, F)


# ------------------------------------------------------------------------------------------------------------------
# 3. against the oracle directly: the k = 4 rows, 12 cells x 70 frames (> 10^6 bits per cell)
@pytest.mark.parametrize("system", STRUCTURES)
def test_built_geometry_against_the_oracle(channels, system):
    k, F, seed, off = 4, 70, 8, 3
    st = W.make_structure(system, N_FFT, CP)
    w_tx, w_rx = W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32)
    snrs = np.array([5.0, 15.0, 25.0], np.float32)
    h = channels[11:15].astype(np.complex64)
    cfg = W.make_cfg(st, k, S, TAPS, 4, 3, 1, seed=seed)
    assert F * 15 * N_FFT * k > 1e6
    with W.Plan(cfg, w_tx, w_rx, h, snrs) as plan:
        assert plan.kernel_geo() == STRUCTURES.index(system) + 1
        got = plan.run(off, F)
    osys = O.make_sys(N_FFT, k, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, TAPS, 1)
    want = O.run(osys, w_tx.astype(np.float64), w_rx.astype(np.float64), h.astype(np.complex128),
                 snrs.astype(np.float64), seed, off, F)
    assert got[..., 0].size == 12
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])
    d = np.abs(got[..., 0].astype(np.int64) - want[..., 0].astype(np.int64))
    print("%s: bit errors %s, |diff| %s" % (system, want[..., 0].ravel(), d.ravel()))
    assert d.max() <= 12, (d, got[..., 0], want[..., 0])


# ------------------------------------------------------------------------------------------------------------------
# 4. what has no row keeps the kernel it had
@pytest.mark.parametrize("case", ["S12", "CP24", "allocation"])
def test_fallback_to_run_time_geometry(channels, case):
    syms, cp = (12 if case == "S12" else S), (24 if case == "CP24" else CP)
    var = 1 if case == "allocation" else 0
    st = W.make_structure("wtx", N_FFT, cp)
    snrs = np.array([5.0, 15.0, 25.0], np.float32)
    cfg = W.make_cfg(st, 4, syms, TAPS, 2, 3, 1, seed=SEED)
    F = 3
    with W.Plan(cfg, W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32),
                channels[:2].astype(np.complex64), snrs) as plan:
        active = np.ones(N_FFT, bool)
        if var:
            active[1::3] = False
            plan.set_allocation(active)
        assert plan.kernel_geo() == 0
        assert plan.kernel_id() == KC.expected_kernel_id(st, syms, {}, var) == (10, var)
        got = plan.run(0, F)
        if var:                                                         # ... and the row comes back with the allocation gone
            plan.set_allocation(None)
            assert plan.kernel_geo() == 1 and plan.kernel_id() == (10, 0)
    n_act = int(active.sum())
    assert np.array_equal(got[..., 1], np.full(got.shape[:-1], F * (syms - 1) * n_act * 4))
    assert np.array_equal(got[..., 3], np.full(got.shape[:-1], F * (syms - 1) * n_act))
    assert got[..., 0].sum() > 0
