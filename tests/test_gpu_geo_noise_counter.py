"""The lane constants and the scalar-unit Philox head of the kernels with a built geometry (philox_head2 in csrc/wofdm_kernel.hip)
against the kernels that read the same geometry at run time.

The built kernels form a noise tile's Philox block from a lane constant made ONCE per kernel plus a wave-uniform addend, draw the
data bits' block the same way, and run the wave-uniform half of rounds 1 ... 3 on the scalar unit.  They have no dump instantiation,
so the four counters are the observable, and the unchanged generic kernel of the same plan (option generic_geometry) is the
reference: a wrong block, key or label moves the error counts with near certainty at -5 and 5 dB.  Everything is np.array_equal.

Shapes: wtx (layout 10, even stride) and wrx (layout 11, odd stride), k = 2, 4, 6, two SNR points x two channels = 4 cells.  Every
tile index, the trailing tile and the data-bit branch run in every frame, so the smallest shapes check them; what they must add is
  * a cell change inside a workgroup's run (3 frames per cell) at frame offsets around the 32-bit carry and beyond 2^40: the
    frame words of the counter are the uniform half the head computes;
  * a launch with a dynamic tail (at least 512 items per workgroup): the lane constants live across the outer chunk loop;
  * two launches through one plan: constants that are hoisted, but clobbered, show in the second."""
import numpy as np
import pytest

import wofdm_amd as W

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
N_FFT, CP, S, TAPS = 256, 32, 16, 21
SNRS = np.array([-5.0, 5.0], np.float32)
N_CH = 2
OFFSETS = (0, 2 ** 32 - 3, 2 ** 40 + 5)
CASES = [(system, k) for system in ("wtx", "wrx") for k in (2, 4, 6)]


def _plan(channels, system, k, generic):
    st = W.make_structure(system, N_FFT, CP)
    cfg = W.make_cfg(st, k, S, TAPS, N_CH, len(SNRS), 1, seed=SEED)
    plan = W.Plan(cfg, W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32),
                  channels[:N_CH].astype(np.complex64), SNRS)
    if generic:
        plan.set_option("generic_geometry", 1)
    return plan


def _totals(got, k, F):
    assert np.array_equal(got[..., 1], np.full(got.shape[:-1], F * (S - 1) * N_FFT * k))
    assert np.array_equal(got[..., 3], np.full(got.shape[:-1], F * (S - 1) * N_FFT))
    assert got[..., 0].sum() > 0 and got[..., 2].sum() > 0


@pytest.mark.parametrize("system,k", CASES)
def test_cells_change_inside_a_run_at_every_offset(channels, monkeypatch, system, k):
    monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
    monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
    F = 3
    seen = []
    with _plan(channels, system, k, False) as plan, _plan(channels, system, k, True) as gen:
        assert plan.kernel_geo() > 0 and gen.kernel_geo() == 0
        for off in OFFSETS:
            got, want = plan.run(off, F), gen.run(off, F)
            print("%s k %d offset %d: bit errors %s / generic %s" % (system, k, off, got[..., 0].ravel(), want[..., 0].ravel()))
            assert np.array_equal(got, want)
            _totals(got, k, F)
            seen.append(got[..., 0].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])      # (other frames, other errors)


@pytest.mark.parametrize("system,k", CASES)
def test_a_launch_with_a_dynamic_tail(channels, monkeypatch, system, k):
    monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
    monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
    with _plan(channels, system, k, False) as plan, _plan(channels, system, k, True) as gen:
        assert plan.kernel_geo() > 0 and gen.kernel_geo() == 0
        wgs = plan.info()["workgroups"]
        cells = len(SNRS) * N_CH
        F = (520 * wgs + cells - 1) // cells
        assert cells * F >= 512 * wgs                                       # the launch is given a tail (WOFDM_SPLIT_MIN_ITEMS)
        got, want = plan.run(7, F), gen.run(7, F)
    print("%s k %d: %d workgroups, %d frames per cell, bit errors %s" % (system, k, wgs, F, got[..., 0].ravel()))
    assert np.array_equal(got, want)
    _totals(got, k, F)


@pytest.mark.parametrize("system,k", CASES)
def test_two_launches_through_one_plan(channels, monkeypatch, system, k):
    monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
    monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
    F = 3
    with _plan(channels, system, k, False) as plan, _plan(channels, system, k, True) as gen:
        assert plan.kernel_geo() > 0 and gen.kernel_geo() == 0
        first, second = plan.run(11, F), plan.run(11, F)
        want = gen.run(11, F)
    assert np.array_equal(first, want) and np.array_equal(second, want)
    _totals(first, k, F)
