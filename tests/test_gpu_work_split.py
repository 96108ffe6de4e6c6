"""How a launch's frames are shared out among its workgroups (wofdm_work_split in csrc/wofdm_kernel.h, take_chunk in the frame
loop of csrc/wofdm_kernel.hip): a static head per workgroup, the rest in chunks through the plan's work counter.

The reference is free of all that: the same plan launched once per frame (frames_per_cell = 1).  Such a launch has no more
items than workgroups, so every workgroup holds at most one item and nothing is handed out.  Philox is keyed by the global
frame index and the counters are integer sums, so one launch of all the frames must give the same counters BIT FOR BIT, in
all four counters of every cell -- whatever the head's share (WOFDM_SPLIT_ALPHA) and the chunk (WOFDM_SPLIT_CHUNK), which
the library reads when a plan is created (tools/README.md); with either of them set, every launch with more items than
workgroups has a tail, however short it is.  No tolerance anywhere in this file."""
import numpy as np
import pytest

import kernel_cases as KC
import wofdm_amd as W

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
N_SNR, N_CH = 12, 8                              # 96 cells: 12 SNR points x 8 channels of the Veh-A fixture
#: (n_fft, k, layout): the benchmark's kernel; one symbol per wave, 16-wave workgroups, scalar error sums; one-wave workgroups
SHAPES = {"n256": (256, 4, 10), "n512": (512, 4, 12), "n64": (64, 2, 13)}

_refs = {}


def _plan(channels, shape, n_snr=N_SNR, n_ch=N_CH, seed=SEED):
    n_fft, k, layout = SHAPES[shape]
    system, cp, S, options = KC.geometry_for(n_fft, layout, 0)
    assert S == 16 and not options
    st = W.make_structure(system, n_fft, cp)
    snrs = np.linspace(-5, 50, n_snr).astype(np.float32)
    cfg = W.make_cfg(st, k, S, 21, n_ch, n_snr, 1, seed=seed)
    plan = W.Plan(cfg, W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32),
                  channels[:n_ch].astype(np.complex64), snrs)
    assert plan.kernel_id() == (layout, 0)
    return plan


def _per_frame(plan, off, F):
    """One launch per frame, all into one counter tensor."""
    import torch
    assert plan.cfg.n_cells <= plan.info()["workgroups"]          # at most one item per workgroup: nothing to share out
    counts = plan.new_counts()
    for f in range(F):
        plan.launch(off + f, 1, counts)
    torch.cuda.synchronize()
    plan.status()
    return counts.cpu().numpy().view(np.uint64)


def _reference(channels, monkeypatch, shape, off, F, n_snr=N_SNR, n_ch=N_CH):
    """Computed once per (shape, frames), shared, never written to."""
    key = (shape, off, F, n_snr, n_ch)
    if key not in _refs:
        monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
        monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
        with _plan(channels, shape, n_snr, n_ch) as plan:
            ref = _per_frame(plan, off, F)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _check_totals(got, shape, F):
    n_fft, k, _ = SHAPES[shape]
    assert np.array_equal(got[..., 1], np.full(got.shape[:-1], F * 15 * n_fft * k))       # every frame counted once
    assert np.array_equal(got[..., 3], np.full(got.shape[:-1], F * 15 * n_fft))


def _one_launch(channels, monkeypatch, shape, off, F, alpha, chunk, n_snr=N_SNR, n_ch=N_CH):
    monkeypatch.setenv("WOFDM_SPLIT_ALPHA", repr(alpha))
    monkeypatch.setenv("WOFDM_SPLIT_CHUNK", str(chunk))
    with _plan(channels, shape, n_snr, n_ch) as plan:
        return plan.run(off, F), plan.info()["workgroups"]


# ------------------------------------------------------------------------------------------------------------------
# chunks that span several cells: 96 cells of 1, 5, 37 frames; chunks of 1, 3, 16 and more than a cell; no head and half
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("chunk", [1, 3, 16, 64])
@pytest.mark.parametrize("F", [1, 5, 37])
def test_one_launch_equals_one_launch_per_frame(channels, monkeypatch, F, chunk, alpha):
    want = _reference(channels, monkeypatch, "n256", 0, F)
    got, grid = _one_launch(channels, monkeypatch, "n256", 0, F, alpha, chunk)
    assert chunk != 64 or chunk > F
    print("F %d chunk %d alpha %.2f: %d items on %d workgroups, bit errors %d" % (F, chunk, alpha, 96 * F, grid, got[..., 0].sum()))
    assert np.array_equal(got, want)
    _check_totals(got, "n256", F)
    assert got[..., 0].sum() > 0 and got[0, 0, 0, 0] > got[0, -1, 0, 0]


# ------------------------------------------------------------------------------------------------------------------
# item counts around a multiple of the grid: grid * 2 + r items, r = 0, 1, grid - 1, in the most cells that divide them
def _cells_for(total):
    best = (1, 1)
    for n_snr in range(1, N_SNR + 1):
        for n_ch in range(1, N_CH + 1):
            if total % (n_snr * n_ch) == 0 and n_snr * n_ch > best[0] * best[1]:
                best = (n_snr, n_ch)
    return best


@pytest.mark.parametrize("alpha,chunk", [(0.0, 3), (0.5, 16), (0.875, 1)])
@pytest.mark.parametrize("r", ["0", "1", "grid-1"])
def test_item_counts_around_a_multiple_of_the_grid(channels, monkeypatch, r, alpha, chunk):
    with _plan(channels, "n256") as plan:
        grid = plan.info()["workgroups"]
    total = 2 * grid + {"0": 0, "1": 1, "grid-1": grid - 1}[r]
    n_snr, n_ch = _cells_for(total)
    F = total // (n_snr * n_ch)
    want = _reference(channels, monkeypatch, "n256", 0, F, n_snr, n_ch)
    got, _ = _one_launch(channels, monkeypatch, "n256", 0, F, alpha, chunk, n_snr, n_ch)
    print("grid %d, %d items = %d x %d cells x %d frames, alpha %.3f chunk %d" % (grid, total, n_snr, n_ch, F, alpha, chunk))
    assert n_snr * n_ch * F == total
    assert np.array_equal(got, want)
    _check_totals(got, "n256", F)


# ------------------------------------------------------------------------------------------------------------------
def test_frame_offset_across_the_carry(channels, monkeypatch):
    """Chunks on both sides of frame 2^32: the chunk's frame index is re-derived per grab and added to a 64-bit offset."""
    off, F = 2 ** 32 - 17, 37
    want = _reference(channels, monkeypatch, "n256", off, F)
    got, _ = _one_launch(channels, monkeypatch, "n256", off, F, 0.5, 3)
    assert np.array_equal(got, want)
    _check_totals(got, "n256", F)
    assert not np.array_equal(got[..., 0], _reference(channels, monkeypatch, "n256", 0, F)[..., 0])


@pytest.mark.parametrize("shape", ["n512", "n64"])
def test_other_workgroup_shapes(channels, monkeypatch, shape):
    """N = 512 (layout 12: 16 waves, the run state beside scalar error sums) and N = 64 (layout 13: one-wave workgroups,
    where thread 0's wave is the whole workgroup), with more than two items per workgroup."""
    with _plan(channels, shape) as plan:
        info = plan.info()
    grid = info["workgroups"]
    F = (2 * grid + 95) // 96 + 1
    assert info["waves_per_workgroup"] == (16 if shape == "n512" else 1) and 96 * F > 2 * grid
    want = _reference(channels, monkeypatch, shape, 3, F)
    got, _ = _one_launch(channels, monkeypatch, shape, 3, F, 0.5, 3)
    print("%s: %d workgroups, %d frames per cell" % (shape, grid, F))
    assert np.array_equal(got, want)
    _check_totals(got, shape, F)
    # ... and as the library ships (no override)
    monkeypatch.delenv("WOFDM_SPLIT_ALPHA")
    monkeypatch.delenv("WOFDM_SPLIT_CHUNK")
    with _plan(channels, shape) as plan:
        assert np.array_equal(plan.run(3, F), want)


def test_the_split_as_shipped(channels, monkeypatch):
    """No override: launch() gives a launch a tail from WOFDM_SPLIT_MIN_ITEMS = 512 items per workgroup on (csrc/wofdm_kernel.h),
    with the shipped share and chunk.  513 items per workgroup, and 96 more."""
    monkeypatch.delenv("WOFDM_SPLIT_ALPHA", raising=False)
    monkeypatch.delenv("WOFDM_SPLIT_CHUNK", raising=False)
    with _plan(channels, "n256") as plan:
        info = plan.info()
        assert info["workgroups_per_cu"] >= 2
        F = (513 * info["workgroups"] + 95) // 96 + 1
        got = plan.run(0, F)
    want = _reference(channels, monkeypatch, "n256", 0, F)
    print("%d workgroups, %d frames per cell, %d items per workgroup" % (info["workgroups"], F, 96 * F // info["workgroups"]))
    assert 96 * F // info["workgroups"] >= 513
    assert np.array_equal(got, want)
    _check_totals(got, "n256", F)


def test_two_launches_on_one_plan(channels, monkeypatch):
    """The work counter is the plan's and is zeroed in front of every launch: two launches into one counter tensor, back to
    back on one stream, against the same two launches on a fresh plan each."""
    import torch
    F = 37
    monkeypatch.setenv("WOFDM_SPLIT_ALPHA", "0.5")
    monkeypatch.setenv("WOFDM_SPLIT_CHUNK", "3")
    with _plan(channels, "n256") as plan:
        counts = plan.new_counts()
        plan.launch(0, F, counts)
        plan.launch(F, F, counts)
        torch.cuda.synchronize()
        plan.status()
        both = counts.cpu().numpy().view(np.uint64)
        third = plan.run(0, F)                                    # (and a third, on its own)
    fresh = []
    for off in (0, F):
        with _plan(channels, "n256") as plan:
            fresh.append(plan.run(off, F))
    assert np.array_equal(both, fresh[0] + fresh[1])
    assert np.array_equal(third, fresh[0])
    assert np.array_equal(fresh[0], _reference(channels, monkeypatch, "n256", 0, F))
    _check_totals(both, "n256", 2 * F)


def test_inject_mode(channels, monkeypatch):
    """Injected labels and noise are addressed by (cell, frame of the cell): a chunk must find its rows."""
    import torch
    F = 9
    g = torch.Generator(device="cuda").manual_seed(5)

    def run(alpha, chunk, per_frame):
        monkeypatch.setenv("WOFDM_SPLIT_ALPHA", repr(alpha))
        monkeypatch.setenv("WOFDM_SPLIT_CHUNK", str(chunk))
        with _plan(channels, "n256") as plan:
            cells, nl = plan.cfg.n_cells, plan.noise_len
            assert cells * F > plan.info()["workgroups"] >= cells
            g.manual_seed(5)
            labels = torch.randint(0, 16, (cells, F, 16, 256), dtype=torch.uint8, device="cuda", generator=g)
            noise = torch.randn((cells, F, nl, 2), dtype=torch.float32, device="cuda", generator=g) * 0.70710678
            counts = plan.new_counts()
            if per_frame:
                for f in range(F):
                    plan.launch_injected(1, labels[:, f:f + 1].contiguous(), noise[:, f:f + 1].contiguous(), counts)
            else:
                plan.launch_injected(F, labels, noise, counts)
            torch.cuda.synchronize()
            plan.status()
            return counts.cpu().numpy().view(np.uint64)

    want = run(0.5, 3, True)
    assert np.array_equal(run(0.5, 3, False), want)
    assert np.array_equal(run(0.0, 16, False), want)
    _check_totals(want, "n256", F)
    assert want[..., 0].sum() > 0


def test_overrides_out_of_range_are_refused(channels, monkeypatch):
    for name, bad in (("WOFDM_SPLIT_ALPHA", "1.0"), ("WOFDM_SPLIT_ALPHA", "-0.1"), ("WOFDM_SPLIT_CHUNK", "0")):
        monkeypatch.setenv(name, bad)
        with pytest.raises(W._lib.WofdmError):
            _plan(channels, "n256")
        monkeypatch.delenv(name)
