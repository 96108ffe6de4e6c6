"""Every instantiation of the frame kernel, by kernel id, against the CPU oracle.

profiles/kernel_table.json lists the 756 kernels wofdm_frames_kernel<N, K, LAY, INJECT, DUMP, VAR> is built as.  Which one a
plan launches is decided by configure() (csrc/wofdm_abi.hip) from the geometry and the plan options; kernel_cases.py has a
geometry for every row.  Each case below first asserts that the plan really picked the row's kernel (plan.kernel_id()), then
compares what it computes with the oracle on the same Philox streams: the 378 production kernels on their error counters,
the 378 instrumented kernels one frame stage by stage -- the counters cannot see an error of 1e-3 in one window-tail sample,
the stage dumps at 2e-5 can."""
import numpy as np
import pytest

import kernel_cases as KC
import wofdm_amd as W
from oracle import oracle as O
from test_gpu_channel_mask import _check_decisions
from wofdm_amd import channel_mask as CM

pytestmark = pytest.mark.gpu

STAGE_RTOL = 2e-5          # fp32 chain of an N<=1024 FFT + 21-tap FIR vs fp64, relative to max|x| (test_gpu_parity.py)
PRODUCTION, DUMP = KC.production_rows(), KC.dump_rows()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _osys(st, k, S, matlab, active=None, mask=None):
    return O.make_sys(st.n_fft, k, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, 21,
                      1 if matlab else 0, active=active,
                      tx_mask=None if mask is None else mask.astype(np.float32).astype(np.float64))


def _allocation_and_mask(st, k, layout, var):
    """Allocation (random, 60 % of the bins, bin 0 loaded) and Tx mask of a row, as test_every_spilling_production_kernel."""
    rs = np.random.RandomState(st.n_fft + 7 * k + layout)
    active = None
    if var >= 1:
        active = rs.rand(st.n_fft) < 0.6
        active[0] = True
    mask = CM.tx_mask(st.sym_len, roll_off=10) if var >= 2 else None
    return active, mask


def _configure(plan, options, active, mask, layout, var):
    for key, val in options.items():
        plan.set_option(key, val)
    if active is not None:
        plan.set_allocation(active)
    if mask is not None:
        plan.set_tx_mask(mask)
    assert plan.kernel_id() == (layout, var), (plan.kernel_id(), layout, var)


# ------------------------------------------------------------------------------------------------------------------
# production kernels: error counters
def production_case(row):
    """Everything of a production row's case that does not need the GPU (also what the floor of expected errors was checked
    with on the CPU)."""
    n_fft, k, layout, inject, var = row
    system, cp, S, options = KC.geometry_for(n_fft, layout, var)
    st = W.make_structure(system, n_fft, cp)
    # bits per cell as test_every_spilling_production_kernel has them, for every row.  (Measured on an MI355X in one visit: this
    # module 68 s at these sizes, 55 s with the non-spilling rows cut to 1e6, the rest of the GPU suite 94 s -- no reason to cut.)
    bits = 1e6 if var >= 2 else (2e6 if inject else 4e6)
    F = max(4, int(bits / ((S - 1) * n_fft * k)))
    matlab = KC.noise_before_truncate(row)        # both noise orders in both modes for every (n_fft, layout, var)
    active, mask = _allocation_and_mask(st, k, layout, var)
    snrs = np.array([5.0, 15.0, 25.0], np.float32) + (k - 4) * 3.0     # BER 0.3 ... 0.01 for every k
    return dict(st=st, S=S, options=options, F=F, matlab=matlab, active=active, mask=mask, snrs=snrs, seed=8, off=3,
                osys=_osys(st, k, S, matlab, active, mask),
                w_tx=W.tx_rc_window(st).astype(np.float32), w_rx=W.rx_rc_window(st).astype(np.float32))


def oracle_counts(c, h):
    return O.run(c["osys"], c["w_tx"].astype(np.float64), c["w_rx"].astype(np.float64), h.astype(np.complex128),
                 c["snrs"].astype(np.float64), c["seed"], c["off"], c["F"])


@pytest.mark.parametrize("row", PRODUCTION, ids=KC.row_id)
def test_production_kernel_against_oracle(channels, row):
    import torch
    n_fft, k, layout, inject, var = row
    c = production_case(row)
    st, S, F, seed, off, osys = c["st"], c["S"], c["F"], c["seed"], c["off"], c["osys"]
    cfg = W.make_cfg(st, k, S, 21, 2, 3, 1, noise_before_truncate=c["matlab"], seed=seed)
    h = channels[11:13].astype(np.complex64)
    with W.Plan(cfg, c["w_tx"], c["w_rx"], h, c["snrs"]) as plan:
        _configure(plan, c["options"], c["active"], c["mask"], layout, var)
        if inject:
            # the oracle's own Philox draws, handed over as injected data
            nl = O.noise_len(osys)
            assert nl == plan.noise_len
            labels = np.zeros((6, F, S, n_fft), np.uint8)
            noise = np.zeros((6, F, nl), np.complex64)
            for cell in range(6):
                for f in range(F):
                    labels[cell, f] = O.gen_labels(osys, seed, cell, off + f)
                    noise[cell, f] = O.gen_noise(osys, seed, cell, off + f)
            counts = plan.new_counts()
            dl = torch.from_numpy(labels).cuda()
            dn = torch.from_numpy(noise.view(np.float32).reshape(6, F, nl, 2)).cuda()
            plan.launch_injected(F, dl, dn, counts)
            torch.cuda.synchronize()
            plan.status()
            got = counts.cpu().numpy().view(np.uint64)
        else:
            got = plan.run(off, F)
    want = oracle_counts(c, h)
    d = np.abs(got[..., 0].astype(np.int64) - want[..., 0].astype(np.int64))
    print("row %s F %d noise_before_truncate %d: max |bit errors - oracle| %d, fewest expected errors %d"
          % (KC.row_id(row), F, c["matlab"], d.max(), want[..., 0].min()))
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])
    assert want[..., 0].min() > 2e2
    assert d.max() <= 12, (d, got[..., 0], want[..., 0])


# ------------------------------------------------------------------------------------------------------------------
# instrumented kernels: one frame stage by stage
def _test_windows(st, seed):
    """Flat level other than 1 and sorted random (not raised-cosine) tails, rounded to float32 on both sides
    (test_one_frame_stage_by_stage)."""
    rs = np.random.RandomState(seed)
    xt = np.concatenate(([1.03], np.sort(rs.uniform(.05, .95, st.tail_tx))[::-1])) if st.tail_tx else [1.0]
    xr = np.concatenate(([0.97], np.sort(rs.uniform(.05, .45, st.tail_rx // 2))[::-1])) if st.tail_rx else [1.0]
    w_tx = (W.expand_tx_window(st, xt) if st.tail_tx else np.ones(st.sym_len)).astype(np.float32)
    w_rx = (W.expand_rx_window(st, xr) if st.tail_rx else np.ones(st.rx_win_len)).astype(np.float32)
    return w_tx, w_rx


def _check_frame(tag, gc, gd, oc, od, lab, noise, st, k, S, matlab, inject, active, w_tx, masked):
    n_fft = st.n_fft
    act = np.ones(n_fft, bool) if active is None else active
    nact = int(act.sum())
    fig = {}
    # integer work: bit-exact
    assert np.array_equal(gd["labels_tx"], lab), tag
    assert int(gc[1]) == int(oc[1]) == (S - 1) * nact * k and int(gc[3]) == int(oc[3]) == (S - 1) * nact, tag
    # floating-point stages
    if not inject:
        fig["unit_noise"] = _rel(gd["unit_noise"], noise)
    fig["X"] = _rel(gd["X"], od["X"])
    nconv = od["conv"].size if matlab else S * st.stride
    fig["tx"] = _rel(gd["tx"], od["tx"])
    fig["conv"] = float(np.abs(gd["conv"][:nconv] - od["conv"][:nconv]).max() / np.abs(od["conv"]).max())
    fig["gain"] = abs(float(gd["gain"][0]) / float(od["gain"][0]) - 1)
    fig["rx"] = _rel(gd["rx"], od["rx"])
    fig["Y"] = _rel(gd["Y"], od["Y"])
    # the equalised symbols, where the channel is not in a null (there the division amplifies fp32 rounding)
    Hest = np.zeros(n_fft, complex)
    Hest[act] = od["Y"][0][act] / od["X"][0][act]
    ok = act & (np.abs(Hest) > 0.1 * np.abs(Hest).max())
    fig["Xhat"] = float(np.abs(gd["Xhat"][:, ok] - od["Xhat"][:, ok]).max() / np.abs(od["Xhat"][:, ok]).max())
    tx_np = None
    if masked:
        # independent restatement of the mask stage with numpy FFTs on the oracle's own symbols
        rows = (np.fft.ifft(od["X"], axis=1)[:, (np.arange(st.sym_len) - st.cp) % n_fft] * w_tx.astype(np.float64)[None, :])
        filt = CM.dft_rc_filt(rows)
        tx_np = np.zeros(st.frame_len(S), complex)
        for s in range(S):
            tx_np[s * st.stride:s * st.stride + st.sym_len] += filt[s]
        fig["tx_oracle_vs_numpy"] = _rel(od["tx"], tx_np)
        fig["tx_vs_numpy"] = _rel(gd["tx"], tx_np)
    mism = (gd["labels_rx"] != od["labels_rx"]) & act[None, :]
    print("%s: %s, decisions that differ %d" % (tag, ", ".join("%s %.3g" % kv for kv in fig.items()), int(mism.sum())))
    if active is not None:
        assert np.all(gd["X"][:, ~act] == 0), tag
    if not inject:
        assert fig["unit_noise"] < 1e-5, (tag, "unit_noise", fig)
    assert fig["X"] < 1e-6, (tag, "X", fig)
    for stage in ("tx", "conv", "rx", "Y"):
        assert fig[stage] < STAGE_RTOL, (tag, stage, fig)
    assert fig["gain"] < 1e-5, (tag, "gain", fig)                # (the noise gain from the measured powers: test_one_frame_stage_by_stage)
    if masked:
        assert fig["tx_oracle_vs_numpy"] < 1e-7, (tag, fig)      # the mask handed to both is float32-rounded
        assert fig["tx_vs_numpy"] < STAGE_RTOL, (tag, "tx", fig)
    # (enough bins left for the comparison to mean something; the Tx mask passes half of the band, so about half of the
    # loaded bins sit in ITS stop band and count as nulls here)
    assert ok.sum() > (nact // 4 if masked else nact // 2), tag
    assert fig["Xhat"] < 20 * STAGE_RTOL, (tag, "Xhat", fig)
    # decisions: identical except where the equalised point sits on a decision boundary of the slicer, loaded bins only
    _check_decisions(gd, od, gc, oc, k, act)


@pytest.mark.parametrize("row", DUMP, ids=KC.row_id)
def test_dump_kernel_stage_by_stage(channels, row):
    n_fft, k, layout, inject, var = row
    system, cp, S, options = KC.geometry_for(n_fft, layout, var)
    st = W.make_structure(system, n_fft, cp)
    seed, frame, cell = 11, 123456789012, 4                       # cell 4: snr index 1, channel 1
    matlab = KC.noise_before_truncate(row)
    w_tx, w_rx = _test_windows(st, n_fft + cp + k)
    active, mask = _allocation_and_mask(st, k, layout, var)
    h = channels[4:7].astype(np.complex64)
    snrs = np.array([8.0, 22.0], dtype=np.float32)
    cfg = W.make_cfg(st, k, S, 21, 3, 2, 1, noise_before_truncate=matlab, seed=seed)
    osys = _osys(st, k, S, matlab, active, mask)
    frames = (frame, frame + 1) if layout == 16 else (frame,)     # (layout 16: a second frame through the same rows)
    with W.Plan(cfg, w_tx, w_rx, h, snrs) as plan:
        _configure(plan, options, active, mask, layout, var)
        if layout == 16:
            spwr = KC.small_spwr(n_fft, S, st.stride)
            assert spwr > 0 and plan.info()["waves_per_workgroup"] == -(-S // spwr)
        else:
            assert plan.info()["waves_per_workgroup"] == -(-S // KC.layout_info(layout, n_fft)["spw"])
        got = []
        for fr in frames:
            lab, noise = O.gen_labels(osys, seed, cell, fr), O.gen_noise(osys, seed, cell, fr)
            got.append((fr, lab, noise) + plan.dump_frame(cell, fr, *((lab, noise.astype(np.complex64)) if inject else ())))
    for fr, lab, noise, gc, gd in got:
        oc, od = O.frame(osys, w_tx.astype(np.float64), w_rx.astype(np.float64), h[1].astype(np.complex128),
                         float(snrs[1]), lab, noise, dump=True)
        _check_frame("row %s frame %d" % (KC.row_id(row), fr - frame), gc, gd, oc, od, lab, noise, st, k, S, matlab, inject,
                     active, w_tx, var >= 2)


# ------------------------------------------------------------------------------------------------------------------
# the strides at which the choice changes
def _cp_structure(n_fft, stride, tail_tx=0):
    """No Rx window, a Tx tail of tail_tx samples (cyclic suffix: at most eight of them), the whole prefix removed: the
    geometry with a given stride and tail."""
    cs = min(tail_tx, 8)
    st = W.Structure("wtx" if tail_tx else "CP", n_fft, stride + tail_tx - n_fft - cs, tail_tx, 0, cs, stride - n_fft, 0)
    assert st.stride == stride == n_fft + st.tail_rx + st.prefix_rm
    return st


#: (n_fft, plan options, largest stride the layout takes, the layout, what the next stride gets: a layout, or None where
#: the plan -- or the option -- is refused, or LAST where there is no stride beyond).  Strides run from n_fft to n_fft + 64
#: (check_cfg: 64 * wofdm_rb(n_fft) FIR outputs per wave; at N = 64 a stride of 129 would need a prefix longer than the symbol,
#: which is an invalid geometry, not an unsupported one).
LAST = "last"
STRIDE_EDGES = [
    (64, {}, 80, 13, 14), (64, {}, 88, 14, 16), (64, {}, 128, 16, LAST),               # 16 symbols within 10 / 11 tiles
    (64, {"fir_valu": 1, "max_spw": 2}, 128, 2, LAST),
    (128, {}, 160, 13, 14), (128, {}, 176, 14, 16), (128, {}, 192, 16, None),          # 8 symbols within 10 / 11 tiles
    (256, {}, 288, 10, 11), (256, {}, 320, 11, None),                                  # 4 symbols within 9 / 10 tiles
    (256, {"dft_valu": 1}, 288, 6, 7), (256, {"dft_valu": 1}, 320, 7, None),
    (256, {"fir_valu": 1}, 288, 4, 5), (256, {"fir_valu": 1}, 320, 5, None),           # 18 / 20 FIR outputs per lane
    (128, {"fir_valu": 1, "max_spw": 2}, 192, 2, None), (256, {"fir_valu": 1, "max_spw": 2}, 320, 2, None),
    (512, {}, 576, 12, None), (512, {"dft_valu": 1}, 576, 8, None), (512, {"fir_valu": 1}, 576, 1, None),
    # N = 1024, S = 16: the LDS ends the range before the FIR tiling does (rows of (B + 3) & ~3 words: (B + 3 & ~3) + tail_tx
    # <= 1072 in layouts 8 / 12)
    (1024, {}, 1072, 12, None), (1024, {"dft_valu": 1}, 1072, 8, None),
    # ... and layout 1 keeps the frame as it is on air: 16 B + 17 tail_tx <= 17148 (wofdm_fbuf_len), B <= 1071 without a tail
    (1024, {"fir_valu": 1}, 1071, 1, None),
]


@pytest.mark.parametrize("var", [0, 1])
@pytest.mark.parametrize("n_fft,options,stride,layout,beyond", STRIDE_EDGES)
def test_layout_stride_edges(channels, n_fft, options, stride, layout, beyond, var):
    k, S, seed, off = 4, 16, 17, 2
    F = 200000 // ((S - 1) * n_fft * k)                              # 2e5 bits per cell
    h = channels[11:13].astype(np.complex64)
    snrs = np.array([8.0, 20.0], np.float32)
    rs = np.random.RandomState(n_fft + stride)
    active = None
    if var:
        active = rs.rand(n_fft) < 0.6
        active[0] = True

    def plan_for(B):
        st = _cp_structure(n_fft, B)
        cfg = W.make_cfg(st, k, S, 21, 2, 2, 1, seed=seed)
        return st, W.Plan(cfg, np.ones(st.sym_len, np.float32), np.ones(st.rx_win_len, np.float32), h, snrs)

    st, plan = plan_for(stride)
    with plan:
        _configure(plan, options, active, None, layout, var)
        assert KC.expected_kernel_id(st, S, options, var) == (layout, var)
        got = plan.run(off, F)
    want = O.run(_osys(st, k, S, True, active), np.ones(st.sym_len), np.ones(st.rx_win_len), h.astype(np.complex128),
                 snrs.astype(np.float64), seed, off, F)
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])
    assert want[..., 0].min() > 2e2
    d = np.abs(got[..., 0].astype(np.int64) - want[..., 0].astype(np.int64))
    assert d.max() <= 12, (d, got[..., 0], want[..., 0])            # (the bound of the production rows; far fewer bits here)
    if beyond is None:
        # one sample more: refused -- when the plan is made, or when the option asks for a layout the frame overflows (the
        # plan then stays as it was) -- and not run
        plan2 = None
        try:
            with pytest.raises(W._lib.WofdmError) as e:
                plan2 = plan_for(stride + 1)[1]
                before = plan2.kernel_id()
                _configure(plan2, options, active, None, layout, var)
            assert e.value.code == -2
            if plan2 is not None:
                assert plan2.kernel_id() == before and plan2.run(off, 2)[0, 0, 0, 1] == 2 * (S - 1) * n_fft * k
        finally:
            if plan2 is not None:
                plan2.close()
    elif beyond != LAST:
        st2, plan2 = plan_for(stride + 1)
        with plan2:
            _configure(plan2, options, active, None, beyond, var)
            assert KC.expected_kernel_id(st2, S, options, var) == (beyond, var)


def test_lds_boundary_at_n1024(channels):
    """N = 1024, S = 16: layouts 8 / 12 pitch their LDS rows by BR = (B + 3) & ~3 words, so the frame fits while
    BR + tail_tx <= 1072 -- with a stride that is no multiple of four less than the B + tail_tx <= 1072 of a pitch of B.
    Where the padded rows do not fit, the plan falls back to the one-symbol-per-wave VALU kernel (layout 1) if that fits
    (16 B + 17 tail_tx <= 17148); else the geometry is refused.  B = 1062, tail_tx = 10 (cp 40, cs 8: P = 1072) is such a
    refusal: it would fit layout 12 at pitch B, which the kernels do not have -- recorded here as the library's behaviour, an
    open regression against round 3."""
    k, S, seed, off, F = 4, 16, 19, 1, 6                           # 3.7e5 bits per cell
    h = channels[11:13].astype(np.complex64)
    snrs = np.array([8.0, 20.0], np.float32)

    def make(B, tail_tx):
        st = _cp_structure(1024, B, tail_tx)
        return st, W.make_cfg(st, k, S, 21, 2, 2, 1, seed=seed)

    def lds12(B, beta, pitch):          # wofdm_lds_bytes(1024, T, 12, 16, B) with rows of `pitch` words
        return 26112 + 8 * ((8 + 2 * S * pitch + 2 * 48) // 2) + 8 * S * beta

    # the last geometry layout 12 takes, and with option fir_valu refused (layout 1 needs more LDS): the plan stays as it was
    st, cfg = make(1072, 0)
    assert lds12(1072, 0, 1072) <= 160 * 1024 < lds12(1073, 0, 1076)
    with W.Plan(cfg, np.ones(st.sym_len, np.float32), np.ones(st.rx_win_len, np.float32), h, snrs) as plan:
        assert plan.kernel_id() == (12, 0) and plan.info()["lds_bytes"] == lds12(1072, 0, 1072)
        first = plan.run(off, F)
        with pytest.raises(W._lib.WofdmError) as e:
            plan.set_option("fir_valu", 1)
        assert e.value.code == -2 and plan.kernel_id() == (12, 0)
        assert np.array_equal(plan.run(off, F), first)
    # an odd stride whose padded rows do not fit, while layout 1 does: B = 1069, tail_tx = 1
    st, cfg = make(1069, 1)
    assert lds12(1069, 1, 1072) > 160 * 1024 and 16 * 1069 + 17 * 1 <= 17148
    w_tx = W.tx_rc_window(st).astype(np.float32)
    with W.Plan(cfg, w_tx, np.ones(st.rx_win_len, np.float32), h, snrs) as plan:
        assert plan.kernel_id() == (1, 0)
        got = plan.run(off, F)
    want = O.run(_osys(st, k, S, True), w_tx.astype(np.float64), np.ones(st.rx_win_len), h.astype(np.complex128),
                 snrs.astype(np.float64), seed, off, F)
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])
    assert want[..., 0].min() > 2e2
    assert np.abs(got[..., 0].astype(np.int64) - want[..., 0].astype(np.int64)).max() <= 12
    # ADVICE.md's geometry: fits at pitch B, not at pitch BR, and layout 1 does not fit either.  KNOWN REGRESSION: the change that
    # gives layouts 8 / 12 rows of pitch B turns this refusal into a plan with kernel_id (12, 0) and a parity check like the one above
    st, cfg = make(1062, 10)
    assert st.sym_len == 1072 and lds12(1062, 10, 1062) <= 160 * 1024 < lds12(1062, 10, 1064) and 16 * 1062 + 17 * 10 > 17148
    with pytest.raises(W._lib.WofdmError) as e:
        W.Plan(cfg, W.tx_rc_window(st).astype(np.float32), np.ones(st.rx_win_len, np.float32), h, snrs).close()
    assert e.value.code == -2
