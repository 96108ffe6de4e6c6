"""wofdm_tx_papr without a GPU: its place in the public header and the binding, its argument checks (every refusal comes
before the device is touched and leaves the outputs alone), and the fp64 host mirror -- ``timefreq.frame_papr`` on grids
mapped from ``oracle.gen_labels`` against the {peak, energy} of the oracle's own ``tx`` dump, ``papr_hist``,
``papr_ccdf`` -- together with the seeds the GPU tests rely on (tests/papr_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

import papr_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_H, SENT_F = 0xA5A5A5A5A5A5A5A5, -7.5


def _call(n_fft=256, k=4, S=4, cp=32, cs=8, beta=8, pairs=2, frames=3, device=99, active="none", mask="none", lo=0.0,
          step=0.25, n_bins=16, periods=True, null=(), cfg_edit=None):
    """-> (rc, outputs untouched); valid arguments end at the device check (-3: no device 99)"""
    lib = _lib.load()
    cfg = _lib.Cfg(n_fft, k, S, cp, cs, beta, 0, 0, 0, 1, 1, 1, pairs, 1, frames, 0, 1)
    if cfg_edit:
        cfg_edit(cfg)
    P = n_fft + max(cp, 0) + max(cs, 0)
    w = np.ones((max(pairs, 1), P), np.float32)
    act = None if isinstance(active, str) else np.ascontiguousarray(active, np.uint8)
    m = None if isinstance(mask, str) else np.ascontiguousarray(mask, np.float32)
    hist = np.full((max(pairs, 1), max(n_bins, 1)), SENT_H, np.uint64)
    mx = np.full(max(pairs, 1), SENT_F, np.float32)
    per = np.full((max(pairs, 1), min(frames, 64), max(S, 1), 2), SENT_F, np.float32)
    ptr = {"cfg": C.byref(cfg), "w": w.ctypes.data, "hist": hist.ctypes.data, "max": mx.ctypes.data,
           "periods": per.ctypes.data if periods else None}
    for name in null:
        ptr[name] = None
    rc = lib.wofdm_tx_papr(ptr["cfg"], device, ptr["w"], None if act is None else act.ctypes.data,
                           None if m is None else m.ctypes.data, lo, step, n_bins, ptr["hist"], ptr["max"], ptr["periods"])
    untouched = bool((hist == SENT_H).all() and (mx == SENT_F).all() and (per == SENT_F).all())
    return rc, untouched


def test_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int wofdm_tx_papr(const wofdm_cfg *cfg, int device, const float *w_tx, const uint8_t *active, "
            "const float *tx_mask, float lo_db, float step_db, int32_t n_bins, uint64_t *hist, float *max_papr, "
            "float *periods);") in flat
    whole = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", hdr))
    comment = whole[whole.index("/* Peak-to-average power ratio"):whole.index("#define WOFDM_TX_PAPR_CHUNK_BYTES")]
    for words in ("The reference has no PAPR", "ACCUMULATED", "holds the same gate", "WOFDM_TX_PAPR_CHUNK_BYTES",
                  "3 P - 2 <= 8 n_fft", "checked before the device is touched", "repeated calls give identical"):
        assert words in comment, words
    assert not re.search(r"\.(m|py):\d", comment)                       # no reference line: there is none to cite
    assert "#define WOFDM_ABI_VERSION 1" in hdr
    assert int(re.search(r"#define WOFDM_TX_PAPR_CHUNK_BYTES \((\d+)u << 20\)", hdr).group(1)) << 20 == _lib.TX_PAPR_CHUNK_BYTES
    assert 1 << int(re.search(r"#define WOFDM_TX_PAPR_MAX_PERIODS \(1 << (\d+)\)", hdr).group(1)) == _lib.TX_PAPR_MAX_PERIODS
    assert "wofdm_tx_papr" in _lib.EXPORTS and "wofdm_tx_papr_kernel_ms" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "wofdm_tx_papr") and len(lib.wofdm_tx_papr.argtypes) == 11
    assert lib.wofdm_tx_papr.argtypes[5] is C.c_float and lib.wofdm_tx_papr.argtypes[7] is C.c_int32
    assert lib.wofdm_version() == 1
    ms = C.c_float(-1.0)
    assert lib.wofdm_tx_papr_kernel_ms(C.byref(ms)) == 0 and ms.value == 0.0 and lib.wofdm_tx_papr_kernel_ms(None) == -1
    for name in ("frame_papr", "papr_hist", "papr_ccdf", "tx_papr_gpu", "papr_for_window_file"):
        assert hasattr(W, name), name


def test_refusals_come_before_the_device_and_leave_the_outputs_alone():
    err = lambda: _lib.load().wofdm_last_error().decode()
    for n_fft in PC.NS:
        for k in (2, 4, 6):
            assert _call(n_fft=n_fft, k=k, S=2 + k) == (-3, True) and "device" in err(), (n_fft, k)
    ok_mask = np.ones(2 * (256 + 40) - 1, np.float32)
    assert _call(mask=ok_mask, active=CM.half_band_allocation(256)) == (-3, True)
    assert _call(periods=False) == (-3, True) and _call(null=("max",)) == (-3, True)
    # WOFDM_E_INVALID
    for name in ("cfg", "w", "hist"):
        assert _call(null=(name,)) == (-1, True), name
    for n_bins in (0, -1):
        assert _call(n_bins=n_bins) == (-1, True), n_bins
    for step in (0.0, -0.25, np.inf, np.nan):
        assert _call(step=step) == (-1, True), step
    assert _call(lo=np.nan) == (-1, True)
    for bad in (np.inf, -np.inf, np.nan):
        m = ok_mask.copy()
        m[11] = bad
        assert _call(mask=m) == (-1, True) and "finite" in err(), bad
    assert _call(active=np.zeros(256, np.uint8)) == (-1, True) and "allocation" in err()
    for kw in (dict(cp=-1), dict(cs=-1), dict(beta=-1), dict(cp=257), dict(cs=257), dict(beta=149), dict(pairs=0)):
        assert _call(**kw) == (-1, True), kw
    # WOFDM_E_UNSUPPORTED
    for n_fft in (32, 192, 2048):
        assert _call(n_fft=n_fft) == (-2, True), n_fft
    for k in (1, 3, 8):
        assert _call(k=k) == (-2, True), k
    for S in (1, 17):
        assert _call(S=S) == (-2, True), S
    assert _call(n_bins=8193) == (-2, True) and _call(n_bins=8192) == (-3, True)
    # the mask's transform length: 3 P - 2 <= 8 n_fft, for a masked call only
    for n_fft in PC.NS:
        pmax = (8 * n_fft + 2) // 3
        cp = min(n_fft, pmax - n_fft)
        geo = dict(n_fft=n_fft, cp=cp, cs=pmax - n_fft - cp, beta=0)
        assert _call(mask=np.ones(2 * pmax - 1, np.float32), **geo) == (-3, True), n_fft
        geo["cs"] += 1
        assert _call(mask=np.ones(2 * pmax + 1, np.float32), **geo) == (-2, True) and "3 P - 2 <= 8 n_fft" in err(), n_fft
        assert _call(**geo) == (-3, True), n_fft
    # periods is a diagnostic output: at most 2^20 periods in total
    assert _call(S=16, pairs=2, frames=(1 << 15) + 1) == (-2, True) and "periods" in err()
    assert _call(S=16, pairs=2, frames=1 << 15) == (-3, True)
    assert _call(S=16, pairs=2, frames=10 ** 9, periods=False) == (-3, True)
    assert _call(frames=1 << 62, periods=False) == (-2, True)


def test_chunk_rule_of_the_binding_is_the_headers():
    st = V.make_structure("wtx", 1024, 128)
    T_len = st.tail_tx + 16 * (st.sym_len - st.tail_tx)
    assert T.tx_papr_chunk_frames(st, 16, False) == (256 << 20) // (8 * (16 * 1024 + T_len))
    assert T.tx_papr_chunk_frames(st, 16, True) == (256 << 20) // (8 * (16 * 1024 + T_len + 16 * (2 * st.sym_len - 1)))
    assert T.tx_papr_chunk_frames(V.make_structure("wrx", 64, 8), 2, False) == 65535


def test_qam_table_is_the_oracles():
    for k in (2, 4, 6):
        assert np.abs(T.qam_table(k) - O.qam_table(k)).max() < 1e-15
        assert abs((np.abs(T.qam_table(k)) ** 2).mean() - 1) < 1e-12


@pytest.mark.parametrize("variant", ["plain", "half", "masked"])
@pytest.mark.parametrize("system", PC.SYSTEMS)
@pytest.mark.parametrize("n_fft", [64, 256])
def test_frame_papr_is_the_oracles_tx_stage(n_fft, system, variant):
    """grids mapped from oracle.gen_labels -> frame_papr = {peak, energy} of the oracle's dump.tx, 1e-12 relative"""
    cp, S, k = PC.shape_of(n_fft, system, variant)
    st = PC.structure(n_fft, system)
    B = st.sym_len - st.tail_tx
    w = PC.random_windows(st, 1, n_fft + 3)[0]
    active, mask = PC.allocation(n_fft, variant), PC.mask_of(st, variant)
    tab = T.qam_table(k)
    grids, want = [], []
    for frame in (0, 2 ** 33 + 1):
        lab, tx = PC.oracle_frame_tx(st, k, S, w, active, mask, 12, 0, frame)
        assert tx.shape == (st.tail_tx + S * B,)
        grids.append(tab[lab] * (1.0 if active is None else active[None, :]))
        want.append(PC.periods_of(tx, S, B))
    got = T.frame_papr(st, np.stack(grids), w, mask)
    want = np.stack(want)
    assert got.shape == want.shape == (2, S, 2)
    assert (np.abs(got - want) / want).max() < 1e-12
    if st.tail_tx:                     # the trailing ramp-down belongs to no period
        assert np.abs(tx[S * B:]).max() > 0


def test_papr_hist_clamps_at_both_ends():
    B = 10
    db = np.array([-3.0, 3.99, 4.0, 4.24, 4.25, 6.1, 13.99, 14.0, 40.0])
    per = np.stack([10.0 ** (db / 10.0) / B * 2.0, np.full(db.size, 2.0)], axis=1)
    per = np.concatenate([per, [[0.0, 0.0]]])                            # no energy: bin 0
    h = T.papr_hist(per, B, 4.0, 0.25, 40)
    assert h.dtype == np.uint64 and h.shape == (40,) and h.sum() == 10
    assert h[0] == 5 and h[1] == 1 and h[8] == 1 and h[39] == 3          # 4.0, 4.24 sit in bin 0 with the three below
    assert T.papr_hist(per, B, 4.0, 0.25, 1)[0] == 10
    assert T.papr_hist(per[:, None, :].reshape(2, 5, 2), B, 4.0, 0.25, 40).sum() == 10


def test_papr_ccdf_of_a_hand_made_histogram():
    h = np.array([0, 6, 3, 0, 1], np.uint64)
    assert np.allclose(T.papr_ccdf(h), [1.0, 1.0, 0.4, 0.1, 0.1])
    two = T.papr_ccdf(np.stack([h, np.zeros(5, np.uint64)]))
    assert two.shape == (2, 5) and np.allclose(two[0], [1.0, 1.0, 0.4, 0.1, 0.1]) and (two[1] == 0).all()


def test_the_gpu_cases_seeds_keep_clear_of_the_bin_edges():
    """the condition of the GPU histogram check, near <= 1 % of the periods, is a property of the oracle alone (the
    cheap cases here; every case asserts it through pick_seed when its reference is built)"""
    for n_fft, system, variant in [(64, "wtx", "plain"), (128, "CPW", "half"), (256, "wrx", "masked"), (256, "CPW", "plain")]:
        r = PC.reference(n_fft, system, variant)
        B = r["st"].sym_len - r["st"].tail_tx
        assert r["near"] == PC.near_edges(r["periods"], B) <= 0.01 * PC.PAIRS * PC.FRAMES * r["S"]
        assert r["periods"].shape == (PC.PAIRS, PC.FRAMES, r["S"], 2)


def test_papr_for_window_file_host_route():
    n, cp = 64, 16
    st = V.make_structure("wtx", n, cp, 8, 0)
    rs = np.random.RandomState(5)
    keys = ("optimizedWindow", "optimizedWindowCaseAStep1", "optimizedWindowCaseAStep3", "optimizedWindowCaseBStep1",
            "optimizedWindowCaseBStep2", "optimizedWindowCaseBStep3")
    wins = {kk: V.expand_tx_window(st, np.concatenate(([1.0], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1]))) for kk in keys}
    res = CM.papr_for_window_file("wtx", cp, wins, num_subcar=n, symbols_per_tx=4, ensemble=6, gpu=False)
    assert list(res) == [name for name, _ in V.matlab_pair_plan("wtx")]
    for d in res.values():
        assert set(d) == {"hist", "hist_masked", "ccdf", "ccdf_masked", "max_db", "max_db_masked", "edges_db"}
        assert d["hist"].sum() == d["hist_masked"].sum() == 24 and d["ccdf"][0] == 1.0 and d["edges_db"].shape == (64,)
        assert 3.0 < d["max_db"] < 15.0 and 3.0 < d["max_db_masked"] < 15.0
