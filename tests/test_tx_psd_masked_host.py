"""wofdm_tx_psd_batch_masked (Tx-PSD of the spectrally masked waveform) without a GPU: its argument checks, its
place in the public header and the binding; the fp64 host mirror ``timefreq.tx_waveform`` / ``mask_rows`` tied to
the untouched ``channel_mask.dft_rc_filt`` and to the CPU oracle's ``tx`` stage with ``tx_mask`` set; and the host
route of ``channel_mask.spectrum_for_window_file``."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"]


def _call(n_fft=512, device=99, jobs=None, masks=None, job_mask="default", n_masks=None, mask_len=None, null=()):
    """jobs: (block, cp, cs, overlap); masks: list of gain vectors; default: job 0 masked with an all-ones mask"""
    lib = _lib.load()
    jobs = [(0, 12, 8, 8), (1, 0, 0, 0)] if jobs is None else jobs
    cj = (_lib.PsdJob * len(jobs))()
    for i, (b, cp, cs, ov) in enumerate(jobs):
        cj[i].block, cj[i].cp, cj[i].cs, cj[i].overlap = b, cp, cs, ov
    P0 = n_fft + jobs[0][1] + jobs[0][2]
    masks = [np.ones(2 * P0 - 1, np.float32)] if masks is None else masks
    job_mask = [0] + [-1] * (len(jobs) - 1) if isinstance(job_mask, str) else job_mask
    jm = None if job_mask is None else np.asarray(job_mask, np.int32)
    ml = np.asarray([len(m) for m in masks] if mask_len is None else mask_len, np.int32)
    mg = np.concatenate([np.asarray(m, np.float32) for m in masks] + [np.zeros(1, np.float32)])
    w = np.ones(sum(n_fft + cp + cs for _, cp, cs, _ in jobs) + 1, np.float32)
    X = np.zeros((2, 3, n_fft, 2), np.float32)
    psd = np.zeros((len(jobs), 8 * n_fft), np.float32)
    ptr = {"jobs": C.addressof(cj), "w": w.ctypes.data, "X": X.ctypes.data, "psd": psd.ctypes.data,
           "mask_len": ml.ctypes.data, "mask_gain": mg.ctypes.data, "job_mask": None if jm is None else jm.ctypes.data}
    for k in null:
        ptr[k] = None
    return lib.wofdm_tx_psd_batch_masked(n_fft, device, len(jobs), ptr["jobs"], ptr["w"],
                                         len(masks) if n_masks is None else n_masks, ptr["mask_len"], ptr["mask_gain"],
                                         ptr["job_mask"], 2, 3, ptr["X"], ptr["psd"])


def test_masked_batch_refuses_bad_arguments_before_any_device_call():
    err = lambda: _lib.load().wofdm_last_error().decode()
    for n_fft in (64, 128, 256, 512, 1024):
        assert _call(n_fft=n_fft) == -3 and "device" in err(), n_fft      # valid arguments reach the device check
    assert _call(job_mask=None) == -3                                     # NULL job_mask: all unmasked
    assert _call(n_masks=0, job_mask=[-1, -1], null=("mask_len", "mask_gain")) == -3
    for k in ("jobs", "w", "X", "psd", "mask_len", "mask_gain"):
        assert _call(null=(k,)) == -1, k
    assert _call(n_masks=-1) == -1
    for n in (32, 192, 2048):
        assert _call(n_fft=n) == -2, n
    for jm in ([1, -1], [-2, -1], [0, 1]):
        assert _call(job_mask=jm) == -1, jm
    assert "mask index" in err()
    P = 512 + 20
    for bad_len in (2 * P, 2 * P - 2, P, 0):
        assert _call(masks=[np.ones(max(bad_len, 1), np.float32)], mask_len=[bad_len]) == -1, bad_len
    assert _call(job_mask=[0, 0]) == -1                                   # job 1 has another P than the mask
    for bad in (np.inf, -np.inf, np.nan):
        m = np.ones(2 * P - 1, np.float32)
        m[7] = bad
        assert _call(masks=[m]) == -1 and "finite" in err(), bad
    # the existing job checks
    for job in [(2, 12, 8, 8), (0, 513, 0, 0), (0, 0, -1, 0), (0, 12, 8, -1), (0, 12, 8, P // 2 + 1)]:
        assert _call(jobs=[(0, 12, 8, 8), job]) == -1, job


@pytest.mark.parametrize("n_fft", [64, 128, 256, 512, 1024])
def test_masked_batch_names_its_geometry_limit(n_fft):
    """3 P - 2 <= 8 n_fft: every cp + cs <= n_fft / 2 is taken, the first P beyond (8 n_fft + 2) / 3 is refused as
    unsupported with the limit in the message -- for a masked job only."""
    pmax = (8 * n_fft + 2) // 3
    assert 3 * pmax - 2 <= 8 * n_fft < 3 * (pmax + 1) - 2 and pmax >= n_fft + n_fft // 2
    for cp, cs in ((n_fft // 2, 0), (n_fft // 4, n_fft // 4), (0, n_fft // 2),
                   ((pmax - n_fft) // 2, pmax - n_fft - (pmax - n_fft) // 2)):      # (cp, cs <= n_fft each)
        assert _call(n_fft=n_fft, jobs=[(0, cp, cs, 0)]) == -3, (cp, cs)
    over = ((pmax + 1 - n_fft) // 2, pmax + 1 - n_fft - (pmax + 1 - n_fft) // 2)
    assert _call(n_fft=n_fft, jobs=[(0,) + over + (0,)]) == -2
    msg = _lib.load().wofdm_last_error().decode()
    assert "3 P - 2 <= 8 n_fft" in msg and str(pmax) in msg, msg
    assert _call(n_fft=n_fft, jobs=[(0,) + over + (0,)], job_mask=[-1]) == -3       # unmasked: no such limit


def test_masked_batch_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int wofdm_tx_psd_batch_masked(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs, "
            "const float *w_tx, int32_t n_masks, const int32_t *mask_len, const float *mask_gain, "
            "const int32_t *job_mask, int32_t n_blocks, int32_t no_symbols, const float *X, float *psd);") in flat
    comment = flat[flat.index("/* wofdm_tx_psd_batch with an optional spectral Tx mask"):flat.index("int wofdm_tx_psd_batch_masked(")]
    assert "holds the same gate" in comment and "WOFDM_E_UNSUPPORTED" in comment and "3 P - 2 <= 8 n_fft" in comment
    assert "wofdm_tx_psd_batch_masked" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "wofdm_tx_psd_batch_masked") and len(lib.wofdm_tx_psd_batch_masked.argtypes) == 13
    assert lib.wofdm_version() == 1
    for name in ("tx_waveform", "tx_psd_batch_gpu", "spectrum_for_window_file"):
        assert hasattr(W, name), name


def _case(system, n_fft, cp, S, seed):
    st = V.make_structure(system, n_fft, cp)
    rs = np.random.RandomState(seed)
    X = T.draw_symbols(n_fft, rs, S, guard_band=n_fft // 8)
    tail = np.concatenate(([1.0], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1]))
    w_tx = V.expand_tx_window(st, tail) if st.tail_tx else np.ones(st.sym_len)
    return st, X, w_tx


@pytest.mark.parametrize("system,n_fft,cp", [("wtx", 64, 16), ("CPW", 256, 32), ("wrx", 128, 20)])
def test_all_ones_mask_is_the_unmasked_waveform(system, n_fft, cp):
    st, X, w = _case(system, n_fft, cp, 9, 1)
    for ov in (st.tail_tx, 0):
        plain = T.overlap_and_add(T.tx_symbols(st, X, w, n_fft // 8), ov)
        assert np.array_equal(T.tx_waveform(st, X, w, ov, guard_band=n_fft // 8), plain)
        got = T.tx_waveform(st, X, w, ov, mask=np.ones(2 * st.sym_len - 1), guard_band=n_fft // 8)
        assert got.shape == plain.shape and np.abs(got - plain).max() < 1e-12 * np.abs(plain).max()


@pytest.mark.parametrize("system,n_fft,cp", [("wtx", 64, 16), ("CPW", 256, 32), ("wrx", 128, 20)])
def test_mirror_rows_are_dft_rc_filt(system, n_fft, cp):
    """overlap 0: the waveform is the filtered rows side by side -- against the untouched dft_rc_filt"""
    st, X, w = _case(system, n_fft, cp, 7, 2)
    rows = T.tx_symbols(st, X, w, n_fft // 8)
    want = CM.dft_rc_filt(rows)
    got = T.tx_waveform(st, X, w, 0, mask=CM.tx_mask(st.sym_len), guard_band=n_fft // 8).reshape(7, st.sym_len)
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()
    assert np.abs(T.mask_rows(rows, CM.tx_mask(st.sym_len, 6)) - CM.dft_rc_filt(rows, 6)).max() < 1e-12 * np.abs(want).max()
    with pytest.raises(ValueError):
        T.mask_rows(rows, np.ones(2 * st.sym_len))


@pytest.mark.parametrize("system,n_fft,cp", [("wtx", 64, 16), ("CPW", 256, 32)])
def test_mirror_is_the_oracles_masked_tx_stage(system, n_fft, cp):
    """The CPU oracle's ``tx`` dump of one masked frame (S = 16) = the mirror's waveform for the same symbols and
    window.  The oracle's IDFT carries the same 1 / N as numpy's, its dump X holds every bin."""
    S, k = 16, 4
    st = W.make_structure(system, n_fft, cp)
    mask = CM.tx_mask(st.sym_len)
    osys = O.make_sys(n_fft, k, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, 21, 1,
                      active=CM.half_band_allocation(n_fft), tx_mask=mask)
    lab, noise = O.gen_labels(osys, 4, 0, 2), O.gen_noise(osys, 4, 0, 2)
    w_tx, w_rx = W.tx_rc_window(st), W.rx_rc_window(st)
    _, d = O.frame(osys, w_tx, w_rx, CH[0], 200.0, lab, noise, dump=True)
    got = T.tx_waveform(st, d["X"].T, w_tx, st.tail_tx, mask=mask, guard_band=None)
    assert got.shape == d["tx"].shape
    assert np.abs(got - d["tx"]).max() < 1e-12 * np.abs(d["tx"]).max()
    plain = T.tx_waveform(st, d["X"].T, w_tx, st.tail_tx, guard_band=None)
    assert np.abs(plain - d["tx"]).max() > 1e-3 * np.abs(d["tx"]).max()


def test_spill_lands_in_the_next_symbol_only():
    """One non-zero symbol s0 among zeros: the masked waveform lives in rows s0 and s0 + 1 only, and a non-zero
    LAST symbol leaves nothing behind the waveform (its spill is dropped)."""
    n, cp, S = 64, 16, 6
    st = V.make_structure("wrx", n, cp)                      # no Tx tail: overlap 0, rows side by side
    P = st.sym_len
    mask = np.random.RandomState(3).uniform(0.2, 1.2, 2 * P - 1)
    for s0 in (0, 2, S - 1):
        X = np.zeros((n, S), complex)
        X[5, s0] = 1 + 2j
        rows = T.tx_waveform(st, X, np.ones(P), 0, mask=mask, guard_band=None).reshape(S, P)
        y = np.fft.ifft(np.fft.fft(T.tx_waveform(st, X, np.ones(P), 0, guard_band=None).reshape(S, P)[s0], 2 * P - 1) * mask)
        assert np.abs(rows[s0] - y[:P]).max() < 1e-14
        live = [s0] + ([s0 + 1] if s0 + 1 < S else [])
        for s in range(S):
            if s not in live:
                assert np.abs(rows[s]).max() == 0, (s0, s)
        if s0 + 1 < S:
            assert np.abs(rows[s0 + 1][:P - 1] - y[P:]).max() < 1e-14 and rows[s0 + 1][P - 1] == 0
            assert np.abs(y[P:]).max() > 1e-4                  # there is a spill to speak of


def _windows(st, seed=5):
    rs = np.random.RandomState(seed)

    def tx():
        return V.expand_tx_window(st, np.concatenate(([1.0], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1])))
    keys = ("optimizedWindow", "optimizedWindowCaseAStep1", "optimizedWindowCaseAStep3", "optimizedWindowCaseBStep1",
            "optimizedWindowCaseBStep2", "optimizedWindowCaseBStep3")
    return {k: tx() for k in keys}


@pytest.mark.parametrize("system", ["wtx", "CPW"])
def test_spectrum_for_window_file_host_route(system):
    n, cp = 256, 32
    st = V.make_structure(system, n, cp, 8, 10 if system in V.RX_WINDOWED else 0)
    res = CM.spectrum_for_window_file(system, cp, _windows(st), num_subcar=n, rng=np.random.RandomState(11), gpu=False)
    assert list(res) == [name for name, _ in V.matlab_pair_plan(system)] and "rc" in res
    for name, d in res.items():
        assert set(d) == {"psd", "psd_masked", "obr", "obr_masked", "f_axis"}
        assert d["psd"].shape == d["psd_masked"].shape == d["f_axis"].shape == (8 * n,)
        assert np.abs(d["psd"] - d["psd_masked"]).max() > 1e-4 * d["psd"].max(), name
        assert 0 < d["obr_masked"] and 0 < d["obr"]
    rc = res["rc"]
    assert rc["obr_masked"] < rc["obr"]
    # half-band loading: the loaded half carries the power, the OBR bins are the other half of the grid
    loaded = np.fft.fftshift(np.repeat(CM.half_band_allocation(n), 8))
    assert rc["psd"][loaded].mean() > 50 * rc["obr"] and abs(rc["psd"][~loaded].mean() - rc["obr"]) < 1e-12 * rc["obr"]
    # given symbols: deterministic, and the same as the draw
    sym = np.random.RandomState(11).choice(T.SYMBOLS_16QAM, size=(n // 2, 256), replace=True)
    again = CM.spectrum_for_window_file(system, cp, _windows(st), num_subcar=n, symbols=sym, gpu=False)
    assert np.array_equal(again["rc"]["psd_masked"], rc["psd_masked"])
