"""wofdm_tx_psd_batch (the Tx-PSD entry point for a batch of jobs at every N) without a GPU: its argument
checks, its place in the public header and the binding, and the host route of run_timefreq (the
``-m run_timefreq`` sweep) against successive timefreq_fun calls."""
import ctypes as C
import os
import re

import numpy as np

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(n_fft=512, device=0, jobs=None, n_jobs=None, w=None, n_blocks=2, no_symbols=3, X=None, psd=None,
          null=()):
    lib = _lib.load()
    jobs = [(0, 12, 8, 8), (1, 0, 0, 0)] if jobs is None else jobs
    cj = (_lib.PsdJob * max(1, len(jobs)))()
    for i, (b, cp, cs, ov) in enumerate(jobs):
        cj[i].block, cj[i].cp, cj[i].cs, cj[i].overlap = b, cp, cs, ov
    w = np.ones(sum(n_fft + cp + cs for _, cp, cs, _ in jobs) + 1, np.float32) if w is None else w
    X = np.zeros((max(n_blocks, 1), max(no_symbols, 1), max(n_fft, 1), 2), np.float32) if X is None else X
    psd = np.zeros((max(1, len(jobs)), 8 * max(n_fft, 1)), np.float32) if psd is None else psd
    ptr = {"jobs": C.addressof(cj), "w": w.ctypes.data, "X": X.ctypes.data, "psd": psd.ctypes.data}
    for k in null:
        ptr[k] = None
    return lib.wofdm_tx_psd_batch(n_fft, device, len(jobs) if n_jobs is None else n_jobs, ptr["jobs"], ptr["w"],
                                  n_blocks, no_symbols, ptr["X"], ptr["psd"])


def test_tx_psd_batch_refuses_bad_arguments():
    for k in ("jobs", "w", "X", "psd"):
        assert _call(null=(k,)) == -1, k
    for n in (32, 128 + 64, 2048, 0):
        assert _call(n_fft=n) == -2, n
    assert _call(n_jobs=0) == -1
    assert _call(n_blocks=0) == -1 and _call(no_symbols=0) == -1
    bad_jobs = [(2, 12, 8, 8), (-1, 12, 8, 8), (0, 513, 0, 0), (0, -1, 0, 0), (0, 0, 513, 0), (0, 0, -1, 0),
                (0, 12, 8, -1), (0, 12, 8, (512 + 20) // 2 + 1)]
    for job in bad_jobs:
        assert _call(jobs=[(0, 0, 0, 0), job]) == -1, job
    assert _call(jobs=[(0, 12, 8, (512 + 20) // 2)], device=99) == -3          # a legal overlap: P / 2
    assert _call(device=99) == -3 and _call(device=-1) == -3
    assert _call(n_fft=1024, device=99) == -3 and _call(n_fft=64, device=99) == -3
    assert "device" in _lib.load().wofdm_last_error().decode()


def test_tx_psd_batch_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    assert re.search(r"^int wofdm_tx_psd_batch\(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job \*jobs,",
                     hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct wofdm_psd_job {"):hdr.index("} wofdm_psd_job;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for grp in re.findall(r"\bint32_t\s+([^;]+);", body) for n in grp.split(",")]
    assert fields == [f for f, _ in _lib.PsdJob._fields_] and C.sizeof(_lib.PsdJob) == 16
    assert "wofdm_tx_psd_batch" in _lib.EXPORTS
    assert hasattr(_lib.load(), "wofdm_tx_psd_batch")
    # the exclusive-use paragraph names it among the entry points that hold the device gate
    assert "wofdm_tx_psd, wofdm_tx_psd_batch) hold the same gate" in re.sub(r"\s*\n \* ", " ", hdr)


def write_windows(folder, systems, cps, seed=5):
    """reference-format window files (``<system>_<cp>.npy``) for the Tx-windowed systems"""
    rs = np.random.RandomState(seed)
    for system in systems:
        for cp in cps:
            if system not in V.TX_WINDOWED:
                continue
            xt = np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(0.02, 0.98, 8))[::-1]))
            xr = np.concatenate(([1.0], np.sort(rs.uniform(0.02, 0.48, 5))[::-1]))
            vec = np.concatenate((xt, xr)) if system in ("WOLA", "CPW") else xt
            np.save(os.path.join(folder, "%s_%d.npy" % (system, cp)), vec)


def test_run_timefreq_host_matches_successive_timefreq_fun_calls(tmp_path):
    systems, cps = ("CPW", "wrx"), (12, 20)
    write_windows(str(tmp_path), systems, cps)
    got = W.run_timefreq(cps, systems, str(tmp_path), str(tmp_path / "a"), n_fft=128,
                         rng=np.random.RandomState(3))
    rng = np.random.RandomState(3)
    for system in systems:
        for cp in cps:
            data = (system, 128, cp, 8 if system in V.TX_WINDOWED else 0, 10 if system in V.RX_WINDOWED else 0,
                    str(tmp_path), str(tmp_path / "b"))
            want = T.timefreq_fun(data, rng)
            for dg, dw in zip(got[(system, cp)], want):
                assert set(dg) == set(dw)
                for k in dw:
                    assert np.array_equal(dg[k], dw[k]), (system, cp, k)
    names = sorted(os.listdir(tmp_path / "a" / "timefreq"))
    assert names == sorted(os.listdir(tmp_path / "b" / "timefreq")) == sorted(
        ["opt_%s_%d.npz" % (s, c) for s in systems for c in cps] + ["rc_%s_%d.npz" % (s, c) for s in systems
                                                                     for c in cps] + ["CP_12.npz", "CP_20.npz"])
    for name in names:
        a, b = np.load(tmp_path / "a" / "timefreq" / name), np.load(tmp_path / "b" / "timefreq" / name)
        assert set(a.files) == set(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files), name
