#!/usr/bin/env python3
"""Generate tests/golden/psd_large.npz from the REFERENCE itself: the Tx-side spectrum estimate (SURVEY.md 8f
row f4) at the DFT lengths past 256, where the periodogram is 4096 / 8192 points long.

Build-container-only tool, in the style of make_golden.py: it imports the reference's Python packages from
/root/reference/python (never copied, never shipped) under the same identity `numba` stub and writes one small
.npz next to this script.  Nothing under tests/ or the library imports this module; the GPU box never runs it.

Contents:
  * the reference's periodogram (wOFDMSystem.__psd_estimate, timefreq_simulation.py:104-124) at FL = 4096 and
    8192 (N = 512 / 1024, FL = 8 N) on seeded complex Gaussian waveforms: an exact multiple of FL, FL + N and a
    long run.  The waveform is not stored: `pl<FL>_<tag>_seed` / `_len` rebuild it bit for bit as
    ((rs.randn(len) + 1j rs.randn(len)) / sqrt(2)).astype(complex64) with rs = RandomState(seed).
  * estimate_obr at N = 512 and 1024, CP 12, for wtx / CPW / wrx / CPwtx with the recipe of make_golden.py's
    fixture_psd_slices (tail vectors from tail_vectors(), the symbols from np.random.seed(<seed>)): the
    periodograms X_est_* (float32) and the OBR figures obr_*.

Usage:  python tests/golden/make_golden_psd_large.py
"""
import os
import sys
import tempfile

import numpy as np

REF = "/root/reference/python"
HERE = os.path.dirname(os.path.abspath(__file__))

if not os.path.isdir(REF):
    sys.exit("make_golden_psd_large.py: %s not found - this tool only runs in the build container" % REF)

sys.dont_write_bytecode = True
_tmp = tempfile.mkdtemp(prefix="wofdm_golden_")
os.makedirs(os.path.join(_tmp, "numba"))
with open(os.path.join(_tmp, "numba", "__init__.py"), "w") as f:
    f.write("def _ident(*a, **k):\n"
            "    if len(a) == 1 and callable(a[0]) and not k:\n"
            "        return a[0]\n"
            "    return lambda fn: fn\n"
            "njit = jit = _ident\n")
sys.path[:0] = [_tmp, REF]

from ofdm_utils import timefreq_simulation as tf  # noqa: E402  (reference)
from optimization_tools.utils import reduce_variable_tx  # noqa: E402  (reference)

TAILS = {"wtx": (8, 0), "wrx": (0, 10), "CPW": (8, 10), "CPwtx": (8, 0)}
SYSTEMS = ("wtx", "CPW", "wrx", "CPwtx")


def tail_vectors(system, rs):
    """make_golden.py's non-RC 'optimised' Tx tail vector (x0 = flat level, then the tail)"""
    btx, _ = TAILS[system]
    if btx == 0:
        return np.array([1.0])
    return np.concatenate(([1.0 + 0.05 * rs.randn()], np.sort(rs.uniform(0.02, 0.98, btx))[::-1]))


def waveform(seed, length):
    rs = np.random.RandomState(seed)
    return ((rs.randn(length) + 1j * rs.randn(length)) / np.sqrt(2)).astype(np.complex64)


def main():
    psd = tf.wOFDMSystem._wOFDMSystem__psd_estimate
    out = {}
    seed = 4100
    for n_fft in (512, 1024):
        fl = 8 * n_fft
        for tag, length in (("exact", 2 * fl), ("plusN", fl + n_fft), ("long", 5 * fl + 3 * n_fft)):
            key = "pl%d_%s" % (fl, tag)
            out[key + "_seed"] = np.array(seed)
            out[key + "_len"] = np.array(length)
            out[key + "_psd"] = psd(waveform(seed, length).astype(np.complex128), fl).astype(np.float32)
            seed += 1
    cp = 12
    out["obr_cp"] = np.array(cp)
    for n_fft, tail_seed in ((512, 79), (1024, 80)):
        rs = np.random.RandomState(tail_seed)
        for i, system in enumerate(SYSTEMS):
            btx, brx = TAILS[system]
            xt = tail_vectors(system, rs)
            m = tf.wOFDMSystem(system, n_fft, cp, btx, brx, _tmp)
            win = np.diagflat(reduce_variable_tx(n_fft, cp, m.cs_len, btx) @ xt.reshape(-1, 1))
            sym_seed = 3000 + 10 * n_fft // 512 + i
            np.random.seed(sym_seed)
            opt, rc, cpd = m.estimate_obr(win, 200e-9)
            pre = "obr%d_%s_" % (n_fft, system)
            out[pre + "seed"] = np.array(sym_seed)
            out[pre + "xt"] = xt
            for tag, d in zip(("opt", "rc", "cp"), (opt, rc, cpd)):
                out[pre + "X_est_" + tag] = np.asarray(d["X_est_" + tag]).astype(np.float32)
                out[pre + "obr_" + tag] = np.asarray(d["obr_" + tag])
    path = os.path.join(HERE, "psd_large.npz")
    np.savez_compressed(path, **out)
    print("%s %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
