"""wofdm_rx_profile without a GPU: its place in the public header and the binding, and its argument checks -- every
WOFDM_E_INVALID / WOFDM_E_UNSUPPORTED condition of include/wofdm.h is answered before the device is touched (this machine
has none: a call that passes the checks ends in WOFDM_E_HIP), and a failed call leaves the outputs as they were."""
import ctypes as C
import os
import re

import numpy as np

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_U, POISON_F = 0xA5A5A5A5A5A5A5A5, -12345.678


def _call(st=None, k=4, S=4, n_taps=3, n_ch=2, n_snr=2, pairs=2, frames=3, device=99, null=(), mask=False, active=None,
          edit=None, cfg_edit=None):
    """rc of one call on small arrays; `edit` changes the arrays, `cfg_edit` the cfg, before the call"""
    st = V.make_structure("CPW", 128, 32) if st is None else st
    cfg = W.make_cfg(st, k, S, n_taps, n_ch, n_snr, pairs, seed=3, frames_per_cell=frames)
    P, NW, N = max(st.sym_len, 1), max(st.n_fft + st.tail_rx, 1), max(st.n_fft, 1)
    a = dict(w_tx=np.ones((max(pairs, 1), P), np.float32), w_rx=np.ones((max(pairs, 1), NW), np.float32),
             h=np.ones((max(n_ch, 1), max(n_taps, 1), 2), np.float32), snr=np.full(max(n_snr, 1), 10.0, np.float32),
             active=None if active is None else np.ascontiguousarray(active, np.uint8),
             mask=np.ones(2 * P - 1, np.float32) if mask else None)
    cells = max(pairs, 1) * max(n_ch, 1) * max(n_snr, 1)
    errs = np.full((cells, N, 2), POISON_U, np.uint64)
    pw = np.full((cells, N), POISON_F, np.float64)
    a.update(errs=errs, pw=pw)
    if edit:
        edit(a)
    if cfg_edit:
        cfg_edit(cfg)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile(None if "cfg" in null else C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"],
                                      ptr["snr"], ptr["active"], ptr["mask"], ptr["errs"], ptr["pw"])
    assert (errs == POISON_U).all() and (pw == POISON_F).all()          # no failed call writes its outputs
    return rc


def _set(name, index, value):
    def edit(a):
        a[name].reshape(-1)[index] = value
    return edit


def test_rx_profile_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile\((.*?)\);", hdr, flags=re.M | re.S)
    assert m
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["const wofdm_cfg *cfg", "int device", "const float *w_tx", "const float *w_rx", "const float *h",
                    "const float *snr_db", "const uint8_t *active", "const float *tx_mask", "uint64_t *errs",
                    "double *err_power"]
    lib = _lib.load()
    assert len(lib.wofdm_rx_profile.argtypes) == len(args)
    assert lib.wofdm_rx_profile.argtypes[0] == C.POINTER(_lib.Cfg) and lib.wofdm_rx_profile.argtypes[1] == C.c_int
    assert all(t == C.c_void_p for t in lib.wofdm_rx_profile.argtypes[2:])
    assert re.search(r"^int wofdm_rx_profile_kernel_ms\(float \*ms\);", hdr, flags=re.M)
    assert re.search(r"^#define WOFDM_RX_PROFILE_CHUNK_BYTES \(256u << 20\)", hdr, flags=re.M)
    assert _lib.RX_PROFILE_CHUNK_BYTES == 256 << 20
    for name in ("wofdm_rx_profile", "wofdm_rx_profile_kernel_ms"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("rx_profile_gpu", "rx_profile_host", "frame_profile", "ber_per_bin", "evm_db", "profile_for_window_file"):
        assert hasattr(W, name)
    ms = C.c_float(-1.0)
    assert lib.wofdm_rx_profile_kernel_ms(C.byref(ms)) == 0 and ms.value == 0.0         # no successful call yet
    assert lib.wofdm_rx_profile_kernel_ms(None) == -1


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _lib.load().wofdm_last_error().decode()
    assert _call(device=-1) == -3
    assert _call(mask=True, active=CM.half_band_allocation(128)) == -3
    # served here although a plan refuses them: the mask at N = 1024, and a frame above 160 KiB of LDS
    assert _call(st=V.make_structure("wtx", 1024, 128), S=2, mask=True) == -3
    assert _call(st=V.make_structure("wtx", 1024, 56), S=16) == -3
    assert _call(n_taps=21) == -3 and _call(S=16) == -3 and _call(S=2) == -3
    assert _call(frames=0) == -3


def test_rx_profile_refuses_invalid_arguments():
    for name in ("cfg", "w_tx", "w_rx", "h", "snr", "errs"):
        assert _call(null=(name,)) == -1, name
    assert _call(null=("pw",)) == -3                                   # err_power is optional
    for bad in (np.nan, np.inf, -np.inf):
        assert _call(edit=_set("w_tx", 5, bad)) == -1
        assert _call(edit=_set("w_tx", -1, bad)) == -1                 # (the last pair's last sample)
        assert _call(edit=_set("w_rx", -1, bad)) == -1
        assert _call(edit=_set("h", -1, bad)) == -1
        assert _call(edit=_set("snr", 1, bad)) == -1
        assert _call(mask=True, edit=_set("mask", -1, bad)) == -1
    assert _call(active=np.zeros(128, np.uint8)) == -1
    assert "loads no subcarrier" in _lib.load().wofdm_last_error().decode()
    for field in ("n_channels", "n_snr", "n_window_pairs"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, 0)) == -1, field
    for field in ("cp", "cs", "tail_tx", "prefix_rm", "circ_shift", "n_taps"):
        assert _call(cfg_edit=lambda c, f=field: setattr(c, f, -1)) == -1, field
    assert _call(cfg_edit=lambda c: setattr(c, "n_taps", 0)) == -1
    assert _call(cfg_edit=lambda c: setattr(c, "circ_shift", 128)) == -1
    # a negative tail_rx with the geometry identity kept
    assert _call(cfg_edit=lambda c: (setattr(c, "prefix_rm", c.prefix_rm + c.tail_rx + 2), setattr(c, "tail_rx", -2))) == -1


def test_rx_profile_refuses_what_lies_outside_its_limits():
    for n in (32, 96, 2048):
        assert _call(cfg_edit=lambda c, n=n: setattr(c, "n_fft", n)) == -2, n
    for k in (1, 3, 8):
        assert _call(k=k) == -2, k
    for S in (1, 17):
        assert _call(S=S) == -2, S
    assert _call(n_taps=22) == -2
    # tail_rx even and <= 64; N + tail_rx + prefix_rm == P - tail_tx
    assert _call(cfg_edit=lambda c: (setattr(c, "tail_rx", 11), setattr(c, "prefix_rm", c.prefix_rm - 1))) == -2
    assert "tail_rx" in _lib.load().wofdm_last_error().decode()
    assert _call(st=V.Structure("wrx", 128, 64, 0, 66, 33, 31, 0)) == -2                 # 128 + 66 + 31 == 225 == P
    assert "tail_rx" in _lib.load().wofdm_last_error().decode()
    assert _call(st=V.Structure("wrx", 128, 64, 0, 64, 32, 32, 0)) == -3
    assert _call(cfg_edit=lambda c: setattr(c, "prefix_rm", c.prefix_rm + 1)) == -2
    assert "prefix_rm" in _lib.load().wofdm_last_error().decode()
    # the Tx-side limits of wofdm_tx_papr: cp, cs <= n_fft, 2 tail_tx <= P; masked: 3 P - 2 <= 8 n_fft
    assert _call(st=V.Structure("wtx", 128, 129, 0, 0, 0, 129, 0)) == -2
    assert _call(st=V.Structure("wtx", 128, 0, 0, 0, 129, 129, 0)) == -2
    assert _call(st=V.Structure("wtx", 128, 128, 0, 0, 128, 256, 0)) == -3
    # (2 tail_tx > P leaves a stride below n_fft, so the identity then needs a negative prefix_rm: that check answers first)
    assert _call(st=V.Structure("wtx", 128, 0, 65, 0, 0, -65, 0)) == -1
    assert "negative length" in _lib.load().wofdm_last_error().decode()
    assert _call(st=V.Structure("wtx", 128, 0, 65, 0, 0, 0, 0)) == -2          # ... and with prefix_rm = 0 the limit itself
    assert "2 tail_tx <= P" in _lib.load().wofdm_last_error().decode()
    pmax = (8 * 128 + 2) // 3
    fits = V.Structure("wrx", 128, 128, 0, 0, pmax - 256, pmax - 128, 0)
    over = V.Structure("wrx", 128, 128, 0, 0, pmax + 1 - 256, pmax + 1 - 128, 0)
    assert _call(st=fits, mask=True) == -3 and _call(st=over, mask=True) == -2 and _call(st=over) == -3
    assert "3 P - 2 <= 8 n_fft" not in _lib.load().wofdm_last_error().decode()
    # fewer than 2^28 cells (the arrays of such a call are never read: the check comes first)
    assert _call(cfg_edit=lambda c: (setattr(c, "n_channels", 1 << 14), setattr(c, "n_snr", 1 << 14))) == -2
