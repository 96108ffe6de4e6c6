"""wofdm_rx_profile_ldpc, wofdm_ldpc_decode and wofdm_ldpc_lift without a GPU: their place in the public header and the binding,
and the argument checks -- the new conditions of include/wofdm.h in their documented order, each answered before the device is
touched (a call that passes the checks ends in WOFDM_E_HIP: device 99 does not exist), and a failed call leaves the nine outputs as
they were.  The pattern, the shapes and the points are tests/test_rx_profile_coded_frame_abi.py's.  n = 16384 passes the decoder's
checks and n = 16385 is refused by the decoder alone -- the profile call splits such a frame into W = 2 words."""
import ctypes as C
import os
import re

import numpy as np

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import rx_profile as R
from wofdm_amd import variants as V

import test_rx_profile_link_abi as LA
import test_rx_profile_tracking_abi as TA

ROOT = LA.ROOT
POISON_U, POISON_F, POISON_B = LA.POISON_U, LA.POISON_F, 0x5A
N, S, TAPS, N_CH, N_SNR, PAIRS = LA.N, LA.S, LA.TAPS, LA.N_CH, LA.N_SNR, LA.PAIRS
COMB = TA.COMB
N_C = 4 * (N - len(COMB))
FRAMES = 3
OK = (4, 8, 30, 0)


def _call(codes=(OK,), llr_scale=0.25, perm="identity", sym_rot=0, pilots=COMB, active=None, null=(), n_codes=None, soft_bits=True,
          tracking=None, frames=FRAMES, device=99, syms=S, N=N):
    """rc of one call on small arrays (the tracking test's, one all-off point) with the codes (J, L, max_iter, reserved)"""
    st = V.make_structure("CPW", N, 32)
    cfg = W.make_cfg(st, 4, syms, TAPS, N_CH, N_SNR, PAIRS, seed=3, frames_per_cell=frames)
    B, P = st.stride, st.sym_len
    n_knots, knot_step = syms + 2, B
    pil = None
    if pilots is not None:
        pil = np.zeros(N, np.uint8)
        pil[list(pilots)] = 1
    n_data = int((np.ones(N, bool) if active is None else np.asarray(active) != 0).sum()) - (0 if pil is None else int(pil.sum()))
    a = dict(w_tx=np.ones((PAIRS, P), np.float32), w_rx=np.ones((PAIRS, N + st.tail_rx), np.float32),
             h=np.ones((N_CH, TAPS, 2), np.float32), snr=np.full(N_SNR, 10.0, np.float32),
             active=None if active is None else np.asarray(active, np.uint8), mask=None,
             h_track=np.ones((2, N_CH, n_knots, TAPS, 2), np.float32), aci_active=np.ones(N, np.uint8),
             aci_h=np.ones((N_CH, TAPS, 2), np.float32), ref_power=np.ones(PAIRS, np.float32), scales=np.asarray((1.0, 0.5), np.float32),
             pilots=pil, perm=None if perm is None else (np.arange(4 * n_data, dtype=np.int32) if isinstance(perm, str)
                                                         else np.asarray(perm, np.int32)))
    cpts = (_lib.LinkPoint * 1)()
    for f, v in LA.OK_POINT.items():
        if f == "reserved":
            cpts[0].reserved = (C.c_int32 * 4)(*v)
        else:
            setattr(cpts[0], f, v)
    ctps = (_lib.TrackingPoint * 1)()
    cpe, post, res = tracking or (0, 0, (0, 0))
    ctps[0].cpe, ctps[0].post, ctps[0].reserved = cpe, post, (C.c_int32 * 2)(*res)
    ccodes = (_lib.LdpcCode * max(len(codes), 1))()
    for q, (J, L, m, res) in zip(ccodes, codes):
        q.J, q.L, q.max_iter, q.reserved = J, L, m, res
    cells, NC = PAIRS * N_CH * N_SNR, max(len(codes), 1)
    outs = dict(errs=np.full((1, cells, N, 2), POISON_U, np.uint64), pw=np.full((1, cells, N), POISON_F, np.float64),
                serrs=np.full((1, cells, syms - 1, 2), POISON_U, np.uint64), spw=np.full((1, cells, syms - 1), POISON_F, np.float64),
                ppw=np.full((1, cells, 2), POISON_F, np.float64), bpen=np.full((1, cells, 2, N), POISON_F, np.float64),
                spen=np.full((1, cells, 2, syms - 1), POISON_F, np.float64), lerrs=np.full((1, cells, NC, 4), POISON_U, np.uint64),
                sbits=np.full((cells, FRAMES, 1, syms - 1, N, 8), POISON_B, np.int8))
    a.update(outs)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_ldpc(
        C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], 2, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"], 1, cpts, 2, ptr["scales"],
        ptr["pilots"], None if "tracking" in null else ctps, C.c_float(llr_scale), ptr["perm"], len(codes) if n_codes is None else n_codes,
        None if "codes" in null else ccodes, sym_rot,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"], ptr["lerrs"],
        ptr["sbits"] if soft_bits else None)
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_B if v.dtype == np.int8 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_all_three_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_ldpc\((.*?)\);", hdr, flags=re.M | re.S)
    frm = re.search(r"^int wofdm_rx_profile_coded_frame\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and frm

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, fargs = args_of(m.group(1)), args_of(frm.group(1))
    # every argument of the coded-frame call through perm, n_codes, the LDPC codes, sym_rot, the seven tracking outputs, ldpc_errs,
    # soft_bits
    assert fargs[24] == "const wofdm_code *codes" and fargs[33] == "uint64_t *frame_errs"
    assert args == fargs[:24] + ["const wofdm_ldpc_code *codes"] + fargs[25:33] + ["uint64_t *ldpc_errs", "int8_t *soft_bits"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_ldpc.argtypes
    assert len(at) == len(args) == 35 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.c_float if arg.startswith("float ") else
                     C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else
                     C.POINTER(_lib.TrackingPoint) if "wofdm_tracking_point" in arg else
                     C.POINTER(_lib.LdpcCode) if "wofdm_ldpc_code " in arg else C.c_void_p), arg
    assert C.sizeof(_lib.LdpcCode) == 16
    assert re.search(r"^#define WOFDM_LDPC_MAX_BITS 16384$", hdr, flags=re.M) and _lib.LDPC_MAX_BITS == 16384
    link = open(os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "wofdm_link.h")).read()
    assert re.search(r"^#define WOFDM_LDPC_BITS 16384\b", link, flags=re.M)
    assert re.search(r"^int wofdm_ldpc_decode\(", hdr, flags=re.M) and re.search(r"^int wofdm_ldpc_lift\(", hdr, flags=re.M)
    for name in ("wofdm_rx_profile_ldpc", "wofdm_ldpc_decode", "wofdm_ldpc_lift"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("RxProfileLdpc", "ldpc_lift", "ldpc_edges", "ldpc_encode", "ldpc_decode", "ldpc_decode_gpu", "frame_profile_ldpc",
                 "rx_profile_ldpc_host", "rx_profile_ldpc_gpu", "rx_profile_ldpc_chunk_frames", "ldpc_ber", "ldpc_fer",
                 "ldpc_mean_iterations", "ldpc_for_window_file"):
        assert hasattr(W, name), name


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _err()
    assert _call(codes=[OK, (3, 6, 1, 0), (6, 24, 64, 0), (4, 16, 20, 0)]) == -3
    assert _call(perm=None) == -3 and _call(soft_bits=False) == -3
    assert _call(perm=R.default_interleaver(N_C), sym_rot=R.default_sym_rot(N_C, S - 1)) == -3
    assert _call(sym_rot=N_C - 1) == -3
    assert _call(pilots=None, sym_rot=4 * N - 1) == -3
    assert _call(tracking=(1, 1, (0, 0))) == -3
    assert _call(syms=2) == -3
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out


def test_a_frame_above_the_longest_word_is_split():
    # N = 1024 without a comb: 4096 coded bits per symbol; over 5 data symbols n_f = 20480 > 16384, W = 2 words of 10240; over 4
    # it is one word of 16384, the longest; over 15, W = 4 words of 15360 -- every code takes them
    assert R.ldpc_frame_words(4096 * 5) == (2, 10240) and R.ldpc_frame_words(4096 * 4) == (1, 16384)
    assert R.ldpc_frame_words(4096 * 15) == (4, 15360)
    for syms in (5, 6, 16):
        assert _call(N=1024, pilots=None, syms=syms, soft_bits=False, frames=1, codes=[OK, (6, 24, 5, 0), (3, 4, 5, 0)]) == -3, syms
    # ... and with a postamble the frame of S = 6 is the longest single word again
    assert _call(N=1024, pilots=None, syms=6, soft_bits=False, frames=1, tracking=(0, 1, (0, 0))) == -3
    assert R.ldpc_frame_words(16384) == (1, 16384) and R.ldpc_frame_words(16385) == (2, 8192)
    assert R.ldpc_frame_words(3 * 16384 + 2) == (4, 12288)              # (two positions left over)


def test_the_new_checks_fire_in_order():
    for bad in (-1, N_C, N_C + 5):
        assert _call(sym_rot=bad) == -1 and "sym_rot" in _err(), bad
    assert _call(pilots=None, sym_rot=N_C) == -3                       # (n_c is the data bins': 4 N without a comb)
    assert _call(null=("lerrs",)) == -1 and "ldpc_errs" in _err()
    for bad, what in (((2, 8, 30, 0), "J"), ((7, 12, 30, 0), "J"), ((4, 4, 30, 0), "L"), ((4, 25, 30, 0), "L"), ((4, 8, 0, 0), "max_iter"),
                      ((4, 8, 65, 0), "max_iter"), ((4, 8, 30, 1), "reserved")):
        assert _call(codes=[OK, bad]) == -1 and "codes[1]." + what in _err(), bad
    # code by code: the first code's reserved before the second code's J; within a code J, L, max_iter, reserved
    assert _call(codes=[(4, 8, 30, 1), (2, 8, 30, 0)]) == -1 and "codes[0].reserved" in _err()
    assert _call(codes=[(2, 4, 0, 1)]) == -1 and "codes[0].J" in _err()
    assert _call(codes=[(4, 4, 0, 1)]) == -1 and "codes[0].L" in _err()
    assert _call(codes=[(4, 8, 0, 1)]) == -1 and "codes[0].max_iter" in _err()
    # five data bins of 16-QAM over S - 1 = 3 symbols: n_f = 60 -- (3, 6) and (4, 8) lift to 11 and keep 27 and 16 information
    # bits, (6, 24) lifts to 29 and keeps none; with a postamble n_f = 40 and (4, 8) keeps none either
    few = np.zeros(N, np.uint8)
    few[[5, 9, 20, 31, 47, 60]] = 1
    assert (R.ldpc_lift(3, 6, 60), R.ldpc_lift(4, 8, 60), R.ldpc_lift(3, 6, 40)) == (11, 11, 11)
    assert _call(active=few, pilots=(5,), codes=[(3, 6, 30, 0), OK]) == -3
    assert _call(active=few, pilots=(5,), codes=[OK, (6, 24, 30, 0)]) == -1 and "codes[1]" in _err() and "information" in _err()
    assert _call(active=few, pilots=(5,), codes=[(3, 6, 30, 0)], tracking=(0, 1, (0, 0))) == -3
    assert _call(active=few, pilots=(5,), codes=[OK], tracking=(0, 1, (0, 0))) == -1 and "information" in _err()
    # the documented order: sym_rot before ldpc_errs before the codes
    assert _call(sym_rot=-1, null=("lerrs",), codes=[(2, 8, 30, 0)]) == -1 and "sym_rot" in _err()
    assert _call(null=("lerrs",), codes=[(2, 8, 30, 0)]) == -1 and "ldpc_errs" in _err()


def test_the_coded_frame_calls_checks_come_first():
    assert _call(null=("codes",), sym_rot=-1) == -1 and "NULL" in _err()
    for bad in (0.0, -0.25, np.nan, np.inf):
        assert _call(llr_scale=bad, sym_rot=-1) == -1 and "llr_scale" in _err(), bad
    assert _call(codes=(), n_codes=0, sym_rot=-1) == -1 and "n_codes" in _err()
    assert _call(codes=[OK] * 4, n_codes=5, sym_rot=-1) == -2 and "n_codes" in _err()
    for bad in (np.zeros(N_C), np.arange(N_C) + 1, np.r_[np.arange(N_C - 1), -1]):
        assert _call(perm=bad, sym_rot=-1) == -1 and "perm" in _err()
    cells = PAIRS * N_CH * N_SNR
    frames = (1 << 30) // (cells * (S - 1) * N * 8) + 1
    assert _call(frames=frames, sym_rot=-1) == -2 and "soft_bits" in _err()
    assert _call(frames=frames, soft_bits=False) == -3
    # and the tracking call's own before those
    assert _call(null=("tracking",), llr_scale=np.nan) == -1 and "NULL" in _err()
    assert _call(tracking=(2, 0, (0, 0)), llr_scale=np.nan) == -1 and "tracking[0]" in _err()
    assert _call(syms=2, tracking=(0, 1, (0, 0))) == -1 and "post" in _err()
    assert _call(pilots=range(N), null=("codes",)) == -1 and "data bin" in _err()
    for name in ("scales", "bpen", "w_tx", "errs"):
        assert _call(null=(name,)) == -1, name


def test_the_decoder_alone_checks_before_the_device():
    lib = _lib.load()
    soft, bits = np.zeros((2, 16385), np.int8), np.full((2, 16385), 7, np.uint8)
    iters, conv = np.full(2, 7, np.int32), np.full(2, 7, np.uint8)

    def dec(J=4, L=8, max_iter=30, n=488, perm=None, n_cw=1, s=soft, b=bits, it=iters, cv=conv, device=99):
        p = None if perm is None else np.asarray(perm, np.int32)
        rc = lib.wofdm_ldpc_decode(device, J, L, max_iter, n, None if p is None else p.ctypes.data, n_cw,
                                   None if s is None else s.ctypes.data, None if b is None else b.ctypes.data,
                                   None if it is None else it.ctypes.data, None if cv is None else cv.ctypes.data)
        assert (bits == 7).all() and (iters == 7).all() and (conv == 7).all()
        return rc
    assert dec() == -3 and "device" in _err()
    assert dec(perm=R.default_interleaver(488)) == -3 and dec(it=None, cv=None) == -3 and dec(n_cw=2) == -3
    assert dec(s=None) == -1 and dec(b=None) == -1
    for J, L in ((2, 8), (7, 12), (4, 4), (4, 25)):
        assert dec(J=J, L=L) == -1, (J, L)
    assert dec(max_iter=0) == -1 and dec(max_iter=65) == -1 and dec(max_iter=1) == -3 and dec(max_iter=64) == -3
    assert dec(n=0) == -1 and dec(n_cw=0) == -1
    # n = 16384 is taken by every check, 16385 is not -- before the code is looked at
    assert dec(n=16384) == -3 and dec(J=6, L=24, n=16384) == -3 and dec(J=3, L=4, n=16384) == -3
    assert dec(n=16385) == -2 and "16384" in _err()
    assert dec(J=6, L=24, n=60) == -1 and "information" in _err() and dec(J=3, L=4, n=16) == -3
    assert dec(perm=np.zeros(488)) == -1 and "perm" in _err()
    # the order: NULL, the code's ranges, max_iter, the counts, the length, K, perm
    assert dec(s=None, J=2) == -1 and "NULL" in _err()
    assert dec(J=2, max_iter=0) == -1 and "J=" in _err()
    assert dec(max_iter=0, n=0) == -1 and "max_iter" in _err()
    assert dec(n=16385, perm=np.zeros(16385)) == -2
