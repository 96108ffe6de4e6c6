"""wofdm_rx_profile_coded_frame and wofdm_viterbi_decode_long without a GPU: their place in the public header and the binding, and
the argument checks -- the new conditions of include/wofdm.h in their documented order, each answered before the device is touched
(a call that passes the checks ends in WOFDM_E_HIP: device 99 does not exist), and a failed call leaves the nine outputs as they
were.  The pattern, the shapes and the points are tests/test_rx_profile_coded_abi.py's.  (WOFDM_E_UNSUPPORTED for T >
WOFDM_CODE_LONG_MAX_STEPS cannot be reached through the profile call -- n_fft <= 1024, k <= 6 and S <= 64 give T <= 294 912 --, so
it is shown on the decoder alone.)"""
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
OK = (0, (0, 0, 0))


def _call(codes=(OK,), llr_scale=0.25, perm="identity", sym_rot=0, pilots=COMB, active=None, null=(), n_codes=None, soft_bits=True,
          tracking=None, frames=FRAMES, device=99, syms=S):
    """rc of one call on small arrays (the tracking test's, one all-off point) with the codes (rate, reserved)"""
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
    ccodes = (_lib.Code * max(len(codes), 1))()
    for q, (rate, res) in zip(ccodes, codes):
        q.rate, q.reserved = rate, (C.c_int32 * 3)(*res)
    cells, NC = PAIRS * N_CH * N_SNR, max(len(codes), 1)
    outs = dict(errs=np.full((1, cells, N, 2), POISON_U, np.uint64), pw=np.full((1, cells, N), POISON_F, np.float64),
                serrs=np.full((1, cells, syms - 1, 2), POISON_U, np.uint64), spw=np.full((1, cells, syms - 1), POISON_F, np.float64),
                ppw=np.full((1, cells, 2), POISON_F, np.float64), bpen=np.full((1, cells, 2, N), POISON_F, np.float64),
                spen=np.full((1, cells, 2, syms - 1), POISON_F, np.float64), ferrs=np.full((1, cells, NC, 2), POISON_U, np.uint64),
                sbits=np.full((cells, FRAMES, 1, syms - 1, N, 8), POISON_B, np.int8))
    a.update(outs)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_coded_frame(
        C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], 2, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"], 1, cpts, 2, ptr["scales"],
        ptr["pilots"], None if "tracking" in null else ctps, C.c_float(llr_scale), ptr["perm"], len(codes) if n_codes is None else n_codes,
        None if "codes" in null else ccodes, sym_rot,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"], ptr["ferrs"],
        ptr["sbits"] if soft_bits else None)
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_B if v.dtype == np.int8 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_both_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_coded_frame\((.*?)\);", hdr, flags=re.M | re.S)
    cod = re.search(r"^int wofdm_rx_profile_coded\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and cod

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, cargs = args_of(m.group(1)), args_of(cod.group(1))
    # every argument of the coded call through `codes`, sym_rot, the seven tracking outputs, frame_errs, soft_bits
    assert cargs[24] == "const wofdm_code *codes" and cargs[32:] == ["uint64_t *code_errs", "int8_t *soft_bits"]
    assert args == cargs[:25] + ["int32_t sym_rot"] + cargs[25:32] + ["uint64_t *frame_errs", "int8_t *soft_bits"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_coded_frame.argtypes
    assert len(at) == len(args) == 35 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.c_float if arg.startswith("float ") else
                     C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else
                     C.POINTER(_lib.TrackingPoint) if "wofdm_tracking_point" in arg else
                     C.POINTER(_lib.Code) if "wofdm_code " in arg else C.c_void_p), arg
    assert re.search(r"^#define WOFDM_CODE_LONG_MAX_STEPS 1048576$", hdr, flags=re.M) and _lib.CODE_LONG_MAX_STEPS == 1048576
    link = open(os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "wofdm_link.h")).read()
    assert re.search(r"^#define WOFDM_CODE_LONG_STEPS 1048576\b", link, flags=re.M)
    dec = re.search(r"^int wofdm_viterbi_decode_long\((.*?)\);", hdr, flags=re.M | re.S)
    old = re.search(r"^int wofdm_viterbi_decode\((.*?)\);", hdr, flags=re.M | re.S)
    assert args_of(dec.group(1)) == args_of(old.group(1))
    assert list(lib.wofdm_viterbi_decode_long.argtypes) == list(lib.wofdm_viterbi_decode.argtypes)
    for name in ("wofdm_rx_profile_coded_frame", "wofdm_viterbi_decode_long"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("RxProfileCodedFrame", "frame_interleaver", "default_sym_rot", "viterbi_decode_long_gpu", "frame_profile_coded_frame",
                 "rx_profile_coded_frame_host", "rx_profile_coded_frame_gpu", "rx_profile_coded_frame_chunk_frames", "coded_frame_ber",
                 "coded_fer", "coded_frame_for_window_file"):
        assert hasattr(W, name), name
    assert R.default_sym_rot(448, 14) == 32 and R.default_sym_rot(56, 5) == 11


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _err()
    assert _call(codes=[OK, (1, (0, 0, 0)), (2, (0, 0, 0)), OK]) == -3
    assert _call(perm=None) == -3 and _call(soft_bits=False) == -3
    assert _call(perm=R.default_interleaver(N_C), sym_rot=R.default_sym_rot(N_C, S - 1)) == -3
    assert _call(sym_rot=N_C - 1) == -3
    assert _call(pilots=None, sym_rot=4 * N - 1) == -3
    assert _call(tracking=(1, 1, (0, 0))) == -3
    assert _call(syms=2) == -3                                         # one data symbol: the per-symbol codeword
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out


def test_the_new_checks_fire_in_order():
    for bad in (-1, N_C, N_C + 5):
        assert _call(sym_rot=bad) == -1 and "sym_rot" in _err(), bad
    assert _call(pilots=None, sym_rot=N_C) == -3                       # (n_c is the data bins': 4 N without a comb)
    assert _call(null=("ferrs",)) == -1 and "frame_errs" in _err()
    # one data bin of 16-QAM over S - 1 = 3 symbols: n_f = 12, T = 6 at rate 1/2, 8 at 2/3, 9 at 3/4 -- and T = 2, 2, 3 per symbol,
    # which the per-symbol call refuses and this one does not ask about
    one = np.zeros(N, np.uint8)
    one[[5, 9]] = 1
    r34, r23 = (2, (0, 0, 0)), (1, (0, 0, 0))
    assert _call(active=one, pilots=(5,), codes=[r34, r23]) == -3
    assert _call(active=one, pilots=(5,), codes=[r34, OK]) == -1 and "codes[1]" in _err() and "steps" in _err()
    # with a postamble two data symbols are left: n_f = 8, T = 4, 5, 6
    assert _call(active=one, pilots=(5,), codes=[r34], tracking=(0, 1, (0, 0))) == -1 and "steps" in _err()
    # the documented order: sym_rot before frame_errs before the codes' lengths
    assert _call(sym_rot=-1, null=("ferrs",)) == -1 and "sym_rot" in _err()
    assert _call(active=one, pilots=(5,), codes=[OK], sym_rot=4) == -1 and "sym_rot" in _err()
    assert _call(active=one, pilots=(5,), codes=[OK], null=("ferrs",)) == -1 and "frame_errs" in _err()


def test_the_coded_calls_checks_come_first():
    assert _call(null=("codes",), sym_rot=-1) == -1 and "NULL" in _err()
    for bad in (0.0, -0.25, np.nan, np.inf):
        assert _call(llr_scale=bad, sym_rot=-1) == -1 and "llr_scale" in _err(), bad
    assert _call(codes=(), n_codes=0, sym_rot=-1) == -1 and "n_codes" in _err()
    assert _call(codes=[OK] * 4, n_codes=5, sym_rot=-1) == -2 and "n_codes" in _err()
    assert _call(codes=[OK, (3, (0, 0, 0))], sym_rot=-1) == -1 and "codes[1].rate" in _err()
    assert _call(codes=[OK, (2, (0, 0, 7))], sym_rot=-1) == -1 and "codes[1].reserved" in _err()
    for bad in (np.zeros(N_C), np.arange(N_C) + 1, np.r_[np.arange(N_C - 1), -1]):
        assert _call(perm=bad, sym_rot=-1) == -1 and "perm" in _err()
    cells = PAIRS * N_CH * N_SNR
    frames = (1 << 30) // (cells * (S - 1) * N * 8) + 1
    assert _call(frames=frames, sym_rot=-1) == -2 and "soft_bits" in _err()
    assert _call(frames=frames, soft_bits=False) == -3
    # and the tracking call's own before those -- a postamble needs three symbols, so S = 2 with post (no data symbol) is refused
    assert _call(null=("tracking",), llr_scale=np.nan) == -1 and "NULL" in _err()
    assert _call(tracking=(2, 0, (0, 0)), llr_scale=np.nan) == -1 and "tracking[0]" in _err()
    assert _call(syms=2, tracking=(0, 1, (0, 0))) == -1 and "post" in _err()
    assert _call(pilots=range(N), null=("codes",)) == -1 and "data bin" in _err()
    for name in ("scales", "bpen", "w_tx", "errs"):
        assert _call(null=(name,)) == -1, name


def test_the_long_decoder_alone_checks_before_the_device():
    lib = _lib.load()
    big = (1 << 21) + 2
    soft, bits, metric = np.zeros((1, big), np.int8), np.full((1, (1 << 20) + 1), 7, np.uint8), np.full(2, 7, np.int32)

    def dec(rate=0, n_c=56, perm=None, n_cw=1, s=soft, b=bits, device=99):
        p = None if perm is None else np.asarray(perm, np.int32)
        rc = lib.wofdm_viterbi_decode_long(device, rate, n_c, None if p is None else p.ctypes.data, n_cw,
                                           None if s is None else s.ctypes.data, None if b is None else b.ctypes.data, metric.ctypes.data)
        assert (bits == 7).all() and (metric == 7).all()
        return rc
    assert dec() == -3 and "device" in _err()
    assert dec(perm=R.default_interleaver(56)) == -3
    assert dec(s=None) == -1 and dec(b=None) == -1
    assert dec(rate=3) == -1 and dec(rate=-1) == -1
    assert dec(n_c=0) == -1 and dec(n_cw=0) == -1
    assert dec(rate=0, n_c=13) == -1 and "steps" in _err() and dec(rate=0, n_c=14) == -3
    # what wofdm_viterbi_decode refuses as too long goes as far as the device
    assert lib.wofdm_viterbi_decode(99, 0, 9218, None, 1, soft.ctypes.data, bits.ctypes.data, metric.ctypes.data) == -2
    assert dec(rate=0, n_c=9218) == -3 and dec(rate=2, n_c=6149) == -3 and dec(rate=1, n_c=20000) == -3
    # T = 2^20 is taken, 2^20 + 1 is not
    assert R.code_steps(0, big - 2) == 1 << 20
    assert dec(rate=0, n_c=big - 2) == -3
    assert dec(rate=0, n_c=big) == -2 and "steps" in _err()
    assert dec(perm=np.zeros(56)) == -1 and "perm" in _err()
