"""wofdm_rx_profile_coded, wofdm_viterbi_decode and wofdm_code_steps without a GPU: their place in the public header and the
binding, and the argument checks -- the new conditions of include/wofdm.h in their documented order, each answered before the
device is touched (this machine has none: a call that passes the checks ends in WOFDM_E_HIP), and a failed call leaves the nine
outputs as they were.  The pattern, the shapes and the points are tests/test_rx_profile_tracking_abi.py's."""
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


def _call(codes=((0, (0, 0, 0)),), llr_scale=0.25, perm="identity", pilots=COMB, active=None, null=(), n_codes=None, soft_bits=True,
          tracking=None, frames=FRAMES, device=99):
    """rc of one call on small arrays (the tracking test's, one all-off point) with the codes (rate, reserved)"""
    st = V.make_structure("CPW", N, 32)
    cfg = W.make_cfg(st, 4, S, TAPS, N_CH, N_SNR, PAIRS, seed=3, frames_per_cell=frames)
    B, P = st.stride, st.sym_len
    n_knots, knot_step = S + 2, B
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
                serrs=np.full((1, cells, S - 1, 2), POISON_U, np.uint64), spw=np.full((1, cells, S - 1), POISON_F, np.float64),
                ppw=np.full((1, cells, 2), POISON_F, np.float64), bpen=np.full((1, cells, 2, N), POISON_F, np.float64),
                spen=np.full((1, cells, 2, S - 1), POISON_F, np.float64), cerrs=np.full((1, cells, NC, S - 1, 2), POISON_U, np.uint64),
                sbits=np.full((cells, FRAMES, 1, S - 1, N, 8), POISON_B, np.int8))
    a.update(outs)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_coded(
        C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], 2, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"], 1, cpts, 2, ptr["scales"],
        ptr["pilots"], None if "tracking" in null else ctps, C.c_float(llr_scale), ptr["perm"], len(codes) if n_codes is None else n_codes,
        None if "codes" in null else ccodes,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"], ptr["cerrs"],
        ptr["sbits"] if soft_bits else None)
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_B if v.dtype == np.int8 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_coded_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_coded\((.*?)\);", hdr, flags=re.M | re.S)
    trk = re.search(r"^int wofdm_rx_profile_tracking\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and trk

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, targs = args_of(m.group(1)), args_of(trk.group(1))
    # every argument of the tracking call through `tracking`, the coded link's, the seven outputs, the two new ones
    assert args == targs[:21] + ["float llr_scale", "const int32_t *perm", "int32_t n_codes", "const wofdm_code *codes"] + targs[21:] + [
        "uint64_t *code_errs", "int8_t *soft_bits"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_coded.argtypes
    assert len(at) == len(args) == 34 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.c_float if arg.startswith("float ") else
                     C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else
                     C.POINTER(_lib.TrackingPoint) if "wofdm_tracking_point" in arg else
                     C.POINTER(_lib.Code) if "wofdm_code " in arg else C.c_void_p), arg
    st = re.search(r"typedef struct wofdm_code \{(.*?)\} wofdm_code;", hdr, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+)(\[\d+\])?;", st.group(1))
    assert [f for f, _ in fields] == [f for f, _ in _lib.Code._fields_] == ["rate", "reserved"]
    assert C.sizeof(_lib.Code) == 16 and fields[1][1] == "[3]"
    assert re.search(r"^#define WOFDM_CODE_MAX 4$", hdr, flags=re.M) and _lib.CODE_MAX == 4
    assert re.search(r"^#define WOFDM_CODE_MAX_STEPS 4608\b", hdr, flags=re.M) and _lib.CODE_MAX_STEPS == 4608
    dec = re.search(r"^int wofdm_viterbi_decode\((.*?)\);", hdr, flags=re.M | re.S)
    assert args_of(dec.group(1)) == ["int device", "int32_t rate", "int32_t n_c", "const int32_t *perm", "int32_t n_cw",
                                     "const int8_t *soft", "uint8_t *bits", "int32_t *metric"]
    assert list(lib.wofdm_viterbi_decode.argtypes) == [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 3
    for name in ("wofdm_rx_profile_coded", "wofdm_viterbi_decode", "wofdm_code_steps"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("RxProfileCoded", "conv_encode", "code_steps", "viterbi_decode", "viterbi_decode_gpu", "soft_bits",
                 "default_interleaver", "coded_ber", "coded_cwer", "frame_profile_coded", "rx_profile_coded_host",
                 "rx_profile_coded_gpu", "rx_profile_coded_chunk_frames", "coded_for_window_file", "LLR_SCALE"):
        assert hasattr(W, name), name
    assert R.LLR_SCALE == 0.25
    assert list(R.default_interleaver(40)) == [j for col in range(17) for j in range(col, 40, 17)]


def test_code_steps_is_the_mirrors():
    lib = _lib.load()
    for rate in (0, 1, 2):
        for n_c in list(range(0, 70)) + [672, 6143, 6144]:
            assert lib.wofdm_code_steps(rate, n_c) == R.code_steps(rate, n_c), (rate, n_c)
    assert [lib.wofdm_code_steps(r, 6144) for r in (0, 1, 2)] == [3072, 4096, 4608]
    assert lib.wofdm_code_steps(3, 56) == -1 and lib.wofdm_code_steps(-1, 56) == -1 and lib.wofdm_code_steps(0, -1) == -1


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _err()
    assert _call(codes=[(0, (0, 0, 0)), (1, (0, 0, 0)), (2, (0, 0, 0)), (0, (0, 0, 0))]) == -3
    assert _call(perm=None) == -3 and _call(soft_bits=False) == -3
    assert _call(perm=R.default_interleaver(N_C)) == -3
    assert _call(pilots=None) == -3
    assert _call(tracking=(1, 1, (0, 0))) == -3
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out


def test_coded_refuses_invalid_arguments_in_order():
    ok = (0, (0, 0, 0))
    assert _call(null=("codes",)) == -1 and "NULL" in _err()
    assert _call(null=("cerrs",)) == -1 and "NULL" in _err()
    for bad in (0.0, -0.25, np.nan, np.inf):
        assert _call(llr_scale=bad) == -1 and "llr_scale" in _err(), bad
    assert _call(codes=(), n_codes=0) == -1 and "n_codes" in _err()
    assert _call(codes=[ok] * 4, n_codes=5) == -2 and "n_codes" in _err()
    for bad in (3, -1):
        assert _call(codes=[ok, (bad, (0, 0, 0))]) == -1 and "codes[1].rate" in _err(), bad
    for res in ((1, 0, 0), (0, 0, 7)):
        assert _call(codes=[ok, (2, res)]) == -1 and "codes[1].reserved" in _err(), res
    # one data bin of 16-QAM: n_c = 4, T = 2, 2 and 3
    one = np.zeros(N, np.uint8)
    one[[5, 9]] = 1
    assert _call(active=one, pilots=(5,)) == -1 and "steps" in _err()
    few = np.zeros(N, np.uint8)
    few[:5] = 1                                                        # four data bins: n_c = 16, T = 8 / 10 / 12
    assert _call(active=few, pilots=(0,), codes=[ok, (2, (0, 0, 0))]) == -3
    few[:4] = 1
    few[4] = 0                                                         # three data bins: n_c = 12, T = 6 at rate 1/2, 9 at 3/4
    assert _call(active=few, pilots=(0,), codes=[(2, (0, 0, 0))]) == -3
    assert _call(active=few, pilots=(0,), codes=[(2, (0, 0, 0)), ok]) == -1 and "codes[1]" in _err()
    for bad in (np.zeros(N_C), np.arange(N_C) + 1, np.r_[np.arange(N_C - 1), -1]):
        assert _call(perm=bad) == -1 and "perm" in _err()
    # the documented order: an earlier condition answers first
    assert _call(llr_scale=np.nan, codes=[(3, (0, 0, 0))]) == -1 and "llr_scale" in _err()
    assert _call(codes=[(3, (1, 0, 0))]) == -1 and "rate" in _err()
    assert _call(codes=[(0, (1, 0, 0))], perm=np.zeros(N_C)) == -1 and "reserved" in _err()
    # the tracking call's own come first
    assert _call(null=("tracking",), llr_scale=np.nan) == -1 and "NULL" in _err()
    assert _call(tracking=(2, 0, (0, 0)), llr_scale=np.nan) == -1 and "tracking[0]" in _err()
    assert _call(pilots=range(N), null=("codes",)) == -1 and "data bin" in _err()
    for name in ("scales", "bpen", "w_tx", "errs"):
        assert _call(null=(name,)) == -1, name


def test_soft_bits_beyond_the_limit_are_refused():
    cells = PAIRS * N_CH * N_SNR
    frames = (1 << 30) // (cells * (S - 1) * N * 8) + 1
    assert _call(frames=frames) == -2 and "soft_bits" in _err()
    assert _call(frames=frames, soft_bits=False) == -3
    assert _call(frames=frames - 1) == -3


def test_the_decoder_alone_checks_before_the_device():
    lib = _lib.load()
    soft, bits, metric = np.zeros((2, 56), np.int8), np.full((2, 42), 7, np.uint8), np.full(2, 7, np.int32)

    def dec(rate=0, n_c=56, perm=None, n_cw=2, s=soft, b=bits, device=99):
        p = None if perm is None else np.asarray(perm, np.int32)
        rc = lib.wofdm_viterbi_decode(device, rate, n_c, None if p is None else p.ctypes.data, n_cw, None if s is None else s.ctypes.data,
                                      None if b is None else b.ctypes.data, metric.ctypes.data)
        assert (bits == 7).all() and (metric == 7).all()
        return rc
    assert dec() == -3 and "device" in _err()
    assert dec(perm=R.default_interleaver(56)) == -3
    assert dec(s=None) == -1 and dec(b=None) == -1
    assert dec(rate=3) == -1 and dec(rate=-1) == -1
    assert dec(n_c=0) == -1 and dec(n_cw=0) == -1
    assert dec(rate=0, n_c=13) == -1 and "steps" in _err() and dec(rate=0, n_c=14) == -3
    assert dec(rate=2, n_c=6148) == -2 and dec(rate=0, n_c=9216) == -3 and dec(rate=0, n_c=9218) == -2
    assert dec(perm=np.zeros(56)) == -1 and "perm" in _err()
