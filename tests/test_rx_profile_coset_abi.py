"""wofdm_rx_profile_coset, wofdm_conv_encode, wofdm_ldpc_encode and wofdm_coset_info without a GPU: their place in the public header
and the binding, and the argument checks -- the conditions of include/wofdm.h in their documented order, each answered before the
device is touched (a call that passes the checks ends in WOFDM_E_HIP: device 99 does not exist), and a failed call leaves the ten
outputs as they were.  The pattern, the shapes and the points are tests/test_rx_profile_ldpc_abi.py's."""
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
VIT = (0, (0, 0, 0))
LDPC = (4, 8, 30, 0)


def _call(codes=(VIT,), ldpc=(LDPC,), llr_scale=0.25, perm="identity", sym_rot=0, pilots=COMB, active=None, null=(), n_codes=None,
          n_ldpc=None, soft_bits=True, tracking=None, frames=FRAMES, device=99, syms=S, N=N):
    """rc of one call on small arrays (the tracking test's, one all-off point) with the Viterbi codes (rate, reserved) and the LDPC
    codes (J, L, max_iter, reserved)"""
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
    lcodes = (_lib.LdpcCode * max(len(ldpc), 1))()
    for q, (J, L, m, res) in zip(lcodes, ldpc):
        q.J, q.L, q.max_iter, q.reserved = J, L, m, res
    cells, NV, NL = PAIRS * N_CH * N_SNR, max(len(codes), 1), max(len(ldpc), 1)
    outs = dict(errs=np.full((1, cells, N, 2), POISON_U, np.uint64), pw=np.full((1, cells, N), POISON_F, np.float64),
                serrs=np.full((1, cells, syms - 1, 2), POISON_U, np.uint64), spw=np.full((1, cells, syms - 1), POISON_F, np.float64),
                ppw=np.full((1, cells, 2), POISON_F, np.float64), bpen=np.full((1, cells, 2, N), POISON_F, np.float64),
                spen=np.full((1, cells, 2, syms - 1), POISON_F, np.float64), ferrs=np.full((1, cells, NV, 2), POISON_U, np.uint64),
                lerrs=np.full((1, cells, NL, 4), POISON_U, np.uint64), sbits=np.full((cells, FRAMES, 1, syms - 1, N, 8), POISON_B, np.int8))
    a.update(outs)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_coset(
        C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], 2, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"], 1, cpts, 2, ptr["scales"],
        ptr["pilots"], None if "tracking" in null else ctps, C.c_float(llr_scale), ptr["perm"],
        len(codes) if n_codes is None else n_codes, None if "codes" in null else ccodes,
        len(ldpc) if n_ldpc is None else n_ldpc, None if "ldpc_codes" in null else lcodes, sym_rot,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"], ptr["ferrs"], ptr["lerrs"],
        ptr["sbits"] if soft_bits else None)
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_B if v.dtype == np.int8 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_coset\((.*?)\);", hdr, flags=re.M | re.S)
    frm = re.search(r"^int wofdm_rx_profile_coded_frame\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and frm

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, fargs = args_of(m.group(1)), args_of(frm.group(1))
    # every argument of the coded-frame call through perm; both families' counts and codes; sym_rot; the seven tracking outputs;
    # frame_errs, ldpc_errs, soft_bits
    assert fargs[22] == "const int32_t *perm" and fargs[25] == "int32_t sym_rot" and fargs[33] == "uint64_t *frame_errs"
    assert args == fargs[:25] + ["int32_t n_ldpc", "const wofdm_ldpc_code *ldpc_codes"] + fargs[25:34] + ["uint64_t *ldpc_errs", "int8_t *soft_bits"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_coset.argtypes
    assert len(at) == len(args) == 38 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.c_float if arg.startswith("float ") else
                     C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else
                     C.POINTER(_lib.TrackingPoint) if "wofdm_tracking_point" in arg else
                     C.POINTER(_lib.LdpcCode) if "wofdm_ldpc_code " in arg else
                     C.POINTER(_lib.Code) if "wofdm_code " in arg else C.c_void_p), arg
    link = open(os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "wofdm_link.h")).read()
    assert re.search(r"^#define WOFDM_STREAM_INFO 4u?\b", link, flags=re.M) and _lib.STREAM_INFO == 4
    philox = open(os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "philox.h")).read()
    assert "WOFDM_STREAM_INFO" not in philox                           # (a file of the frame kernels' source hash)
    for name in ("wofdm_rx_profile_coset", "wofdm_conv_encode", "wofdm_ldpc_encode", "wofdm_coset_info"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("RxProfileCoset", "STREAM_INFO", "coset_info", "conv_encode_gpu", "ldpc_encode_gpu", "rx_profile_coset_gpu",
                 "rx_profile_coset_host", "rx_profile_coset_chunk_frames", "frame_profile_coset", "coset_ber", "coset_fer",
                 "coset_codewords", "coset_for_window_file"):
        assert hasattr(W, name), name


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _err()
    assert _call(codes=[VIT, (1, (0, 0, 0)), (2, (0, 0, 0)), VIT], ldpc=[LDPC, (3, 6, 1, 0), (6, 24, 64, 0), (4, 16, 20, 0)]) == -3
    assert _call(perm=None) == -3 and _call(soft_bits=False) == -3
    assert _call(perm=R.default_interleaver(N_C), sym_rot=R.default_sym_rot(N_C, S - 1)) == -3
    assert _call(sym_rot=N_C - 1) == -3
    assert _call(tracking=(1, 1, (0, 0))) == -3
    assert _call(syms=2) == -3
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out
    # one family alone: its count 0, its codes and its counters NULL
    assert _call(codes=(), null=("codes", "ferrs")) == -3 and _call(ldpc=(), null=("ldpc_codes", "lerrs")) == -3
    assert _call(codes=()) == -3 and _call(ldpc=()) == -3              # (an array that is there beside a count of 0 is not read)
    # N = 1024 over 15 data symbols: T up to 46 080 steps, W = 4 words of 15 360, the largest code's LDS with the word's bits
    assert _call(N=1024, pilots=None, syms=16, soft_bits=False, frames=1, codes=[VIT, (2, (0, 0, 0))], ldpc=[LDPC, (6, 24, 5, 0)]) == -3
    assert _call(N=1024, pilots=None, syms=5, soft_bits=False, frames=1, ldpc=[(6, 24, 5, 0), (3, 4, 5, 0)]) == -3


def test_the_new_checks_fire_in_order():
    # 2. a negative count, 3. a count above the limit, 4. both counts 0
    assert _call(n_codes=-1) == -1 and "n_codes" in _err() and _call(n_ldpc=-1) == -1 and "n_ldpc" in _err()
    assert _call(codes=[VIT] * 4, n_codes=5) == -2 and _call(ldpc=[LDPC] * 4, n_ldpc=5) == -2 and "exceeds" in _err()
    assert _call(n_codes=-1, n_ldpc=5) == -1 and _call(n_codes=5, n_ldpc=-1) == -1     # (either negative before either too large)
    assert _call(codes=(), ldpc=()) == -1 and "n_codes + n_ldpc" in _err()
    assert _call(codes=(), ldpc=(), n_ldpc=5) == -2
    # 5. NULL code arrays where the count is > 0
    assert _call(null=("codes",)) == -1 and "NULL" in _err() and _call(null=("ldpc_codes",)) == -1 and "NULL" in _err()
    assert _call(codes=(), ldpc=(), null=("codes",)) == -1 and "n_codes + n_ldpc" in _err()
    # 6. sym_rot
    for bad in (-1, N_C, N_C + 5):
        assert _call(sym_rot=bad) == -1 and "sym_rot" in _err(), bad
    assert _call(pilots=None, sym_rot=N_C) == -3                       # (n_c is the data bins': 4 N without a comb)
    assert _call(null=("codes",), sym_rot=-1) == -1 and "NULL" in _err()
    # 7. NULL counters where the count is > 0
    assert _call(null=("ferrs",)) == -1 and "frame_errs" in _err() and _call(null=("lerrs",)) == -1 and "ldpc_errs" in _err()
    assert _call(null=("ferrs",), sym_rot=-1) == -1 and "sym_rot" in _err()
    # 8. the Viterbi codes one by one, as the coded-frame call checks them, before any LDPC code
    assert _call(codes=[VIT, (3, (0, 0, 0))]) == -1 and "codes[1].rate" in _err()
    assert _call(codes=[VIT, (-1, (0, 0, 0))]) == -1 and "codes[1].rate" in _err()
    assert _call(codes=[(1, (0, 1, 0))]) == -1 and "codes[0].reserved" in _err()
    assert _call(codes=[(0, (0, 0, 1)), (5, (0, 0, 0))]) == -1 and "codes[0].reserved" in _err()
    assert _call(codes=[(3, (0, 0, 0))], ldpc=[(2, 8, 30, 0)]) == -1 and "rate" in _err()
    assert _call(codes=[(3, (0, 0, 0))], null=("ferrs",)) == -1 and "frame_errs" in _err()
    # two data bins of 16-QAM over S - 1 = 3 symbols: n_f = 24, T = 12 / 16 / 18; with one bin n_f = 12: T = 6 at rate 1/2
    two, one = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    two[[5, 9, 20]], one[[5, 9]] = 1, 1
    assert _call(active=two, pilots=(5,), ldpc=()) == -3
    assert _call(active=one, pilots=(5,), ldpc=(), codes=[(2, (0, 0, 0)), VIT]) == -1 and "codes[1]" in _err() and "steps" in _err()
    assert _call(active=one, pilots=(5,), codes=[VIT], ldpc=[(2, 8, 30, 0)]) == -1 and "steps" in _err()
    # 9. the LDPC codes one by one, as wofdm_rx_profile_ldpc checks them
    for bad, what in (((2, 8, 30, 0), "J"), ((7, 12, 30, 0), "J"), ((4, 4, 30, 0), "L"), ((4, 25, 30, 0), "L"), ((4, 8, 0, 0), "max_iter"),
                      ((4, 8, 65, 0), "max_iter"), ((4, 8, 30, 1), "reserved")):
        assert _call(ldpc=[LDPC, bad]) == -1 and "ldpc_codes[1]." + what in _err(), bad
    assert _call(ldpc=[(4, 8, 30, 1), (2, 8, 30, 0)]) == -1 and "ldpc_codes[0].reserved" in _err()
    assert _call(codes=(), ldpc=[(2, 4, 0, 1)]) == -1 and "ldpc_codes[0].J" in _err()
    few = np.zeros(N, np.uint8)
    few[[5, 9, 20, 31, 47, 60]] = 1
    assert _call(active=few, pilots=(5,), ldpc=[(3, 6, 30, 0), LDPC]) == -3
    assert _call(active=few, pilots=(5,), ldpc=[LDPC, (6, 24, 30, 0)]) == -1 and "ldpc_codes[1]" in _err() and "information" in _err()
    assert _call(active=few, pilots=(5,), ldpc=[LDPC], tracking=(0, 1, (0, 0))) == -1 and "information" in _err()


def test_the_coded_frame_calls_checks_come_first():
    # 1. llr_scale, perm and the size of soft_bits, before the counts and the codes
    for bad in (0.0, -0.25, np.nan, np.inf):
        assert _call(llr_scale=bad, n_codes=-1) == -1 and "llr_scale" in _err(), bad
    for bad in (np.zeros(N_C), np.arange(N_C) + 1, np.r_[np.arange(N_C - 1), -1]):
        assert _call(perm=bad, n_codes=-1) == -1 and "perm" in _err()
    cells = PAIRS * N_CH * N_SNR
    frames = (1 << 30) // (cells * (S - 1) * N * 8) + 1
    assert _call(frames=frames, n_codes=-1) == -2 and "soft_bits" in _err()
    assert _call(frames=frames, soft_bits=False) == -3
    assert _call(llr_scale=np.nan, perm=np.zeros(N_C)) == -1 and "llr_scale" in _err()
    # and the tracking call's own before those
    assert _call(null=("tracking",), llr_scale=np.nan) == -1 and "NULL" in _err()
    assert _call(tracking=(2, 0, (0, 0)), llr_scale=np.nan) == -1 and "tracking[0]" in _err()
    assert _call(syms=2, tracking=(0, 1, (0, 0))) == -1 and "post" in _err()
    assert _call(pilots=range(N), null=("codes",)) == -1 and "data bin" in _err()
    for name in ("scales", "bpen", "w_tx", "errs"):
        assert _call(null=(name,)) == -1, name


def test_the_encoders_check_before_the_device():
    lib = _lib.load()
    info, out = np.zeros((2, 20000), np.uint8), np.full((2, 40000), 7, np.uint8)

    def conv(rate=0, n_c=64, n_cw=1, i=info, o=out, device=99):
        rc = lib.wofdm_conv_encode(device, rate, n_c, n_cw, None if i is None else i.ctypes.data, None if o is None else o.ctypes.data)
        assert (out == 7).all()
        return rc
    assert conv() == -3 and "device" in _err() and conv(rate=2, n_c=37632, n_cw=2) == -3
    assert conv(i=None) == -1 and conv(o=None) == -1 and "NULL" in _err()
    assert conv(rate=-1) == -1 and conv(rate=3) == -1 and "rate" in _err()
    assert conv(n_c=0) == -1 and conv(n_cw=0) == -1
    assert conv(n_c=13) == -1 and "steps" in _err() and conv(n_c=14) == -3             # (T = 6 and 7 at rate 1/2)
    assert conv(rate=2, n_c=9) == -1 and conv(rate=2, n_c=10) == -3
    assert conv(n_c=2 * _lib.CODE_LONG_MAX_STEPS + 2) == -2 and conv(i=None, rate=3) == -1 and "NULL" in _err()
    assert conv(rate=3, n_c=0) == -1 and "rate" in _err()

    def ldpc(J=4, L=8, n=488, n_cw=1, i=info, o=out, device=99):
        rc = lib.wofdm_ldpc_encode(device, J, L, n, n_cw, None if i is None else i.ctypes.data, None if o is None else o.ctypes.data)
        assert (out == 7).all()
        return rc
    assert ldpc() == -3 and "device" in _err() and ldpc(n_cw=2, n=16384) == -3 and ldpc(J=6, L=24, n=16384) == -3
    assert ldpc(i=None) == -1 and ldpc(o=None) == -1 and "NULL" in _err()
    for J, L in ((2, 8), (7, 12), (4, 4), (4, 25)):
        assert ldpc(J=J, L=L) == -1, (J, L)
    assert ldpc(n=0) == -1 and ldpc(n_cw=0) == -1
    assert ldpc(n=16385) == -2 and "16384" in _err()
    assert ldpc(J=6, L=24, n=60) == -1 and "information" in _err() and ldpc(J=3, L=4, n=16) == -3
    # the order: NULL, the code's ranges, the counts, the length, K
    assert ldpc(i=None, J=2) == -1 and "NULL" in _err()
    assert ldpc(J=2, n=0) == -1 and "J=" in _err()
    assert ldpc(n=0, n_cw=0) == -1 and ldpc(J=6, L=24, n=16385) == -2
