"""wofdm_rx_profile_harq and wofdm_ldpc_harq_decode without a GPU: their place in the public header and the binding, and the
argument checks -- the conditions of include/wofdm.h in their documented order, each answered before the device is touched (a
call that passes the checks ends in WOFDM_E_HIP: device 99 does not exist), and a failed call leaves its outputs as they were.
The pattern, the shapes and the points are tests/test_rx_profile_coset_abi.py's."""
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
FRAMES = 4
LDPC = (4, 8, 30, 0)


def _call(ldpc=(LDPC,), llr_scale=0.25, perm="identity", sym_rot=0, rounds=2, combine=1, pilots=COMB, active=None, null=(), n_ldpc=None,
          soft_bits=True, tracking=None, frames=FRAMES, frame_offset=0, device=99, syms=S, N=N):
    """rc of one call on small arrays (the tracking test's, one all-off point) with the LDPC codes (J, L, max_iter, reserved)"""
    st = V.make_structure("CPW", N, 32)
    cfg = W.make_cfg(st, 4, syms, TAPS, N_CH, N_SNR, PAIRS, seed=3, frames_per_cell=frames, frame_offset=frame_offset)
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
    lcodes = (_lib.LdpcCode * max(len(ldpc), 1))()
    for q, (J, L, m, res) in zip(lcodes, ldpc):
        q.J, q.L, q.max_iter, q.reserved = J, L, m, res
    cells, NL = PAIRS * N_CH * N_SNR, max(len(ldpc), 1)
    outs = dict(errs=np.full((1, cells, N, 2), POISON_U, np.uint64), pw=np.full((1, cells, N), POISON_F, np.float64),
                serrs=np.full((1, cells, syms - 1, 2), POISON_U, np.uint64), spw=np.full((1, cells, syms - 1), POISON_F, np.float64),
                ppw=np.full((1, cells, 2), POISON_F, np.float64), bpen=np.full((1, cells, 2, N), POISON_F, np.float64),
                spen=np.full((1, cells, 2, syms - 1), POISON_F, np.float64),
                herrs=np.full((1, cells, NL, _lib.HARQ_FIELDS), POISON_U, np.uint64),
                sbits=np.full((cells, FRAMES, 1, syms - 1, N, 8), POISON_B, np.int8))
    a.update(outs)
    ptr = {n: (None if v is None or n in null else v.ctypes.data) for n, v in a.items()}
    rc = _lib.load().wofdm_rx_profile_harq(
        C.byref(cfg), device, ptr["w_tx"], ptr["w_rx"], ptr["h"], ptr["snr"], ptr["active"], ptr["mask"],
        ptr["h_track"], 2, n_knots, knot_step, ptr["aci_active"], ptr["aci_h"], ptr["ref_power"], 1, cpts, 2, ptr["scales"],
        ptr["pilots"], None if "tracking" in null else ctps, C.c_float(llr_scale), ptr["perm"],
        len(ldpc) if n_ldpc is None else n_ldpc, None if "ldpc_codes" in null else lcodes, sym_rot, rounds, combine,
        ptr["errs"], ptr["pw"], ptr["serrs"], ptr["spw"], ptr["ppw"], ptr["bpen"], ptr["spen"], ptr["herrs"],
        ptr["sbits"] if soft_bits else None)
    for n, v in outs.items():                                          # no failed call writes its outputs
        assert (v == (POISON_U if v.dtype == np.uint64 else POISON_B if v.dtype == np.int8 else POISON_F)).all(), n
    return rc


def _err():
    return _lib.load().wofdm_last_error().decode()


def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wofdm.h")).read()
    m = re.search(r"^int wofdm_rx_profile_harq\((.*?)\);", hdr, flags=re.M | re.S)
    cos = re.search(r"^int wofdm_rx_profile_coset\((.*?)\);", hdr, flags=re.M | re.S)
    assert m and cos

    def args_of(text):
        return [a.strip() for a in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    args, cargs = args_of(m.group(1)), args_of(cos.group(1))
    # every argument of the coset call through perm; n_ldpc, ldpc_codes, sym_rot; rounds, combine; the seven tracking outputs;
    # harq_errs, soft_bits
    assert cargs[22] == "const int32_t *perm" and cargs[25] == "int32_t n_ldpc" and cargs[27] == "int32_t sym_rot"
    assert args == cargs[:23] + cargs[25:28] + ["int32_t rounds", "int32_t combine"] + cargs[28:35] + ["uint64_t *harq_errs", "int8_t *soft_bits"]
    lib = _lib.load()
    at = lib.wofdm_rx_profile_harq.argtypes
    assert len(at) == len(args) == 37 and at[0] == C.POINTER(_lib.Cfg) and at[1] == C.c_int
    for t, arg in zip(at[2:], args[2:]):
        assert t == (C.c_int32 if arg.startswith("int32_t") else C.c_float if arg.startswith("float ") else
                     C.POINTER(_lib.LinkPoint) if "wofdm_link_point" in arg else
                     C.POINTER(_lib.TrackingPoint) if "wofdm_tracking_point" in arg else
                     C.POINTER(_lib.LdpcCode) if "wofdm_ldpc_code " in arg else C.c_void_p), arg
    d = re.search(r"^int wofdm_ldpc_harq_decode\((.*?)\);", hdr, flags=re.M | re.S)
    dargs = args_of(d.group(1))
    assert dargs == ["int device", "int32_t J", "int32_t L", "int32_t max_iter", "int32_t n", "const int32_t *perm", "int32_t n_cw",
                     "int32_t rounds", "int32_t combine", "const int8_t *soft", "uint8_t *bits", "int32_t *round", "int32_t *iters",
                     "uint8_t *converged"]
    assert len(lib.wofdm_ldpc_harq_decode.argtypes) == 14
    assert re.search(r"^#define WOFDM_HARQ_MAX_ROUNDS 8\b", hdr, flags=re.M) and _lib.HARQ_MAX_ROUNDS == 8
    assert re.search(r"^#define WOFDM_HARQ_FIELDS 13\b", hdr, flags=re.M) and _lib.HARQ_FIELDS == 13
    link = open(os.path.join(ROOT, "w-ofdm-optimization_amd", "csrc", "wofdm_link.h")).read()
    assert re.search(r"^#define WOFDM_HARQ_ROUNDS 8\b", link, flags=re.M) and re.search(r"^#define WOFDM_HARQ_NF 13\b", link, flags=re.M)
    for name in ("wofdm_rx_profile_harq", "wofdm_ldpc_harq_decode"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("RxProfileHarq", "ldpc_harq_decode", "ldpc_harq_decode_gpu", "rx_profile_harq_gpu", "rx_profile_harq_host",
                 "rx_profile_harq_chunk_frames", "harq_acked", "harq_mean_transmissions", "harq_residual_fer", "harq_undetected",
                 "harq_goodput", "harq_bits_per_sample", "harq_for_window_file"):
        assert hasattr(W, name), name


def test_a_valid_call_reaches_the_device_and_no_further():
    assert _call() == -3 and "device" in _err()
    assert _call(ldpc=[LDPC, (3, 6, 1, 0), (6, 24, 64, 0), (4, 16, 20, 0)]) == -3
    assert _call(perm=None) == -3 and _call(soft_bits=False) == -3
    assert _call(perm=R.default_interleaver(N_C), sym_rot=R.default_sym_rot(N_C, S - 1)) == -3 and _call(sym_rot=N_C - 1) == -3
    assert _call(tracking=(1, 1, (0, 0))) == -3 and _call(syms=2) == -3
    for out in ("pw", "serrs", "spw", "ppw", "spen"):
        assert _call(null=(out,)) == -3, out
    for rounds in (1, 2, 4):
        for combine in (0, 1):
            assert _call(rounds=rounds, combine=combine) == -3, (rounds, combine)
    assert _call(rounds=3, frames=3) == -3 and _call(rounds=8, frames=8, soft_bits=False) == -3
    assert _call(rounds=4, frame_offset=2 ** 32 + 4) == -3 and _call(rounds=3, frames=3, frame_offset=2 ** 32 - 1) == -3
    # N = 1024 over 15 data symbols: W = 4 words of 15 360, the largest code's LDS with the word's bits
    assert _call(N=1024, pilots=None, syms=16, soft_bits=False, frames=2, ldpc=[LDPC, (6, 24, 5, 0)]) == -3


def test_the_new_checks_fire_in_order():
    # 2. a negative count, 3. a count above the limit, 4. a count of 0, 5. NULL codes
    assert _call(n_ldpc=-1) == -1 and "n_ldpc" in _err()
    assert _call(ldpc=[LDPC] * 4, n_ldpc=5) == -2 and "exceeds" in _err()
    assert _call(ldpc=()) == -1 and "n_ldpc" in _err() and _call(ldpc=(), null=("ldpc_codes",)) == -1 and "n_ldpc" in _err()
    assert _call(null=("ldpc_codes",)) == -1 and "NULL" in _err()
    # 6. sym_rot
    for bad in (-1, N_C, N_C + 5):
        assert _call(sym_rot=bad) == -1 and "sym_rot" in _err(), bad
    assert _call(pilots=None, sym_rot=N_C) == -3                       # (n_c is the data bins': 4 N without a comb)
    assert _call(null=("ldpc_codes",), sym_rot=-1) == -1 and "NULL" in _err()
    # 7. NULL harq_errs
    assert _call(null=("herrs",)) == -1 and "harq_errs" in _err()
    assert _call(null=("herrs",), sym_rot=-1) == -1 and "sym_rot" in _err()
    # 8. rounds, 9. combine
    for bad in (0, -1, 9, 64):
        assert _call(rounds=bad) == -1 and "rounds" in _err(), bad
    assert _call(rounds=0, null=("herrs",)) == -1 and "harq_errs" in _err()
    for bad in (-1, 2, 7):
        assert _call(combine=bad) == -1 and "combine" in _err(), bad
    assert _call(rounds=9, combine=2) == -1 and "rounds" in _err()
    # 10. frames_per_cell, 11. frame_offset: whole groups on the global frame index
    assert _call(rounds=3) == -1 and "frames_per_cell" in _err()
    assert _call(rounds=2, frames=3) == -1 and "frames_per_cell" in _err()
    assert _call(rounds=2, frame_offset=1) == -1 and "frame_offset" in _err()
    assert _call(rounds=4, frame_offset=2 ** 32 + 2) == -1 and "frame_offset" in _err()
    assert _call(rounds=2, frames=3, frame_offset=1) == -1 and "frames_per_cell" in _err()
    assert _call(rounds=2, frames=3, combine=2) == -1 and "combine" in _err()
    # 12. the LDPC codes one by one, as the coset call checks them, behind the groups
    for bad, what in (((2, 8, 30, 0), "J"), ((7, 12, 30, 0), "J"), ((4, 4, 30, 0), "L"), ((4, 25, 30, 0), "L"), ((4, 8, 0, 0), "max_iter"),
                      ((4, 8, 65, 0), "max_iter"), ((4, 8, 30, 1), "reserved")):
        assert _call(ldpc=[LDPC, bad]) == -1 and "ldpc_codes[1]." + what in _err(), bad
    assert _call(ldpc=[(2, 8, 30, 0)], frame_offset=1) == -1 and "frame_offset" in _err()
    few = np.zeros(N, np.uint8)
    few[[5, 9, 20, 31, 47, 60]] = 1
    assert _call(active=few, pilots=(5,), ldpc=[(3, 6, 30, 0), LDPC]) == -3
    assert _call(active=few, pilots=(5,), ldpc=[LDPC, (6, 24, 30, 0)]) == -1 and "ldpc_codes[1]" in _err() and "information" in _err()


def test_the_coded_frame_calls_checks_come_first():
    for bad in (0.0, -0.25, np.nan, np.inf):
        assert _call(llr_scale=bad, n_ldpc=-1) == -1 and "llr_scale" in _err(), bad
    for bad in (np.zeros(N_C), np.arange(N_C) + 1, np.r_[np.arange(N_C - 1), -1]):
        assert _call(perm=bad, rounds=0) == -1 and "perm" in _err()
    cells = PAIRS * N_CH * N_SNR
    frames = ((1 << 30) // (cells * (S - 1) * N * 8) + 2) // 2 * 2
    assert _call(frames=frames, n_ldpc=-1) == -2 and "soft_bits" in _err()
    assert _call(frames=frames, soft_bits=False) == -3
    assert _call(null=("tracking",), llr_scale=np.nan) == -1 and "NULL" in _err()
    assert _call(tracking=(2, 0, (0, 0)), rounds=0) == -1 and "tracking[0]" in _err()
    assert _call(pilots=range(N), null=("ldpc_codes",)) == -1 and "data bin" in _err()
    for name in ("scales", "bpen", "w_tx", "errs"):
        assert _call(null=(name,)) == -1, name


def test_the_decoder_checks_before_the_device():
    lib = _lib.load()
    soft = np.zeros((2, 8, 16384), np.int8)
    outs = dict(bits=np.full((2, 16384), 7, np.uint8), rnd=np.full(2, 7, np.int32), iters=np.full(2, 7, np.int32),
                conv=np.full(2, 7, np.uint8))

    def dec(J=4, L=8, max_iter=30, n=488, perm=None, n_cw=1, rounds=2, combine=1, null=(), device=99):
        p = None if perm is None else np.asarray(perm, np.int32)
        rc = lib.wofdm_ldpc_harq_decode(device, J, L, max_iter, n, None if p is None else p.ctypes.data, n_cw, rounds, combine,
                                        None if "soft" in null else soft.ctypes.data,
                                        *(None if k in null else v.ctypes.data for k, v in outs.items()))
        assert all((v == 7).all() for v in outs.values())
        return rc
    assert dec() == -3 and "device" in _err() and dec(n_cw=2, n=16384, rounds=8) == -3 and dec(J=6, L=24, n=16384) == -3
    assert dec(rounds=1, combine=0) == -3 and dec(perm=np.arange(488)[::-1]) == -3 and dec(null=("rnd", "iters", "conv")) == -3
    assert dec(null=("soft",)) == -1 and dec(null=("bits",)) == -1 and "NULL" in _err()
    for Jc, Lc in ((2, 8), (7, 12), (4, 4), (4, 25)):
        assert dec(J=Jc, L=Lc) == -1, (Jc, Lc)
    assert dec(max_iter=0) == -1 and dec(max_iter=65) == -1 and "max_iter" in _err()
    assert dec(rounds=0) == -1 and dec(rounds=9) == -1 and "rounds" in _err()
    assert dec(combine=2) == -1 and dec(combine=-1) == -1 and "combine" in _err()
    assert dec(n=0) == -1 and dec(n_cw=0) == -1
    assert dec(n=16385) == -2 and "16384" in _err()
    assert dec(J=6, L=24, n=60) == -1 and "information" in _err() and dec(J=3, L=4, n=16) == -3
    assert dec(perm=np.zeros(488)) == -1 and "perm" in _err()
    # the order: NULL, the code's ranges, max_iter, rounds, combine, the counts, the length, K, perm
    assert dec(null=("soft",), J=2) == -1 and "NULL" in _err()
    assert dec(J=2, max_iter=0) == -1 and "J=" in _err()
    assert dec(max_iter=0, rounds=0) == -1 and "max_iter" in _err()
    assert dec(rounds=0, combine=2) == -1 and "rounds" in _err()
    assert dec(combine=2, n=0) == -1 and "combine" in _err()
    assert dec(n=0, perm=np.zeros(488)) == -1 and "n=" in _err()
    assert dec(n=16385, perm=np.zeros(488)) == -2
