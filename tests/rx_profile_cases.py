"""Cases and oracle references of the receive-profile tests (tests/test_rx_profile_host.py, tests/test_gpu_rx_profile.py).

The reference is always the CPU oracle: ``oracle.frame`` on ``oracle.gen_labels`` / ``oracle.gen_noise`` of (seed, cell,
frame) with ``dump=True``; its ``labels_rx`` and ``Xhat`` are reduced per bin.  References are computed once per case and
shared (``reference`` is cached); the arrays they return are not to be modified.

GPU and oracle may differ only on "near" decisions: a component of the oracle's fp64 Xhat lies within
``NEAR_TOL * max(1, |Xhat|) * max_n |Y0| / |Y0[n]|`` of a slicer threshold (1e-4 = five times the project's 2e-5 stage
tolerance; the weight is the gain the equaliser puts on an absolute error of Y on a faded bin).  They have to be at most
1 % of a case's decisions; ``reference`` takes the first seed, counting up from the case's base seed, for which the oracle
alone meets that -- decided on the CPU, as ``papr_cases.pick_seed`` does for the PAPR histograms.
"""
import concurrent.futures
import functools
import os

import numpy as np

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import rx_profile as R
from wofdm_amd import variants as V

import papr_cases as PC

NS, SYSTEMS, VARIANTS = PC.NS, PC.SYSTEMS, PC.VARIANTS
NEAR_TOL = 1e-4
PAIRS, N_SNR, N_CH, FRAMES = 2, 2, 2, 8
#: two SNR points per k at which the oracle counts bit and symbol errors in every case (checked in the host test).  64-QAM
#: runs at the low pair as well: on the full band the Tx mask leaves half of the bins to the noise, and the share of near
#: decisions there grows with the SNR (|Y0[n]| falls against max |Y0|) -- 1.5 % at 14 dB and 3 % at 22 dB whatever the seed,
#: against the 1 % the seed condition asks for; at 0 and 8 dB it is 0.7 ... 1.0 %.
SNR_DB = {2: (0.0, 8.0), 4: (8.0, 16.0), 6: (0.0, 8.0)}
#: err_power: |gpu - ref| <= POW_TOL * (ref[n] + mean_n ref) against the oracle's fp64 sums.  Measured on an MI355X
#: (profiles/rx_profile.txt): at most 2.93e-4 (N = 1024 wtx masked).  Ten times that, 3e-3, is more than the 1e-3 an fp32
#: chain may take, so the cause was looked for: it is the conditioning of Xhat = Y X0 / Y0 on faded bins, no stage -- storing
#: the waveform x in single precision and doing everything else in fp64 gives 6.1e-5 on the same case (host mirror), the
#: relative error of |Xhat - X|^2 being 2 |dY| / |Y0[n]|, i.e. the stage error times max |Y0| / |Y0[n]| (the weight of the
#: near rule), which reaches several hundred among the 65536 pilots of a case.  The tolerance stays at the 1e-3.
POW_TOL = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def shape_of(n_fft, system, variant="plain"):
    """(cp, S, k): the rotation of ``papr_cases.shape_of``; every masked case at N = 1024 runs S = 2 (the oracle applies
    the mask as a direct-form DFT pair, 34 ms per symbol there)."""
    cp, S, k = PC.shape_of(n_fft, system, variant)
    if n_fft == 1024 and variant.endswith("masked"):
        S = 2
    return cp, S, k


def channels():
    return np.load(os.path.join(GOLDEN, "channels_vehA.npz"), allow_pickle=False)["h"][:N_CH].astype(np.complex64)


def random_rx_windows(st, pairs, seed):
    """[pairs, N + delta] Rx windows: a random level and a random monotone tail per pair"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(pairs):
        level = 1.0 + 0.05 * rs.randn()
        tail = np.sort(rs.uniform(0.02, 0.48, st.tail_rx // 2))[::-1] * level
        out.append(V.expand_rx_window(st, np.concatenate(([level], tail))))
    return np.stack(out).astype(np.float32)


def make_case(st, k, S, variant, wseed, nbt=1):
    return dict(st=st, k=k, S=S, nbt=nbt, w_tx=PC.random_windows(st, PAIRS, wseed), w_rx=random_rx_windows(st, PAIRS, wseed + 1),
                h=channels(), snr=np.array(SNR_DB[k], np.float32), active=PC.allocation(st.n_fft, variant),
                mask=PC.mask_of(st, variant))


def oracle_sys(c):
    st = c["st"]
    return O.make_sys(st.n_fft, c["k"], c["S"], st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift,
                      c["h"].shape[1], c["nbt"], active=c["active"],
                      tx_mask=None if c["mask"] is None else np.asarray(c["mask"], np.float64))


def oracle_frame(c, seed, cell, frame, osys=None):
    """(bit [N], sym [N], pow [N], near, counts [4]) of one frame of `cell` from the oracle"""
    osys = oracle_sys(c) if osys is None else osys
    st, k = c["st"], c["k"]
    p, s, ch = cell // (N_SNR * N_CH), (cell // N_CH) % N_SNR, cell % N_CH
    lab = O.gen_labels(osys, seed, cell, frame)
    counts, d = O.frame(osys, c["w_tx"][p].astype(np.float64), c["w_rx"][p].astype(np.float64),
                        c["h"][ch].astype(np.complex128), float(c["snr"][s]), lab, O.gen_noise(osys, seed, cell, frame),
                        dump=True)
    on = np.ones(st.n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    diff = np.where(on[None, :], lab[1:] ^ d["labels_rx"], 0).astype(np.int64)
    bits = sum((diff >> b) & 1 for b in range(k)).sum(axis=0)
    pw = np.where(on[None, :], np.abs(d["Xhat"] - d["X"][1:]) ** 2, 0.0).sum(axis=0)
    near = int(R.near_decisions(k, np.where(on[None, :], d["Xhat"], 0.0), np.where(on, d["Y"][0], 0.0), NEAR_TOL).sum())
    assert int(bits.sum()) == int(counts[0]) and int((diff != 0).sum()) == int(counts[2])
    return bits, (diff != 0).sum(axis=0), pw, near, counts


def oracle_profile(c, seed, frame_offset, frames):
    """dict: bit, sym (int64), pow (float64) [PAIRS, N_SNR, N_CH, N]; near [PAIRS, N_SNR, N_CH]; counts [..., 4];
    decisions (per case).  The frames run on a few threads (the oracle keeps its workspace per thread)."""
    n = c["st"].n_fft
    cells = PAIRS * N_SNR * N_CH
    bit = np.zeros((cells, n), np.int64)
    sym = np.zeros((cells, n), np.int64)
    pw = np.zeros((cells, n), np.float64)
    near = np.zeros(cells, np.int64)
    counts = np.zeros((cells, 4), np.uint64)
    osys = oracle_sys(c)
    jobs = [(cell, frame_offset + f) for cell in range(cells) for f in range(frames)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda j: oracle_frame(c, seed, j[0], j[1], osys), jobs))
    for (cell, _), (b, s, e, nr, cnt) in zip(jobs, res):          # (in job order: the fp64 sums are reproducible)
        bit[cell] += b
        sym[cell] += s
        pw[cell] += e
        near[cell] += nr
        counts[cell] += cnt
    shp = (PAIRS, N_SNR, N_CH)
    n_on = n if c["active"] is None else int(np.count_nonzero(c["active"]))
    return dict(bit=bit.reshape(shp + (n,)), sym=sym.reshape(shp + (n,)), pow=pw.reshape(shp + (n,)), near=near.reshape(shp),
                counts=counts.reshape(shp + (4,)), decisions=cells * frames * (c["S"] - 1) * n_on)


def pick_seed(c, base_seed, frame_offset=0, frames=FRAMES, tries=32):
    """first seed from base_seed on whose oracle profile has at most 1 % near decisions"""
    for seed in range(base_seed, base_seed + tries):
        ref = oracle_profile(c, seed, frame_offset, frames)
        if ref["near"].sum() <= 0.01 * ref["decisions"]:
            return seed, ref
    raise AssertionError("no seed in [%d, %d) keeps the oracle's decisions clear of the thresholds" % (base_seed, base_seed + tries))


@functools.lru_cache(maxsize=None)
def reference(n_fft, system, variant, nbt=1, cp=None):
    """(case, seed, oracle profile of the frames [0, FRAMES)) of a case of the matrix; cp: another CP than the matrix's"""
    cp0, S, k = shape_of(n_fft, system, variant)
    cp = cp0 if cp is None else cp
    c = make_case(V.make_structure(system, n_fft, cp), k, S, variant, 2000 + n_fft + SYSTEMS.index(system), nbt)
    seed, ref = pick_seed(c, 10 * (n_fft + 7 * SYSTEMS.index(system) + VARIANTS.index(variant)))
    return c, seed, ref


@functools.lru_cache(maxsize=None)
def reference_over_the_frame_limit():
    """N = 1024, S = 16, cp + cs = 64: the frame's LDS image exceeds 160 KiB, wofdm_plan_create refuses it"""
    c = make_case(V.make_structure("wtx", 1024, 56), 4, 16, "plain", 3001)
    assert c["st"].cp + c["st"].cs == 64
    seed, ref = pick_seed(c, 7000)
    return c, seed, ref


def run_gpu(c, seed, frame_offset, frames, **kw):
    return W.rx_profile_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                            active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], **kw)


def pow_ratio(got, ref):
    """largest |got - ref| / (ref[n] + mean_n ref) over the cells and loaded bins"""
    ref = np.asarray(ref, np.float64)
    den = ref + ref.mean(axis=-1, keepdims=True)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.where(den > 0, den, 1.0)).max())


def check_profile(prof, ref, c, tag=""):
    """the rules of the module docstring, per cell; prints the figures before it asserts; returns the err_power ratio"""
    k = c["k"]
    on = np.ones(c["st"].n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    ds = np.abs(prof.sym_err.astype(np.int64) - ref["sym"]).sum(axis=-1)
    db = np.abs(prof.bit_err.astype(np.int64) - ref["bit"]).sum(axis=-1)
    ratio = pow_ratio(prof.err_power, ref["pow"])
    print("%s: sym diff %d, bit diff %d, near %d of %d decisions, err_power ratio %.2e"
          % (tag, ds.sum(), db.sum(), ref["near"].sum(), ref["decisions"], ratio))
    assert (ds <= ref["near"]).all(), (tag, ds, ref["near"])
    assert (db <= k * ref["near"]).all(), (tag, db, ref["near"])
    for a in (prof.bit_err, prof.sym_err, prof.err_power):
        assert (a[..., ~on] == 0).all(), tag
    assert ratio <= POW_TOL, (tag, ratio)
    return ratio
