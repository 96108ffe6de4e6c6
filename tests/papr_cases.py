"""Cases and oracle references of the Tx-PAPR tests (tests/test_tx_papr_host.py, tests/test_gpu_tx_papr.py).

The reference is always the CPU oracle: ``oracle.frame`` on ``oracle.gen_labels`` of (seed, cell = pair, frame), its
``tx`` dump cut into symbol periods.  References are computed once per case and shared (``reference`` is cached); the
arrays they return are not to be modified.

Histogram checks allow a difference only for periods whose fp64 PAPR lies within ``NEAR_DB`` of a bin edge, and need
those to be at most 1 % of the periods; ``reference`` therefore takes the first seed, counting up from the case's base
seed, for which the oracle alone meets that condition -- a property of the oracle's numbers, decided on the CPU.
"""
import functools

import numpy as np

import wofdm_amd as W
from oracle import oracle as O
from wofdm_amd import channel_mask as CM
from wofdm_amd import timefreq as T
from wofdm_amd import variants as V

NS = (64, 128, 256, 512, 1024)
SYSTEMS = ("wtx", "CPW", "wrx")
VARIANTS = ("plain", "half", "masked", "half_masked")
LO_DB, STEP_DB, N_BINS = 4.0, 0.25, 40          # 4 ... 14 dB
NEAR_DB = 2e-4
FRAMES, PAIRS = 8, 2


def shape_of(n_fft, system, variant="plain"):
    """(cp, S, k): cp = N / 8 (CPW: 32 at every N -- an odd stride at N = 256), S and k rotated over the cases.  The
    oracle applies the mask as a direct-form DFT pair, 34 ms per symbol at N = 1024 on one core: the masked cases there
    run S = 2 where the rotation gives 16 (S = 16 at N = 1024 runs unmasked here, masked at N = 512)."""
    i = NS.index(n_fft) + SYSTEMS.index(system)
    S = (2, 9, 16)[i % 3]
    if n_fft == 1024 and variant.endswith("masked") and S == 16:
        S = 2
    return (32 if system == "CPW" else n_fft // 8), S, (2, 4, 6)[(i // 3 + SYSTEMS.index(system)) % 3]


def structure(n_fft, system):
    return V.make_structure(system, n_fft, shape_of(n_fft, system)[0])


def random_windows(st, pairs, seed):
    """[pairs, P] Tx windows: a random level and a random monotone tail per pair (all ones without a Tx tail, scaled)"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(pairs):
        level = 1.0 + 0.05 * rs.randn()
        if st.tail_tx:
            out.append(V.expand_tx_window(st, np.concatenate(([level], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1]))))
        else:
            out.append(np.full(st.sym_len, level))
    return np.stack(out).astype(np.float32)


def allocation(n_fft, variant):
    return CM.half_band_allocation(n_fft) if variant.startswith("half") else None


def mask_of(st, variant):
    return CM.tx_mask(st.sym_len).astype(np.float32) if variant.endswith("masked") else None


def oracle_frame_tx(st, k, S, w_tx, active, mask, seed, cell, frame):
    """(labels [S, N], tx [beta + S B]) of one frame from the oracle"""
    osys = O.make_sys(st.n_fft, k, S, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm, st.circ_shift, 1, 1,
                      active=active, tx_mask=None if mask is None else np.asarray(mask, np.float64))
    lab = O.gen_labels(osys, seed, cell, frame)
    _, d = O.frame(osys, np.asarray(w_tx, np.float64), W.rx_rc_window(st), np.ones(1, complex), 30.0, lab,
                   O.gen_noise(osys, seed, cell, frame), dump=True)
    return lab, d["tx"]


def periods_of(tx, S, B):
    """[S, 2] = {peak, energy} of the symbol periods of one frame"""
    p = np.abs(np.asarray(tx)[:S * B].reshape(S, B)) ** 2
    return np.stack([p.max(axis=1), p.sum(axis=1)], axis=1)


def oracle_periods(st, k, S, w_pairs, active, mask, seed, frame_offset, frames, pairs=None):
    """[pairs, frames, S, 2] from the oracle; pair p is cell p"""
    B = st.sym_len - st.tail_tx
    pairs = range(len(w_pairs)) if pairs is None else pairs
    out = np.empty((len(pairs), frames, S, 2))
    for i, p in enumerate(pairs):
        for f in range(frames):
            out[i, f] = periods_of(oracle_frame_tx(st, k, S, w_pairs[p], active, mask, seed, p, frame_offset + f)[1], S, B)
    return out


def near_edges(periods, B, lo_db=LO_DB, step_db=STEP_DB):
    """number of periods whose fp64 PAPR lies within NEAR_DB of a bin edge"""
    t = (T.papr_db(periods, B).reshape(-1) - lo_db) / step_db
    return int((np.abs(t - np.round(t)) * step_db <= NEAR_DB).sum())


def pick_seed(make_periods, B, base_seed, tries=16):
    """first seed from base_seed on whose oracle periods have at most 1 % within NEAR_DB of a bin edge"""
    for seed in range(base_seed, base_seed + tries):
        per = make_periods(seed)
        near = near_edges(per, B)
        if near <= 0.01 * (per.size // 2):
            return seed, per, near
    raise AssertionError("no seed in [%d, %d) keeps the oracle's periods clear of the bin edges" % (base_seed, base_seed + tries))


@functools.lru_cache(maxsize=None)
def reference(n_fft, system, variant):
    """dict of the case: st, k, S, w [PAIRS, P] float32, active, mask, seed, periods [PAIRS, FRAMES, S, 2], near"""
    cp, S, k = shape_of(n_fft, system, variant)
    st = structure(n_fft, system)
    w = random_windows(st, PAIRS, 1000 + n_fft + SYSTEMS.index(system))
    active, mask = allocation(n_fft, variant), mask_of(st, variant)
    base = 10 * (n_fft + 7 * SYSTEMS.index(system) + VARIANTS.index(variant))
    seed, per, near = pick_seed(lambda sd: oracle_periods(st, k, S, w, active, mask, sd, 0, FRAMES),
                                st.sym_len - st.tail_tx, base)
    return dict(st=st, k=k, S=S, w=w, active=active, mask=mask, seed=seed, periods=per, near=near)


def check_hist(hist_gpu, ref_periods, B, near, lo_db=LO_DB, step_db=STEP_DB, n_bins=N_BINS):
    """hist_gpu [pairs, n_bins] against papr_hist of the oracle's periods [pairs, frames, S, 2]: every row sums to
    exactly frames * S, and the rows together differ by at most 2 near counts.  Returns the difference."""
    hist_gpu = np.atleast_2d(hist_gpu)
    assert hist_gpu.shape == (ref_periods.shape[0], n_bins)
    diff = 0
    for row, per in zip(hist_gpu, ref_periods):
        want = T.papr_hist(per, B, lo_db, step_db, n_bins)
        assert int(row.sum()) == per.size // 2, (int(row.sum()), per.size // 2)
        diff += int(np.abs(row.astype(np.int64) - want.astype(np.int64)).sum())
    assert diff <= 2 * near, (diff, near)
    return diff
