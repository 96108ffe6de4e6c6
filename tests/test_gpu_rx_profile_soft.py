"""``wofdm_rx_profile_soft`` on the GPU (the link call's kernels with wofdm_rxprof_soft_kernel<N> in the link kernel's place, and
wofdm_rxprof_soft_reduce_kernel<N>), on the seven shapes, the composed points and the seeds of tests/test_gpu_rx_profile_link.py
(2 pairs x 2 SNR points x 2 channels x 8 frames; the seed of a case is that test's ``pick_seed``'s).

1. The five link fields are the bytes of ``rx_profile_link_gpu`` with the same arguments; the all-off point's per-bin fields are
   those of ``rx_profile_gpu``.
2. ``bit_penalty`` and ``bit_penalty_sym`` against the fp64 host route ``rx_profile_soft_host`` (tied to the CPU oracle's dump in
   tests/test_rx_profile_soft_host.py) under ``RC.pow_ratio`` <= ``RC.POW_TOL`` = 1e-3, per point, cell and scale -- err_power's
   bound and its derivation (tests/rx_profile_cases.py): a penalty is at most linear in Lambda, and Lambda has the conditioning 2
   |dY| / |Y_0[n]| of |Xhat - X|^2.  Unloaded bins are exactly 0.  The default sixteen scales.
3. Per cell, point and scale the symbols' totals and the bins' totals agree to 1e-4 relative: sums of the same positive fp32
   terms in two orders, at most 1024 terms times 2^-24 = 6e-5.
4. A call with scales (a, b, c) returns for b the bytes of a call with (b) alone; a sweep of points returns the bytes of its
   points one per call.
5. Repeated calls give identical bytes; a frame range split in two and accumulated through ``out`` gives the same integer
   counters and penalties within 1e-12 relative (the halves' fp64 totals are added once on the host).
6. Seed and frame indices beyond 32 bits.
7. N = 1024, S = 16, cp + cs = 64, two points, two scales: a chunk of the documented budget ends inside a cell; the chunking
   changes no counter and no penalty byte.
8. ``soft_for_window_file`` equals the direct calls.

Measured on an MI355X (profiles/rx_profile_soft.txt), the largest ratio of test 2 per case, bit_penalty / per symbol: n64_wtx_plain
7.4e-07 / 7.4e-08, n128_wrx_half 1.6e-06 / 2.8e-07, n256_cpw_half_masked 1.4e-05 / 5.7e-07, n512_wola_plain 5.6e-06 / 1.0e-07,
n1024_wtx_half_masked 4.6e-05 / 2.0e-07, n128_cpw_half_nbt0 4.9e-06 / 5.9e-07, n64_cp_masked 2.1e-06 / 2.6e-07; test 3 at most
5.4e-08."""
import functools

import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC
import test_gpu_rx_profile_link as TL

pytestmark = pytest.mark.gpu

CASES = TL.CASES
L = R.LinkPoint
LINK_FIELDS = R.RxProfileLink._fields[:-1]


def points_of(c):
    """the link test's four composed points, and the all-off point"""
    return c["composed"] + [L()]


def run_soft(c, seed, frame_offset, frames, points=None, scales=None, ref_frames=None, **kw):
    s = TL.sides(c, seed, *((frame_offset, frames) if ref_frames is None else ref_frames))
    return W.rx_profile_soft_gpu(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                 points_of(c) if points is None else points, scales, **s, **kw)


def host_soft(c, seed, frame_offset, frames, points=None, scales=None):
    return R.rx_profile_soft_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                  points_of(c) if points is None else points, scales, **TL.sides(c, seed, frame_offset, frames))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, seed, the mirror's soft profile of points_of(case) at the default scales); computed once, not to be modified"""
    c, seed, _, _ = TL.reference(name)
    return c, seed, host_soft(c, seed, 0, RC.FRAMES)


@functools.lru_cache(maxsize=None)
def gpu_profile(name):
    c, seed, _, _ = TL.reference(name)
    return run_soft(c, seed, 0, RC.FRAMES)


same_bits = TL.same_bits


def pen_ratio(got, ref):
    """RC.pow_ratio of the penalties: |got - ref| / (ref[n] + mean_n ref) per (cell, scale) row, the largest"""
    return RC.pow_ratio(got, ref)


# ---- 1. the link fields ----

@pytest.mark.parametrize("name", list(CASES))
def test_link_fields_are_the_link_calls_bytes(name):
    c, seed, _, _ = TL.reference(name)
    soft = gpu_profile(name)
    link = TL.run_gpu(c, seed, 0, RC.FRAMES, points=points_of(c))
    assert type(soft) is R.RxProfileSoft and soft.bit_err.shape == link.bit_err.shape
    assert same_bits([getattr(soft, f) for f in LINK_FIELDS], link[:-1]), name
    assert np.array_equal(soft.decisions, link.decisions)
    plain = RC.run_gpu(c, seed, 0, RC.FRAMES)
    assert same_bits([soft.bit_err[-1], soft.sym_err[-1], soft.err_power[-1]], plain[:3]), "all off"
    n, S, ns = c["st"].n_fft, c["S"], len(R.SOFT_SCALES)
    assert soft.bit_penalty.shape == (5, RC.PAIRS, RC.N_SNR, RC.N_CH, ns, n) and soft.bit_penalty.dtype == np.float64
    assert soft.bit_penalty_sym.shape == (5, RC.PAIRS, RC.N_SNR, RC.N_CH, ns, S - 1)
    assert np.array_equal(soft.scales, np.asarray(R.SOFT_SCALES, np.float32))


# ---- 2. the penalties against the mirror ----

@pytest.mark.parametrize("name", list(CASES))
def test_penalties_against_the_mirror(name):
    """Measured on an MI355X: profiles/rx_profile_soft.txt"""
    c, seed, ref = reference(name)
    soft = gpu_profile(name)
    st = c["st"]
    on = np.ones(st.n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    # (a loaded bin's penalty may be 0 in single precision: at the largest scales every 2^-|t| of a good bin underflows)
    assert (soft.bit_penalty[..., ~on] == 0).all() and np.isfinite(soft.bit_penalty).all() and (soft.bit_penalty >= 0).all()
    worst = worst_sym = 0.0
    for i in range(soft.bit_penalty.shape[0]):
        rb, rs = pen_ratio(soft.bit_penalty[i], ref.bit_penalty[i]), pen_ratio(soft.bit_penalty_sym[i], ref.bit_penalty_sym[i])
        per_scale = [pen_ratio(soft.bit_penalty[i][..., j, :], ref.bit_penalty[i][..., j, :]) for j in range(soft.scales.size)]
        print("%s seed=%d point %d: bit_penalty ratio %.2e (scale %d), per symbol %.2e"
              % (name, seed, i, rb, int(np.argmax(per_scale)), rs))
        worst, worst_sym = max(worst, rb), max(worst_sym, rs)
    k = c["k"]
    print("%s: largest bit_penalty ratio %.2e, per symbol %.2e; rate per point (GPU) %s (mirror) %s"
          % (name, worst, worst_sym, np.round(R.gmi(soft, k)[0].mean(axis=(1, 2, 3)), 4), np.round(R.gmi(ref, k)[0].mean(axis=(1, 2, 3)), 4)))
    assert worst <= RC.POW_TOL and worst_sym <= RC.POW_TOL, (name, worst, worst_sym)


# ---- 3. the symbols add up to the bins ----

@pytest.mark.parametrize("name", list(CASES))
def test_symbol_totals_and_bin_totals_agree(name):
    soft = gpu_profile(name)
    a, b = soft.bit_penalty.sum(axis=-1), soft.bit_penalty_sym.sum(axis=-1)
    rel = np.abs(a - b) / b
    print("%s: symbols against bins, largest relative difference %.2e" % (name, rel.max()))
    assert (b > 0).all() and rel.max() <= 1e-4


# ---- 4. a scale is its own call, a sweep is its points ----

@pytest.mark.parametrize("name", ("n64_wtx_plain", "n256_cpw_half_masked", "n1024_wtx_half_masked"))
def test_a_scale_and_a_point_do_not_depend_on_their_neighbours(name):
    c, seed, _, _ = TL.reference(name)
    allp = gpu_profile(name)
    pts = points_of(c)
    three = run_soft(c, seed, 0, RC.FRAMES, scales=(0.7, R.SOFT_SCALES[5], 0.03))
    one = run_soft(c, seed, 0, RC.FRAMES, scales=(R.SOFT_SCALES[5],))
    assert same_bits(three[:7], one[:7]) and same_bits(three[:7], allp[:7])
    for f in ("bit_penalty", "bit_penalty_sym"):
        mid = np.ascontiguousarray(getattr(three, f)[..., 1, :])
        assert mid.tobytes() == np.ascontiguousarray(getattr(one, f)[..., 0, :]).tobytes(), f
        assert mid.tobytes() == np.ascontiguousarray(getattr(allp, f)[..., 5, :]).tobytes(), f
        assert not np.array_equal(getattr(three, f)[..., 0, :], mid)
    for i in (0, 3, 4):
        alone = run_soft(c, seed, 0, RC.FRAMES, points=[pts[i]])
        assert same_bits(alone[:9], [a[i:i + 1] for a in allp[:9]]), (name, i)
    other = run_soft(c, seed, 0, RC.FRAMES, points=[pts[1], L(linewidth=0.11), pts[0]], scales=R.SOFT_SCALES[:4])
    assert same_bits([a[0] for a in other[:7]], [a[1] for a in allp[:7]])
    assert same_bits([a[2][..., :4, :] for a in other[7:9]], [a[0][..., :4, :] for a in allp[7:9]])


# ---- 5. repeated calls, split frame ranges ----

def test_repeated_calls_are_identical():
    for name in ("n512_wola_plain", "n64_cp_masked"):
        c, seed, _, _ = TL.reference(name)
        assert same_bits(gpu_profile(name)[:9], run_soft(c, seed, 0, RC.FRAMES)[:9]), name


def test_split_frame_ranges_accumulate_to_one_call():
    name = "n256_cpw_half_masked"
    c, seed, _, _ = TL.reference(name)
    one = gpu_profile(name)
    a = run_soft(c, seed, 0, 5, ref_frames=(0, RC.FRAMES))
    both = run_soft(c, seed, 5, 3, ref_frames=(0, RC.FRAMES), out=a)
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym", "decisions"):
        assert np.array_equal(getattr(both, f), getattr(one, f)), f
    assert (both.bit_penalty >= a.bit_penalty).all() and both.bit_penalty.sum() > a.bit_penalty.sum()
    for f in ("err_power", "err_power_sym", "pa_power", "bit_penalty", "bit_penalty_sym"):
        assert RC.pow_ratio(getattr(both, f), getattr(one, f)) < 1e-12, f
    assert np.array_equal(both.scales, one.scales)
    with pytest.raises(ValueError):
        run_soft(c, seed, 5, 3, ref_frames=(0, RC.FRAMES), scales=(1.0,), out=a)


# ---- 6. keys beyond 32 bits ----

def test_seed_and_frame_index_beyond_32_bits():
    """seed with both halves set, frames 2^32 - 3 ... 2^32 + 4: the frame index crosses 2^32 (tests/test_gpu_rng_keys.py's pattern)"""
    c = TL.case("n128_cpw_half_nbt0")
    seed, f0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    pts, sc = [c["composed"][0], L()], (0.5, 0.1)
    ref = host_soft(c, seed, f0, 8, pts, sc)
    got = run_soft(c, seed, f0, 8, pts, sc)
    for i in range(2):
        rb, rs = pen_ratio(got.bit_penalty[i], ref.bit_penalty[i]), pen_ratio(got.bit_penalty_sym[i], ref.bit_penalty_sym[i])
        print("keys beyond 32 bits, point %d: bit_penalty ratio %.2e, per symbol %.2e" % (i, rb, rs))
        assert rb <= RC.POW_TOL and rs <= RC.POW_TOL
    # the low words alone are another experiment: the seed's, and the frames 2^32 ... against 0 ...
    low_seed = run_soft(c, seed & 0xFFFFFFFF, f0, 8, pts, sc, ref_frames=(f0, 8))
    assert pen_ratio(low_seed.bit_penalty, got.bit_penalty) > 1e-2
    high, low = run_soft(c, seed, 2 ** 32, 5, pts, sc, ref_frames=(f0, 8)), run_soft(c, seed, 0, 5, pts, sc, ref_frames=(f0, 8))
    assert pen_ratio(high.bit_penalty, low.bit_penalty) > 1e-2
    part = run_soft(c, seed, f0, 3, pts, sc, ref_frames=(f0, 8))
    assert RC.pow_ratio(part.bit_penalty + high.bit_penalty, got.bit_penalty) < 1e-12


# ---- 7. chunks ----

def test_chunks_and_cells_that_straddle_them():
    """N = 1024, S = 16, cp + cs = 64, two points, two scales: a chunk of the documented budget ends inside a cell; neither the
    split of the frame range nor the link call's other chunking changes an integer counter, and no chunk boundary changes a
    penalty byte (one addition per frame onto the running total)"""
    c = dict(RC.reference_over_the_frame_limit()[0])
    st, S = c["st"], c["S"]
    pts, sc = [L(), L(linewidth=0.01)], (0.5, 0.1)
    c.update(active=CM.half_band_allocation(1024))
    Tv = st.frame_len(S)
    per_chunk = R.rx_profile_soft_chunk_frames(st, S, False, 2, False, 2)
    link_bytes = 8 * (S * 1024 + Tv) + 8 * 2 * (1024 + S + Tv) + 8 * S * st.stride
    assert per_chunk == _lib.RX_PROFILE_CHUNK_BYTES // (link_bytes + 4 * 2 * 2 * ((S - 1) * 1024 + S))
    link_chunk = R.rx_profile_link_chunk_frames(st, S, False, 2, False)
    assert 250 < per_chunk < link_chunk
    frames = per_chunk // 2 + 19                                            # 8 cells: four chunks and a bit

    def run(f0, n, **kw):
        return W.rx_profile_soft_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, f0, n, pts, sc, active=c["active"], **kw)
    one = run(0, frames)
    assert int(one.decisions.max()) == frames * (S - 1) and (frames * 8) % per_chunk != 0 and frames % per_chunk != 0
    assert R.rx_profile_kernel_ms() > 0.0
    link = W.rx_profile_link_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, 0, frames, pts, active=c["active"])
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym"):          # (the link call cuts its chunks elsewhere)
        assert np.array_equal(getattr(one, f), getattr(link, f)), f
    assert RC.pow_ratio(one.err_power, link.err_power) < 1e-12
    parts = run(frames - 7, 7, out=run(0, frames - 7))
    for f in ("bit_err", "sym_err", "bit_err_sym", "sym_err_sym"):
        assert np.array_equal(getattr(parts, f), getattr(one, f)), f
    assert RC.pow_ratio(parts.bit_penalty, one.bit_penalty) < 1e-12 and RC.pow_ratio(parts.bit_penalty_sym, one.bit_penalty_sym) < 1e-12
    # Other chunkings of the same frames: one scale, or one point, makes a frame smaller and a chunk longer, so the chunks end at
    # other frames, inside other cells.  A cell's total is its frames' sums added one by one onto the running total, so every
    # byte -- penalties, powers, counters -- is the same.
    one_scale = R.rx_profile_soft_chunk_frames(st, S, False, 2, False, 1)
    one_point = R.rx_profile_soft_chunk_frames(st, S, False, 1, False, 2)
    assert per_chunk < one_scale < one_point and frames % one_scale != 0 and frames % one_point != 0
    alone = W.rx_profile_soft_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, 0, frames, pts, sc[:1], active=c["active"])
    assert same_bits(alone[:7], one[:7])
    assert same_bits([a[..., 0, :] for a in alone[7:9]], [a[..., 0, :] for a in one[7:9]])
    alone = W.rx_profile_soft_gpu(st, c["k"], S, c["w_tx"], c["w_rx"], c["h"], c["snr"], 7000, 0, frames, pts[1:], sc, active=c["active"])
    assert same_bits(alone[:9], [a[1:] for a in one[:9]])
    assert not np.array_equal(one.bit_penalty[0], one.bit_penalty[1])


# ---- 8. the window file ----

def test_soft_for_window_file_equals_the_direct_calls(channels):
    st = W.make_structure("wtx", 64, 8)
    rs = np.random.RandomState(4)
    win = {"optimizedWindow": W.expand_tx_window(st, np.concatenate(([1.03], np.sort(rs.uniform(0.02, 0.98, 8))[::-1])))}
    kw = dict(num_subcar=64, bits_per_subcar=4, symbols_per_tx=4, ensemble=4, seed=21)
    h, snr, B = channels[:2], [8.0, 16.0], st.stride
    pts = [L(), L(TL.RAPP6, None, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0)), L(pa=TL.RAPP6, aci=(5, 3.0))]
    sc = (0.5, 0.25, 0.05)
    gpu = W.soft_for_window_file("wtx", 8, win, h, snr, pts, sc, gpu=True, **kw)
    hst = W.soft_for_window_file("wtx", 8, win, h, snr, pts, sc, gpu=False, **kw)
    link = W.link_for_window_file("wtx", 8, win, h, snr, pts, gpu=True, **kw)
    assert list(gpu) == list(hst) == ["opt", "rc"]
    alloc = CM.half_band_allocation(64)
    w_tx = np.stack([win["optimizedWindow"], W.tx_rc_window(st)])
    w_rx = np.stack([W.rx_rc_window(st)] * 2)
    for key, mask in (("profile", None), ("profile_masked", CM.tx_mask(st.sym_len))):
        ref = R.pa_ref_power(st, 4, 4, w_tx, 21, 0, 4, active=alloc, mask=mask, gpu=True)
        want = W.rx_profile_soft_gpu(st, 4, 4, w_tx, w_rx, h, snr, 21, 0, 4, pts, sc, aci_active=~alloc, ref_power=ref, active=alloc,
                                     mask=mask)
        for i, name in enumerate(("opt", "rc")):
            g, hh = gpu[name][key], hst[name][key]
            assert type(g) is R.RxProfileSoft and g.bit_penalty.shape == (3, 2, 2, 3, 64) and g.bit_penalty_sym.shape == (3, 2, 2, 3, 3)
            assert same_bits(g[:9], [a[:, i] for a in want[:9]]), (name, key)
            assert same_bits(g[:7], link[name][key][:7]), (name, key)
            assert np.array_equal(g.scales, np.asarray(sc, np.float32)) and np.array_equal(g.decisions, hh.decisions)
            assert (g.bit_penalty[..., ~alloc] == 0).all()
            for p in range(3):
                assert pen_ratio(g.bit_penalty[p], hh.bit_penalty[p]) <= RC.POW_TOL
                assert pen_ratio(g.bit_penalty_sym[p], hh.bit_penalty_sym[p]) <= RC.POW_TOL
