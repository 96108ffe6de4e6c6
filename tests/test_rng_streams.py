"""The random streams, restated a second time: Philox4x32-10, the data-bit fields and the Box-Muller noise in plain Python
integers, written from the text of csrc/philox.h and DESIGN.md "RNG" -- not from the oracle's C -- and compared with the oracle
at keys whose HIGH words are busy: a 64-bit seed, frame indices on both sides of 2^32 and with all 64 bits in use, cells up
to 2^28 - 1.

The GPU tests compare the kernels with the oracle on the same streams (tests/test_gpu_rng_keys.py at these keys); this
module anchors the oracle, so that the two cannot share a misreading of the layout.  With a zero frame-hi word the first
Philox round multiplies by zero, and with a zero seed-hi word the second key word is a constant: tests that stay below 2^32
cannot see a high word that is dropped, swapped or truncated."""
import math

import numpy as np
import pytest

from oracle import oracle as O

M32 = 0xFFFFFFFF
SEED = 0x9E3779B97F4A7C15                        # distinct, non-zero halves
FRAMES = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 0xFEDCBA9876543210]
CELLS = [0, 65535, 65536, 2 ** 28 - 1]
STREAM_BITS, STREAM_NOISE = 0, 1


# ------------------------------------------------------------------------------------------------------------------
# the definition, from philox.h
def philox4x32_10(ctr, key):
    """Philox4x32-10 of Salmon et al. (SC'11): ten rounds of two 32 x 32 -> 64 multiplies, the key bumped by the Weyl
    constants between rounds."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def stream_block(seed, stream, cell, frame, block):
    """key = (seed lo, seed hi), counter = (block, frame lo, frame hi, stream << 28 | cell)."""
    assert 0 <= cell < 2 ** 28 and 0 <= seed < 2 ** 64 and 0 <= frame < 2 ** 64 and 0 <= block < 2 ** 32
    return philox4x32_10((block, frame & M32, frame >> 32, (stream << 28) | cell), (seed & M32, seed >> 32))


def labels(n_fft, k, S, seed, cell, frame):
    """Subcarrier n of symbol s owns a kslot-bit field (kslot = 2, 4, 8 for k = 2, 4, 6) at bit offset n * kslot of the
    symbol's bit stream: block s * (N * kslot / 128) + (n * kslot >> 7), word (n * kslot >> 5) & 3, shift n * kslot & 31; the
    label is the field's low k bits."""
    kslot = {2: 2, 4: 4, 6: 8}[k]
    per_symbol = n_fft * kslot // 128
    out = np.zeros((S, n_fft), np.uint8)
    blocks = {}
    for s in range(S):
        for n in range(n_fft):
            bit = n * kslot
            b = s * per_symbol + (bit >> 7)
            if b not in blocks:
                blocks[b] = stream_block(seed, STREAM_BITS, cell, frame, b)
            out[s, n] = (blocks[b][(bit >> 5) & 3] >> (bit & 31)) & ((1 << k) - 1)
    return out


def uniforms(w_a, w_b):
    """u1 = fma(w_a, 2^-32, 2^-33) in single precision (the word converted to float first), u2 = (w_b >> 9) * 2^-23: the
    top 23 bits.  Every product and the sum below are exact in double precision, so one rounding to float32 at the end of u1
    is the fused multiply-add."""
    u1 = float(np.float32(float(np.float32(w_a)) * 2.0 ** -32 + 2.0 ** -33))
    u2 = (w_b >> 9) * 2.0 ** -23
    return u1, u2


def unit_noise(n_samples, seed, cell, frame):
    """Block p carries the complex unit normals of samples 2p (words 0, 1) and 2p + 1 (words 2, 3):
    n = sqrt(-2 ln u1) (cos 2 pi u2 + j sin 2 pi u2), here in float64."""
    out = np.zeros(n_samples, np.complex128)
    for j in range(n_samples):
        if j % 2 == 0:
            w = stream_block(seed, STREAM_NOISE, cell, frame, j // 2)
        u1, u2 = uniforms(w[2 * (j % 2)], w[2 * (j % 2) + 1])
        rad, ang = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
        out[j] = complex(rad * math.cos(ang), rad * math.sin(ang))
    return out


# ------------------------------------------------------------------------------------------------------------------
def _sys(n_fft, k, S=5, matlab=1):
    # wtx with a prefix of N / 4 and a Tx tail of 8: (n_fft, k, S, cp, cs, tail_tx, tail_rx, prefix_rm, circ_shift, taps, order)
    return O.make_sys(n_fft, k, S, n_fft // 4, 8, 8, 0, n_fft // 4, 0, 21, matlab)


def test_philox_known_answers():
    """The Random123 known-answer vectors (the ones the GPU hook is checked with): the restatement and the oracle."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert philox4x32_10(ctr, key) == want
        assert tuple(int(x) for x in O.philox(ctr, key)) == want


def test_uniforms_stay_inside_the_open_interval():
    """u1 is never 0 (the logarithm) and never above 1; u2 is in [0, 1)."""
    assert uniforms(0, 0) == (2.0 ** -33, 0.0)
    u1, u2 = uniforms(M32, M32)
    assert u1 == 1.0 and u2 == 1.0 - 2.0 ** -23
    assert uniforms(0x80000000, 0x1FF) == (0.5, 0.0)         # (2^-33 is below half an ulp of 0.5; the low nine bits are dropped)


@pytest.mark.parametrize("n_fft", [64, 256])
@pytest.mark.parametrize("k", [2, 4, 6])
def test_labels_at_key_corners(n_fft, k):
    osys = _sys(n_fft, k)
    seen = set()
    for frame in FRAMES:
        for cell in CELLS:
            want = labels(n_fft, k, osys.syms_per_frame, SEED, cell, frame)
            assert want.max() < (1 << k)
            assert np.array_equal(O.gen_labels(osys, SEED, cell, frame), want), (hex(frame), cell)
            seen.add(want.tobytes())
    assert len(seen) == len(FRAMES) * len(CELLS)              # every key its own stream


@pytest.mark.parametrize("n_fft", [64, 256])
@pytest.mark.parametrize("matlab", [1, 0])
def test_noise_at_key_corners(n_fft, matlab):
    osys = _sys(n_fft, 4, S=3, matlab=matlab)
    nl = O.noise_len(osys)
    assert nl == (osys.T + 20 if matlab else 3 * osys.B)
    worst = 0.0
    for frame in FRAMES:
        for cell in CELLS:
            want = unit_noise(nl, SEED, cell, frame)
            got = O.gen_noise(osys, SEED, cell, frame)
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print("N %d noise_before_truncate %d: %d samples per frame, max |oracle - restatement| / max |.| %.3g" % (n_fft, matlab, nl, worst))
    # the uniforms are formed identically; only the libm calls differ
    assert worst < 1e-12
    # ... and the samples ARE unit normals: sixteen keys of nl samples each, so 32 nl real values
    z = np.concatenate([unit_noise(nl, SEED, c, FRAMES[3]) for c in CELLS])
    n = 2 * z.size
    # (mean of n unit normals: sigma n^-1/2; their mean square: sigma (2 / n)^1/2 -- five sigma)
    assert abs(z.real.mean() + z.imag.mean()) / 2 < 5 / math.sqrt(n)
    assert abs((np.abs(z) ** 2).mean() / 2 - 1) < 5 * math.sqrt(2.0 / n)


def test_every_high_word_matters():
    """Changing only seed >> 32, or only frame >> 32, changes the labels and the noise -- in the restatement and in the
    oracle (which agree, above); so does a cell bit above 2^16."""
    osys = _sys(64, 4, S=3)
    nl = O.noise_len(osys)
    frame, cell = 0x0000000500000007, 3
    base_l, base_n = O.gen_labels(osys, SEED, cell, frame), O.gen_noise(osys, SEED, cell, frame)
    assert np.array_equal(base_l, labels(64, 4, 3, SEED, cell, frame))
    others = [(SEED ^ (1 << 32), cell, frame), (SEED ^ (1 << 63), cell, frame), (SEED & M32, cell, frame),
              (SEED, cell, frame ^ (1 << 32)), (SEED, cell, frame ^ (1 << 63)), (SEED, cell, frame & M32),
              (SEED, cell | (1 << 16), frame), (SEED, cell | (1 << 27), frame),
              # halves swapped
              ((SEED >> 32) | ((SEED & M32) << 32), cell, frame), (SEED, cell, (frame >> 32) | ((frame & M32) << 32))]
    for seed2, cell2, frame2 in others:
        l2, n2 = O.gen_labels(osys, seed2, cell2, frame2), O.gen_noise(osys, seed2, cell2, frame2)
        assert np.array_equal(l2, labels(64, 4, 3, seed2, cell2, frame2))
        # independent streams: about 15 / 16 of the 16-QAM labels differ, and no noise sample repeats
        assert (l2 != base_l).mean() > 0.8, (hex(seed2), cell2, hex(frame2))
        assert np.abs(n2 - base_n).min() > 0 and np.abs(unit_noise(nl, seed2, cell2, frame2) - n2).max() < 1e-12


def test_oracle_run_adds_up_across_the_carry(channels):
    """O.run keys every frame by its global 64-bit index: a range that straddles 2^32 equals the sum of its parts, and differs
    from the same range one carry lower."""
    osys = _sys(64, 4, S=3)
    w_tx, w_rx = np.ones(osys.P), np.ones(64)
    h = channels[11:13].astype(np.complex128)
    snrs = np.array([6.0, 18.0])
    lo, mid, hi = 2 ** 32 - 3, 2 ** 32, 2 ** 32 + 5

    def run(a, b, seed=SEED):
        return O.run(osys, w_tx, w_rx, h, snrs, seed, a, b - a)

    whole = run(lo, hi)
    assert np.array_equal(whole, run(lo, mid) + run(mid, hi))
    assert np.array_equal(whole, run(lo, lo + 1) + run(lo + 1, mid + 1) + run(mid + 1, hi))
    assert np.array_equal(whole[..., 1], np.full((1, 2, 2), 8 * 2 * 64 * 4))
    assert whole[..., 0].min() > 0
    # the frames below 2^32 alone, and the same low words with the high word cleared / the seed's high word cleared, are
    # other experiments
    assert not np.array_equal(run(mid, hi)[..., 0], run(0, hi - mid)[..., 0])
    assert not np.array_equal(run(mid, hi)[..., 0], run(mid, hi, SEED & M32)[..., 0])
    # one frame of it, from the restated draws handed to the oracle's frame function
    cell, frame = 3, mid + 1                                    # cell 3: snr 1, channel 1
    c1, _ = O.frame(osys, w_tx, w_rx, h[1], float(snrs[1]), labels(64, 4, 3, SEED, cell, frame),
                    unit_noise(O.noise_len(osys), SEED, cell, frame))
    assert np.array_equal(c1, run(frame, frame + 1)[0, 1, 1])
