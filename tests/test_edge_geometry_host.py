"""The geometry-limit cases (tests/edge_geometry_cases.py) without a GPU: the oracle-only conditions the GPU tests rely on -- the
seed's cap on near decisions, errors of both kinds in every pair at both SNR points, fewer than half of the decisions wrong at the
upper one --, the fp64 mirror ``rx_profile_host`` against the oracle at every geometry, the mirrors' conditions of the three cases
that run the combined chain, the layout the frame kernels are expected to pick, and the documented limits one step outside (what
tests/test_rx_profile_abi.py does not assert already)."""
import numpy as np
import pytest

import wofdm_amd as W
from wofdm_amd import _lib
from wofdm_amd import variants as V

import doppler_cases as DC
import edge_geometry_cases as EC
import kernel_cases as KC
import rx_profile_cases as RC
import test_rx_profile_abi as ABI


def test_the_list_keeps_its_spread():
    """all three constellations, both noise orders, at least two cases (one of them masked) at noise_before_truncate = 0, eleven
    geometries of which the frame kernels take seven"""
    rows = list(EC.CASES.values())
    assert len(rows) == 11 and len(EC.PLAN_CASES) == 7 and len(EC.REFUSED_CASES) == 4
    assert {r[8] for r in rows} == {2, 4, 6} and {r[10] for r in rows} == {0, 1}
    nbt0 = [r for r in rows if r[10] == 0]
    assert len(nbt0) >= 2 and any(r[7].endswith("masked") for r in nbt0)
    assert {r[0] for r in rows} == set(V.SYSTEMS)
    for name in EC.CASES:
        st = EC.structure(name)
        assert st.tail_rx <= 64 and st.cp <= st.n_fft and st.cs <= st.n_fft and 2 * st.tail_tx <= st.sym_len
    st = EC.structure("fold_all_n64")
    assert (st.sym_len, st.stride - st.n_fft, st.tail_rx, st.cp, st.cs) == (192, 96, 64, 64, 64)
    assert EC.structure("plan_n256_cpw").stride == 320 and EC.structure("plan_n1024_wrx").stride == 1024 + 64
    assert EC.structure("cpwtx_n256").circ_shift == 48 and EC.structure("plan_n128_wola").circ_shift == 32


@pytest.mark.parametrize("name", list(EC.CASES))
def test_the_oracle_meets_the_conditions(name):
    c, seed, ref = EC.reference(name)
    share = ref["near"].sum() / ref["decisions"]
    print("%s: seed %d, near share %.4f" % (name, seed, share))
    assert EC.BASE_SEED <= seed < EC.BASE_SEED + 32 and share <= 0.01
    n_on = c["st"].n_fft if c["active"] is None else int(np.count_nonzero(c["active"]))
    assert ref["decisions"] == 8 * RC.FRAMES * (c["S"] - 1) * n_on == int(ref["counts"][..., 3].sum())
    assert c["h"].shape == (RC.N_CH, EC.CASES[name][6])
    EC.check_error_rates(c, ref["bit"], ref["sym"], ref["decisions"], name)


@pytest.mark.parametrize("name", list(EC.CASES))
def test_the_mirror_equals_the_oracle(name):
    c, seed, ref = EC.reference(name)
    prof, near = W.rx_profile_host(*EC.head(c, seed), active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"],
                                   with_near=True)
    assert np.array_equal(prof.bit_err.astype(np.int64), ref["bit"]) and np.array_equal(prof.sym_err.astype(np.int64), ref["sym"])
    assert np.array_equal(near, ref["near"])
    assert int(prof.decisions.sum()) * 8 == ref["decisions"]
    ratio = RC.pow_ratio(prof.err_power, ref["pow"])
    print("%s: err_power of the mirror against the oracle %.2e" % (name, ratio))
    assert ratio < 1e-10


@pytest.mark.parametrize("name", list(EC.LINK_CASES))
def test_the_link_mirror_meets_the_conditions(name):
    c, seed, prof, near = EC.link_reference(name)
    dec = DC.decisions_of(c, RC.FRAMES)
    share = near.sum(axis=(1, 2, 3)) / dec
    print("%s: seed %d, near shares per point %s" % (name, seed, np.round(share, 4)))
    assert (share <= 0.01).all()
    EC.check_error_rates(c, prof.bit_err, prof.sym_err, dec, name + " link")
    st, (early, late) = c["st"], c["points"]
    assert st.prefix_rm + early.timing == -3 and early.aci[0] == st.stride - 1 and (late.timing, late.aci[0]) == (5, 0)
    assert (early.cfo_tracked, early.cpe_tracked, late.cfo_tracked, late.cpe_tracked) == (1, 1, 0, 0)
    assert early.cfo > 0 and early.linewidth > 0 and c["aci_active"].any() and early.track == late.track == 1
    # the two points are two experiments, and the moving track is no copy of the static one
    assert (np.abs(prof.err_power[0] - prof.err_power[1]).max(axis=-1) > 0).all()
    assert np.abs(c["tracks"][1] - c["tracks"][0]).max() > 0


def test_the_tracking_mirror_meets_the_conditions():
    c, seed, prof, near = EC.tracking_reference()
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    dec = cells * prof.decisions.sum(axis=-1).astype(np.float64)
    share = near.sum(axis=(1, 2, 3)) / dec
    print("%s tracking: seed %d, near shares per point %s" % (c["name"], seed, np.round(share, 4)))
    assert (share <= 0.01).all()
    assert c["S"] >= 3 and c["pilots"].sum() == c["on"].sum() // 8 and all(tp == (1, 1) for tp in c["tracking"])
    ser = prof.sym_err.sum(axis=(1, 3, 4)) / (dec[:, None] / RC.N_SNR)
    print("%s tracking: symbol-error rate [point, SNR point] %s" % (c["name"], np.round(ser, 4)))
    assert (prof.sym_err.sum(axis=(-1, -2)) > 0).all() and (ser[:, 1] < 0.5).all()


@pytest.mark.parametrize("name", list(EC.CASES))
def test_the_expected_kernel_of_the_plan_cases(name):
    c = EC.case(name)
    st, S = c["st"], c["S"]
    takes = st.stride - st.n_fft <= 64 and st.tail_tx <= 16 and st.cp + st.cs <= (64 if st.n_fft >= 1024 else 128)
    assert takes == (name in EC.PLAN_CASES)
    if takes:
        layout, var = KC.expected_kernel_id(st, S, None, EC.plan_var(c))
        print("%s: stride %d, S %d: the frame kernels run layout %d, variant %d" % (name, st.stride, S, layout, var))
        assert KC.layout_info(layout, st.n_fft) is not None and var in KC.layout_info(layout, st.n_fft)["vars"]
        for opts in ({"dft_valu": 1}, {"fir_valu": 1}):
            lay, _ = KC.expected_kernel_id(st, S, opts, EC.plan_var(c))
            print("%s: with %s layout %d" % (name, opts, lay))


def test_every_case_passes_the_argument_checks():
    """the receive profile takes all eleven: the call fails only at the device (this machine has none)"""
    for name in EC.CASES:
        c = EC.case(name)
        rc = ABI._call(st=c["st"], k=c["k"], S=c["S"], n_taps=c["h"].shape[1], mask=c["mask"] is not None, active=c["active"])
        assert rc == -3, (name, rc, _lib.load().wofdm_last_error().decode())


def test_the_limits_one_step_outside():
    err = lambda: _lib.load().wofdm_last_error().decode()
    # 2 tail_tx <= P with the geometry identity kept: P = 192, tail_tx = 96 is the limit itself; P = 191 is one sample short
    assert ABI._call(st=V.Structure("custom", 64, 64, 96, 0, 64, 32, 0)) == -3
    assert ABI._call(st=V.Structure("custom", 64, 63, 96, 0, 64, 31, 0)) == -2 and "2 tail_tx <= P" in err()
    # tail_rx = 64 and 21 taps at N = 64 pass, one step further does not (the identity kept)
    st = EC.structure("fold_all_n64")
    assert ABI._call(st=st, n_taps=21) == -3 and ABI._call(st=st, n_taps=22) == -2
    over = V.Structure("custom", 64, 64, 31, 66, 64, 31, 0)
    assert over.stride == 64 + 66 + 31 and ABI._call(st=over) == -2 and "tail_rx" in err()
    # cp = n_fft passes, n_fft + 1 does not; circ_shift = n_fft - 1 passes, n_fft does not
    st = EC.structure("cpfull_n128")
    assert ABI._call(st=st) == -3
    assert ABI._call(st=V.Structure("CP", 128, 129, 0, 0, 0, 129, 0)) == -2
    assert ABI._call(st=st, cfg_edit=lambda c: setattr(c, "circ_shift", 127)) == -3
    assert ABI._call(st=st, cfg_edit=lambda c: setattr(c, "circ_shift", 128)) == -1
    # the mask's own limit 3 P - 2 <= 8 n_fft: fold_all_n64 (P = 192) runs unmasked only
    st = EC.structure("fold_all_n64")
    assert 3 * st.sym_len - 2 > 8 * st.n_fft
    assert ABI._call(st=st, mask=True) == -2 and "3 P - 2 <= 8 n_fft" in err()
    assert ABI._call(st=st) == -3
