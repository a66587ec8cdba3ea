"""CPU side of the tap-generator edge tests: the float64 anchors and derived bounds of tests/tdl_f32.py and tests/cdl_f32.py against
the NumPy float32 models of the kernels (tests/kernel_models.py ``tdl_cir_model``, ``cdl_cir_model``) and against the pinned float32
oracles, on every case of tests/tap_channel_cases.py - the inputs the GPU tests (tests/test_gpu_tap_channel_edges.py) use.

What is shown here, without a GPU:
- the model of each kernel lies inside the bound on every case: the derivation has missed no rounding of the kernel's arithmetic;
- the float32 oracle (``oracle.ofdm.tdl_cir``, ``oracle.cdl.CDL``) lies inside the bound of its own anchor (TDL: without the rotation
  term - the oracle evaluates every step directly): the anchor is the pinned oracle's function;
- a seeded one-line fault in the model leaves the bound on a named case: the bound is tight enough to see it.

Largest |model - anchor| / bound over the case list (NumPy's float32 sin / cos, which are closer than the 4 ulp the bound grants):
  TDL   0.141 (D_T200_n2_slow, N = 2);  0.09 at N = 1, 2;  0.02 ... 0.044 at N >= 20 - the bound adds N sinusoids' errors linearly,
        their roundings add like sqrt(N), and 4 ulp are granted where the library delivers about 1
  CDL   0.039 (E_T33, A_panel_T16);  0.011 ... 0.038 elsewhere (20 rays, the same two effects)
  the float32 oracles: TDL 0.141, CDL 0.019 (its interior is float64: what remains is the velocity vector in float32)
Both are above 1/50 and below 1.

The bound against the present bars at the standard cases (asserted below):
  TDL model A, T = 14, B = 64, (4, 2): max bound 3.6e-5 against atol 2e-4 of test_gpu_ofdm.py: 1 / 5.6
  CDL model A uplink "mimo", T = 14, B = 33: max bound 1.16e-4 rms against atol 1e-3 rms of test_gpu_cdl.py: 1 / 8.6
Less than one order of magnitude, not two: the bars were not far above a worst-case count with 4 ulp per sin / cos.  What the new
check adds is less the factor than that it holds on every output (the old atol let a weak tap be wrong altogether: the bound
scales with sqrt(P_p) and with the per-ray magnitudes) and that it scales with |d t| instead of being sized for the largest.

The rotation comment of tdl_cir_kernel (|error| < 2e-6): the bound grants 15 steps x 10.8 u = 1e-5 per sinusoid, the model shows
|model - anchor| <= 7e-7 on a whole tap at the standard cases - the comment agrees with what is observed and stays.

The TDL outputs are held twice: in modulus, and per component (``bound_re``, ``bound_im``, item 10 of tests/tdl_f32.py), where 4 ulp
of a sin or cos are 4 ulp of that value and not a disc of 8 u.  Largest per-component ratios: model 0.23 (D_T200_n2_slow), 0.12 at
N = 1, 2, 0.03 ... 0.08 elsewhere; oracle 0.28.  One seeded fault, ``pi_ulp``, moves a phase by at most 4 u: it cannot leave the
modulus bound (0.34) and leaves the per-component one at t = 0 (79 on N1, 8.3 on N2).
"""
import numpy as np
import pytest

import cdl_f32 as cf
import kernel_models as km
import tap_channel_cases as tc
import tdl_f32 as tf
from oracle import cdl as oc
from oracle import ofdm as o32

SEED = 11


@pytest.fixture(scope="module")
def t38():
    import sionna_amd.phy as p
    return p.channel.tr38901


@pytest.fixture(scope="module")
def tdl_ref(t38):
    """anchor, bounds (modulus, real part, imaginary part) and the arguments of a TDL case, computed once and shared (read-only)"""
    cache = {}

    def get(case):
        if case.name not in cache:
            tdl = tc.tdl_object(t38, case)
            args, kw = tc.tdl_args(tdl, case, SEED)
            ref = tf.anchor_and_bounds(*args, **kw)
            for x in ref:
                x.setflags(write=False)
            cache[case.name] = (tdl, args, kw, ref)
        return cache[case.name]
    return get


def _both(out, ref):
    """the two ratios every TDL output is held to: in modulus, and per component (item 10 of tests/tdl_f32.py)"""
    an, bd, b_re, b_im = ref
    return tf.ratio(out, an, bd), tf.ratio_parts(out, an, b_re, b_im)


@pytest.mark.parametrize("case", tc.TDL, ids=[c.name for c in tc.TDL])
def test_tdl_model_and_oracle_inside_the_bound(tdl_ref, case):
    tdl, args, kw, ref = tdl_ref(case)
    (q, at), (qp, atp) = _both(km.tdl_cir_model(*args, **kw), ref)
    ref0 = tf.anchor_and_bounds(*args, **kw, rotation=False)
    oa, _ = o32.tdl_cir(*args[:5], tdl.delays, *args[5:], **kw)
    (qo, ato), (qop, atop) = _both(oa, ref0)
    print(f"tdl {case.name}: model {q:.4f} at {at} / per component {qp:.4f} at {atp}, oracle {qo:.4f} / {qop:.4f}, "
          f"max bound {ref[1].max():.3e}")
    assert all(np.all(x > 0) for x in ref[1:] + ref0[1:])
    assert np.all(ref[2] <= ref[1] * (1 + 1e-9)) and np.all(ref[3] <= ref[1] * (1 + 1e-9))      # a component's bound is within the disc
    assert q <= 1 and qp <= 1, (case.name, q, at, qp, atp)
    assert qo <= 1 and qop <= 1, (case.name, qo, ato, qop, atop)


TDL_FAULTS = [("restart_t0_plus_1", "D_T17"), ("drop_last", "D_T17"), ("no_reanchor", "D_T200_n2_slow"), ("w_prev", "D_T17"),
              ("theta_no_p", "N25"), ("los_p1", "D_T17"), ("los_sin", "aoa0")]


@pytest.mark.parametrize("fault,name", TDL_FAULTS, ids=[f for f, _ in TDL_FAULTS])
def test_tdl_seeded_fault_leaves_the_bound(tdl_ref, fault, name):
    """the chunk restarted at t0 + 1; the last step of a short chunk dropped; one rotation chain over T = 200; w of the previous
    sinusoid; theta indexed without p where the draws are made per chunk (N > 24); the LoS term at p = 1; sin for cos of the angle.
    Each leaves the bound in modulus"""
    _, args, kw, ref = tdl_ref(tc.TDL_BY_NAME[name])
    q, at = tf.ratio(km.tdl_cir_model(*args, **kw, fault=fault), ref[0], ref[1])
    print(f"tdl fault {fault} on {name}: {q:.3g} at {at}")
    assert q > 1, (fault, name, q)


def test_tdl_uncached_fault_is_inert_in_the_register_path(tdl_ref):
    """``theta_no_p`` sits in the N > 24 branch only: at N = 24 the faulty model equals the sound one"""
    _, args, kw, _ = tdl_ref(tc.TDL_BY_NAME["N24"])
    assert np.array_equal(km.tdl_cir_model(*args, **kw, fault="theta_no_p"), km.tdl_cir_model(*args, **kw))


def test_tdl_fault_pi_one_ulp_leaves_the_bound(tdl_ref):
    """pi replaced by float32(pi) + 1 ulp in the draw intervals, on case N1 (one sinusoid per tap; N2 shows it too).

    The fault moves a phase phi by at most ulp(pi) = 2^-22 = 4 u.  In modulus it cannot be seen: the bound grants every sinusoid a
    disc of 2 C_SC u = 8 u for ``sincosf`` alone (measured: 0.34 on N2, 0.27 on N1, at most 0.12 elsewhere).  Per component it can
    (item 10 of tests/tdl_f32.py): at t = 0 the argument is the stored phi exactly, and where phi lies near +-pi / 2 the real part
    is held to some 30 u of |cos phi| while a phase one float32 step (2 u) off moves it by 2 u |sin phi|.  Measured: 79 on N1, 8.3
    on N2, against 0.12 of the sound model."""
    _, args, kw, ref = tdl_ref(tc.TDL_BY_NAME["N1"])
    (q, _), (qp, atp) = _both(km.tdl_cir_model(*args, **kw, fault="pi_ulp"), ref)
    print(f"tdl fault pi_ulp on N1: in modulus {q:.3g}, per component {qp:.3g} at {atp}")
    assert qp > 1, ("pi_ulp", "N1", qp)
    assert atp[-1] == 0, atp


def test_tdl_bound_against_the_present_bar(t38):
    """the standard case of test_gpu_ofdm.py::test_tdl_matches_oracle_and_statistics: the bound is below its atol = 2e-4"""
    case = tc.TDL_STANDARD
    tdl = t38.TDL(case.model, tc.DELAY_SPREAD, case.fc, min_speed=3., max_speed=30., num_rx_ant=4, num_tx_ant=2)
    args, kw = tc.tdl_args(tdl, case, SEED)
    ref = tf.anchor_and_bounds(*args, **kw)
    an, bd = ref[:2]
    print(f"tdl standard: max bound {bd.max():.3e} = 2e-4 / {2e-4 / bd.max():.1f}")
    assert bd.max() < 2e-4 / 5
    (q, _), (qp, _) = _both(km.tdl_cir_model(*args, **kw), ref)
    assert q <= 1 and qp <= 1, (q, qp)


# ------------------------------------------------------------------ CDL
def _cdl_pair(t38, case):
    cdl = t38.CDL(case.model, tc.DELAY_SPREAD, tc.FC_CDL, *tc.cdl_arrays(t38, case.kind), case.direction, **tc.cdl_kwargs(case))
    ref = oc.CDL(case.model, tc.DELAY_SPREAD, tc.FC_CDL, *tc.cdl_arrays(oc, case.kind), case.direction, **tc.cdl_kwargs(case))
    return cdl, ref


@pytest.fixture(scope="module")
def cdl_ref(t38):
    cache = {}

    def get(case):
        if case.name not in cache:
            cdl, ref = _cdl_pair(t38, case)
            an, bd, m, m_w, tau = cf.anchor_and_bound(ref, SEED, case.call, case.b, case.t, case.fs)
            for x in (an, bd, m, m_w):
                x.setflags(write=False)
            args = (cdl._host_tables(), SEED, case.call, case.b, case.t, case.fs, cdl._min_speed, cdl._max_speed)
            cache[case.name] = (ref, args, an, bd, m, m_w, tau)
        return cache[case.name]
    return get


@pytest.mark.parametrize("case", tc.CDL, ids=[c.name for c in tc.CDL])
def test_cdl_model_and_oracle_inside_the_bound(cdl_ref, case):
    ref, args, an, bd, m, m_w, tau = cdl_ref(case)
    q, at = cf.ratio(km.cdl_cir_model(*args), an, bd)
    oa, otau = ref(SEED, case.call, case.b, case.t, case.fs)
    qo, ato = cf.ratio(oa, an, bd)
    rms = np.sqrt(np.mean(np.abs(an) ** 2))
    print(f"cdl {case.name}: model {q:.4f} at {at}, oracle {qo:.4f} at {ato}, max bound {bd.max() / rms:.3e} rms")
    assert np.all(bd > 0) and np.all(np.abs(an) <= m * (1 + 1e-12)) and np.all(m_w >= 0)
    assert np.array_equal(otau[0, 0, 0], tau.astype(np.float32))
    assert q <= 1, (case.name, q, at)
    assert qo <= 1, (case.name, qo, ato)


CDL_FAULTS = [("zod_next_ray", "E_T33"), ("phases_1_2_swapped", "D_T15"), ("xpr_squared", "D_T15"), ("los_pm_identity", "D_T15"),
              ("los_position_1", "D_T1"), ("amp_unordered", "A_siso_b1"), ("a_tx_conj", "E_T1"), ("pol_tx_ignored", "D_T16"),
              ("time_plus_1", "high_A"), ("r_rx_departure", "D_T17")]


@pytest.mark.parametrize("fault,name", CDL_FAULTS, ids=[f for f, _ in CDL_FAULTS])
def test_cdl_seeded_fault_leaves_the_bound(cdl_ref, fault, name):
    """the zenith-of-departure permutation read at ray m + 1; phase draws 1 and 2 swapped (statistically invisible: it shows on the
    same draws only); xpr_scale squared; the LoS phase matrix diag(1, 1); the LoS term at output position 1; amp[no] for
    amp[order[no]]; a_tx conjugated; pol_tx ignored; the Doppler time t + 1; r_rx indexed by the departure ray pair"""
    _, args, an, bd, _, _, _ = cdl_ref(tc.CDL_BY_NAME[name])
    q, at = cf.ratio(km.cdl_cir_model(*args, fault=fault), an, bd)
    print(f"cdl fault {fault} on {name}: {q:.3g} at {at}")
    assert q > 1, (fault, name, q)


def test_cdl_bound_against_the_present_bar(t38):
    """the standard case of test_gpu_cdl.py::test_cdl_vs_oracle (model A, uplink, "mimo", T = 14, B = 33): the bound is below its
    atol = 1e-3 rms"""
    case = tc.CDL_STANDARD
    cdl, ref = _cdl_pair(t38, case)
    an, bd, _, _, _ = cf.anchor_and_bound(ref, 42, 0, case.b, case.t, case.fs)
    rms = np.sqrt(np.mean(np.abs(an) ** 2))
    print(f"cdl standard: max bound {bd.max() / rms:.3e} rms = 1e-3 rms / {1e-3 * rms / bd.max():.1f}")
    assert bd.max() < 1e-3 * rms / 5


def test_every_axis_value_of_the_issue_appears():
    """the case lists are no full product: every value of every axis is there, and every LoS model meets every T edge"""
    t = tc.TDL
    assert {c.t for c in t} == set(tc.T_EDGES) and {c.n for c in t} >= {1, 2, 20, 24, 25, 40}
    assert {c.model for c in t} == set("ACDE") and {(c.ra, c.ta) for c in t} == {(1, 1), (3, 5)} and {c.b for c in t} == {1, 7}
    assert {round(c.aoa, 3) for c in t if c.model == "D"} == {round(np.pi / 4, 3), 0.0, 2.0} and {c.call for c in t} == {0, 4}
    for m in "DE":
        assert {c.t for c in t if c.model == m} == set(tc.T_EDGES)
    assert {(c.t, c.n) for c in tc.TDL64} == {(a, b) for a in (1, 17, 200) for b in (20, 25)}
    c_ = tc.CDL
    assert {c.t for c in c_} == {1, 15, 16, 17, 33} and {c.model for c in c_} == set("ABCDE") and {c.b for c in c_} == {1, 3}
    assert {c.direction for c in c_} == {"uplink", "downlink"} and {c.kind for c in c_} == {"siso", "mimo", "panel"}
    assert {c.call for c in c_} == {0, 8} and any(c.orient for c in c_) and {c.speeds for c in c_} >= {(0.0, None), (30.0, None), (3.0, 30.0)}
    for m in "DE":
        assert {c.t for c in c_ if c.model == m} == {1, 15, 16, 17, 33}
    assert any(c.kind == "siso" and c.b == 1 and c.model == "A" for c in c_)
    assert {(c.model, c.t) for c in tc.CDL64} == {(m, t) for m in "BD" for t in (1, 17)}
