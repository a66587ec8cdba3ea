"""CPU side of the symbol-domain edge tests: the anchors and derived bounds of tests/symbol_f32.py against the pinned oracle, the
reference-executed fixtures and the NumPy float32 models of the five kernels (tests/kernel_models.py ``symbol_demap_model``,
``logits2llrs_model``, ``llrs2logits_model``, ``logits2moments_model``, ``pam2qam_model``), on every case of tests/symbol_cases.py -
the inputs the GPU tests (tests/test_gpu_symbol_edges.py) use.

Shown here, without a GPU:
- each anchor is the oracle's function: ``oracle.mapping.*`` in float64 within 1e-12 on every case with finite inputs, and the
  reference's own output (tests/golden: ``l2l*``, ``l2s*``, ``mom*``, ``p2q*``) within its float32 noise;
- at -inf members, empty sets, LLRs of +-inf, no = 0 and exact ties the anchors return what the reference's own code returns
  (tests/golden/symbol_edges_ref_golden.npz);
- each model, and the oracle, lies inside the bound on every case: the derivation has missed no rounding;
- twelve seeded faults leave the bound on a named case, a thirteenth (the LAST maximum) misses the constructed ties: the checks are
  tight enough to see them;
- the hard-output rule leaves out at most 10 % of the rows of any case.

By construction ``scatter`` in ``pam2qam_model`` (pam1_i + pam2_j placed at i P + j without the gather) is the same function for
nbh <= 2, where the label permutation is its own inverse: it is seeded at nbh = 3 and would not be seen below.  The variance as
E|x|^2 - |mean|^2 is seen only where the variance is small against |x|^2 (a dominant logit); with two equal dominant points its
error, u |x|^2, is inside the bound (0.05) - recorded, not counted twice."""
import os

import numpy as np
import pytest

import kernel_models as km
import symbol_cases as sc
import symbol_f32 as sf
from oracle import mapping as om

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def mapping():
    import sionna_amd.phy as p
    return p.mapping


@pytest.fixture(scope="module")
def ref(mapping):
    """``symbol_cases.expected`` of a case, computed once and shared (read-only)"""
    cache = {}

    def get(case):
        if case.name not in cache:
            ex = sc.expected(case, mapping)
            for x in ex.anchors + ex.bounds:
                x.setflags(write=False)
            cache[case.name] = ex
        return cache[case.name]
    return get


def model(case, ex, hard=False, fault=None):
    """the float32 model's outputs in the order of ``ex.anchors`` (hard: the decision)"""
    m, i = case.m, ex.inputs
    if case.op == "sd":
        out = km.symbol_demap_model(i[0], i[1], ex.pts, i[2], hard_out=hard, fault=fault)
    elif case.op == "l2l":
        out = km.logits2llrs_model(i[0], m, case.method, i[1], hard_out=hard, fault=fault)
    elif case.op == "l2s":
        out = km.llrs2logits_model(i[0], m, hard_out=hard, fault=fault)
    elif case.op == "mom":
        mean, var = km.logits2moments_model(i[0], ex.pts, fault=fault)
        return mean.real, mean.imag, var
    else:
        out = km.pam2qam_model(i[0], i[1], m // 2, fault=fault)
    return out if hard else (out,)


def _finite_inputs(ex):
    return all(x is None or np.all(np.isfinite(x)) for x in ex.inputs)


def _oracle(case, ex):
    i, m = ex.inputs, case.m
    w = lambda x: None if x is None else np.asarray(x, np.complex128 if np.iscomplexobj(x) else np.float64)
    if case.op == "sd":
        no = w(i[1])
        return (om.symbol_demapper(w(i[0]), no if no.size > 1 else float(no[0]), w(ex.pts), w(i[2])),)
    if case.op == "l2l":
        return (om.symbol_logits2llrs(w(i[0]), m, case.method, w(i[1])),)
    if case.op == "l2s":
        return (om.llrs2symbol_logits(w(i[0]), m),)
    if case.op == "mom":
        mean, var = om.symbol_logits2moments(w(i[0]), w(ex.pts))
        return mean.real, mean.imag, var
    return (om.pam2qam(i[0], i[1], m, hard_in_out=False),)


ORACLE_CASES = [c for c in sc.ALL if c.n and c.no != "zero"]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_anchor_equals_oracle_and_oracle_inside_the_bound(ref, case):
    """float64 against float64 at 1e-12 of the quantities that are subtracted (|e_c| + |lse|; |R_1| + |R_0|; sum_j |ls_j|;
    E|x| and E|x|^2) wherever the inputs are finite; on EVERY case the oracle lies inside the float32 bound (where it is defined:
    at -inf members it follows the same tf rules)"""
    ex = ref(case)
    with np.errstate(all="ignore"):
        o = _oracle(case, ex)
    if _finite_inputs(ex):
        i = ex.inputs
        if case.op == "sd":
            e = sf.sd_exponents(i[0], i[1], ex.pts, i[2])
            scale = (np.abs(e) + np.abs(sf.lse_tf(e))[:, None] + 1e-300,)
        elif case.op == "l2l":
            e = np.abs(sf.l2l_exponents(i[0], case.m, i[1])).max(-1, keepdims=True)
            scale = (2 * e + 1,)
        elif case.op == "l2s":
            scale = (np.abs(ex.anchors[0]) + 1,)
        elif case.op == "mom":
            a = np.abs(ex.pts).max()
            scale = (a, a, a * a)
        else:
            scale = (1e-300,)
        for oo, an, s in zip(o, ex.anchors, scale):
            err = np.max(np.abs(np.asarray(oo, np.float64).reshape(an.shape) - an) / s)
            print(f"{case.name}: anchor vs oracle {err:.2e}")
            assert err <= 1e-12
    q, at = sf.worst(o, ex)
    print(f"{case.name}: oracle / bound {q:.3g} at {at}")
    assert q <= 1


@pytest.mark.parametrize("case", sc.ALL, ids=[c.name for c in sc.ALL])
def test_model_inside_the_bound(ref, case):
    ex = ref(case)
    for an, bd in zip(ex.anchors, ex.bounds):
        assert bd.shape == an.shape and not np.any(np.isnan(bd)) and np.all(bd >= 0)
    q, at = sf.worst(model(case, ex), ex)
    print(f"{case.name}: model {q:.4f} at {at}")
    assert q <= 1, (case.name, q, at)


HARD = [c for c in sc.ALL if c.hard]


@pytest.mark.parametrize("case", HARD, ids=[c.name for c in HARD])
def test_hard_rule_on_the_model(ref, case):
    """the share of rows the gap rule leaves out is a condition on the inputs: at most 10 %, from the anchor alone; the model decides
    as the anchor on the certain rows and takes the first maximum (bit LLRs: 0) on the exact ties of the cases built for them"""
    ex = ref(case)
    checked = ex.sure | (ex.tied if case.tie else False)
    share = 1 - checked.mean()
    print(f"{case.name}: {share:.1%} of the decisions left out, {int(np.sum(ex.tied))} exact ties")
    assert share <= 0.10
    if case.tie:
        assert ex.tied.any()
    hard = np.asarray(model(case, ex, hard=True), np.float64).reshape(ex.decision.shape)
    assert np.array_equal(hard[checked], ex.decision[checked])


FAULTS = [("no_shift", "sd4_qam_far"), ("sum_pm1", "sd2_qam_random_span"), ("sum_pm1", "mom4_qam_dom20"), ("prior_as_vec", "l2l6_app_prior_mat50"),
          ("lsb_first", "l2l3_max_normal"), ("lsb_first", "l2l8_app_normal"), ("sign_swapped", "l2s3_small"), ("naive_log_sigmoid", "l2s6_c104"),
          ("var_cancel", "mom4_qam_dom20"), ("var_cancel", "mom3_c3_dom20"), ("var_about_0", "mom3_c3_normal"), ("den_unshifted", "mom6_qam_offset"),
          ("unclamped", "l2l4_app_low_inf"), ("unclamped", "l2l4_app_low_1e10"), ("unclamped", "l2l3_app_low_fltmax"), ("unclamped", "l2l4_app_from_llrs"),
          ("no_empty_rule", "l2l3_app_empty"), ("scatter", "p2q6_n257")]


@pytest.mark.parametrize("fault,name", FAULTS, ids=[f"{f}-{n}" for f, n in FAULTS])
def test_seeded_fault_leaves_the_bound(ref, fault, name):
    """the max shift dropped; the sum over P - 1 points; a prior [n, m] indexed as [m]; label bits LSB first; the two log_sigmoid signs
    swapped on bit 0; log_sigmoid as log(1 / (1 + exp(-p))); the variance as E|x|^2 - |mean|^2 and about 0; den from an un-shifted pass;
    ``exp_core_f32`` without the clamp at -104 on members at -inf, -FLT_MAX, -1e10 and on the logits of LLRs of +-inf; a whole set at
    -inf without the rule for a non-finite maximum; the PAM2QAM gather replaced by a scatter"""
    case = sc.BY_NAME[name]
    ex = ref(case)
    q, at = sf.worst(model(case, ex, fault=fault), ex)
    print(f"fault {fault} on {name}: {q:.3g} at {at}")
    assert q > 1, (fault, name, q)


LAST_MAX = ["sd4_hard_ties", "l2s2_zero"]


@pytest.mark.parametrize("name", LAST_MAX)
def test_last_maximum_fault_is_seen_on_the_ties(ref, name):
    case = sc.BY_NAME[name]
    ex = ref(case)
    hard = model(case, ex, hard=True, fault="last_max")
    assert not np.array_equal(hard[ex.tied], ex.decision[ex.tied])


def test_unfixed_kernel_model_fails_exactly_the_cases_built_for_it(ref):
    """the model of ``logits2llrs_kernel`` before the clamp and the empty-set rule leaves the bound on the cases with members at -inf,
    -FLT_MAX, -1e10, with a whole set at -inf and on the logits LLRs2SymbolLogits forms from LLRs of +-inf - and on no other"""
    bad = set()
    for case in sc.L2L:
        ex = ref(case)
        if sf.worst(model(case, ex, fault="unfixed"), ex)[0] > 1:
            bad.add(case.name)
    print(sorted(bad))
    assert bad == {"l2l4_app_low_1e10", "l2l3_app_low_fltmax", "l2l4_app_low_inf", "l2l3_app_empty", "l2l4_app_from_llrs"}


def test_round_trip_returns_the_llrs(ref):
    """LLRs2SymbolLogits -> SymbolLogits2LLRs("app"): the LLRs come back within the bound of the second block on the first block's
    float32 output plus the first block's bounds carried through (an LLR is a difference of two reductions over logits that each
    contain the bit's own log-sigmoid once: twice the largest logit bound of the row), +-inf preserved"""
    case = sc.BY_NAME["l2s4_roundtrip"]
    ex = ref(case)
    llrs, m = ex.inputs[0], case.m
    logits = km.llrs2logits_model(llrs, m)
    back = km.logits2llrs_model(logits, m, "app")
    q = sf.round_trip_ratio(llrs, logits, back, ex.bounds[0], m)
    print(f"round trip: {q:.3g}")
    assert q <= 1


def test_anchors_against_the_reference_executed_fixtures():
    """the reference's own float32 output: within 1e-5 max(1, |ref|) (its float32 noise: tests/test_oracle_ref_exec_symbol.py holds the
    oracle to the same)"""
    phy, sym = np.load(os.path.join(GOLD, "phy_ref_golden.npz")), np.load(os.path.join(GOLD, "symbol_ref_golden.npz"))

    def near(a, b):
        b = np.asarray(b, np.float64)
        return np.all(np.abs(np.asarray(a, np.float64).reshape(b.shape) - b) <= 1e-5 * np.maximum(1, np.abs(b)))
    for m in (1, 2, 4, 6):
        z, pr, pv = phy[f"l2l{m}_z"], phy[f"l2l{m}_prior"], phy[f"l2l{m}_prior_vec"]
        for meth in ("app", "maxlog"):
            assert near(sf.anchor_logits2llrs(z, m, meth), phy[f"l2l{m}_{meth}"])
            assert near(sf.anchor_logits2llrs(z, m, meth, pr.reshape(-1, m)), phy[f"l2l{m}_{meth}_prior"])
            assert near(sf.anchor_logits2llrs(z, m, meth, pv), phy[f"l2l{m}_{meth}_prior_vec"])
        assert near(sf.anchor_llrs2logits(sym[f"l2s{m}_llrs"], m), sym[f"l2s{m}_logits"])
        assert np.array_equal(sf.anchor_llrs2logits(sym[f"l2s{m}_llrs"], m, hard=True), sym[f"l2s{m}_hard"].reshape(-1))
    for m in (2, 4, 6):
        mr, mi, var = sf.anchor_moments(sym[f"mom{m}_logits"], om.qam(m))
        assert near(mr, sym[f"mom{m}_mean"].real) and near(mi, sym[f"mom{m}_mean"].imag) and near(var, sym[f"mom{m}_var"])
        assert np.array_equal(sf.anchor_pam2qam(sym[f"p2q{m}_a"], sym[f"p2q{m}_b"], m // 2).reshape(sym[f"p2q{m}_logits"].shape), sym[f"p2q{m}_logits"])


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_anchors_at_the_edges_the_reference_defines(p):
    """tests/golden/symbol_edges_ref_golden.npz: infinities and NaN in the same places, finite values within the precision's noise"""
    g = np.load(os.path.join(GOLD, "symbol_edges_ref_golden.npz"))
    tol = 1e-5 if p == "f32" else 1e-12

    def same(a, b, rel=tol):
        a, b = np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64)
        fin = np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
        assert np.all(np.abs(a[fin] - b[fin]) <= rel * np.maximum(1, np.abs(b[fin])))
    z, pr = g[f"l2l_z_{p}"], g[f"l2l_prior_{p}"]
    for meth in ("app", "maxlog"):
        same(sf.anchor_logits2llrs(z, 2, meth), g[f"l2l_{meth}_{p}"])
        same(sf.anchor_logits2llrs(z, 2, meth, pr), g[f"l2l_{meth}_prior_{p}"])
        with np.errstate(invalid="ignore"):
            same(sf.anchor_logits2llrs(z, 2, meth) > 0, g[f"l2l_{meth}_hard_{p}"])
    l = g[f"l2s_llrs_{p}"]
    same(sf.anchor_llrs2logits(l, 3), g[f"l2s_logits_{p}"])
    assert np.array_equal(sf.anchor_llrs2logits(l, 3, hard=True), g[f"l2s_hard_{p}"])
    same(sf.anchor_logits2llrs(sf.anchor_llrs2logits(l, 3), 3, "app"), g[f"l2s_round_{p}"])
    pts = om.qam(4, dtype=np.complex64 if p == "f32" else np.complex128)
    y, prior = g[f"sd_y_{p}"], g[f"sd_prior_{p}"]
    for name, no in (("zero", 0.0), ("tiny", float(np.finfo(np.float32).tiny)), ("one", 1.0)):
        # (float32 reference at no = tiny: |e| of 1e38, its own rounding is relative to that)
        a = sf.anchor_symbol_demap(y, np.float64(no), pts)
        ref = np.asarray(g[f"sd_{name}_{p}"], np.float64)
        if name == "zero":
            assert np.all(np.isnan(ref)) and np.all(np.isnan(a)), "the reference defines nothing at no = 0"
            continue
        assert np.all(np.abs(a - ref) <= (1e-6 if p == "f32" else 1e-12) * np.maximum(1, np.abs(ref).max(-1, keepdims=True)))
        assert np.array_equal(sf.anchor_symbol_demap(y, np.float64(no), pts, hard=True), g[f"sd_{name}_hard_{p}"])
    same(sf.anchor_symbol_demap(y, 1.0, pts, prior), g[f"sd_one_prior_{p}"])
    assert np.array_equal(sf.anchor_symbol_demap(y, 1.0, pts, prior, hard=True), g[f"sd_one_prior_hard_{p}"])
    mr, mi, var = sf.anchor_moments(g[f"mom_z_{p}"], om.qam(2, dtype=np.complex128))
    ref_var = g[f"mom_var_{p}"]
    same(mr, g[f"mom_mean_{p}"].real, 1e-6 if p == "f32" else tol)
    same(mi, g[f"mom_mean_{p}"].imag, 1e-6 if p == "f32" else tol)
    # (the reference at a common offset of 1e6 forms lse = 1e6 + ln 4: that costs it 1e6 u in every exponent - 0.06 in float32,
    # 1e-10 in float64)
    same(var, ref_var, 0.1 if p == "f32" else 1e-9)


def test_every_axis_value_of_the_issue_appears():
    by = lambda op: [c for c in sc.ALL if c.op == op]
    sd, l2l, l2s, mom, p2q = (by(o) for o in ("sd", "l2l", "l2s", "mom", "p2q"))
    assert 60 <= len(sc.ALL) <= 95 and max(c.n for c in sc.ALL) <= 257
    assert all(c.n <= 64 for c in sc.ALL if c.m == 10 and c.op != "p2q")
    assert {c.m for c in sd} == {c.m for c in mom} == {1, 2, 3, 4, 6, 8, 10} and {c.m for c in l2l} >= {1, 2, 3, 4, 6, 8}
    assert {c.m for c in l2s} >= {1, 2, 3, 4, 6, 8} and {c.m for c in p2q} == {2, 4, 6, 8, 10}
    for lst in (sd, l2l, mom):
        assert {c.n for c in lst} >= {0, 1, 255, 256, 257}
    assert {c.n for c in l2s} >= {0, 1, 63, 64, 65, 129} and {c.n for c in p2q} >= {0, 1, 257}
    assert {c.table for c in sd} >= {"qam", "pam", "c3"} and {c.table for c in mom} >= {"qam", "pam", "c3"}
    assert {c.kind for c in sd} >= {"points", "midway", "far", "random"} and {c.no for c in sd} >= {"span", "tiny", "zero", 1e-4, 1e4}
    assert {c.prior[0] for c in sd if c.prior} >= {"vec", "mat", "pm", "inf"}
    assert {c.kind for c in l2l} >= {"normal", ("dom", 100.0), ("dom", 1e4), "equal", ("offset", 1e6), ("offset", -1e6), "gaps",
                                     ("low", -1e10), ("low", -sc.FLT_MAX), ("low", -np.inf), "empty", "from_llrs"}
    assert {c.prior for c in l2l} >= {None, ("vec", 0.0), ("vec", 1.0), ("mat", 50.0), ("vec", 5000.0), ("mat", 5000.0)}
    assert all(c.hard for c in l2l if c.prior and c.prior[1] == 5000.0) and {c.method for c in l2l} == {"app", "maxlog"}
    assert {c.kind for c in l2s} >= {("const", a) for a in (0.0, 1e-3, 20.0, 88.0, 104.0, 1e4, np.inf)} | {"mixed", "roundtrip"}
    assert {c.kind for c in mom} >= {"uniform", ("dom", 20.0), ("dom", 100.0), ("dom", 1e4), "two", "offset", "low", "normal"}
    assert all(any(c.hard for c in lst) for lst in (sd, l2l, l2s)) and all(any(c.tie for c in lst) for lst in (sd, l2l, l2s))


def test_moments_bound_scales_with_the_variance():
    """one dominant logit by 20: the variance is 6e-9 ... 2e-6 and its bound below 1e-3 OF IT (the square of the mean's own bound,
    22 u |x|, is the largest part) - the former bar of tests/test_gpu_symbol.py, 4e-5 max(var, 1), is 1e6 times the largest bound"""
    import sionna_amd.phy as p
    ex = sc.expected(sc.BY_NAME["mom4_qam_dom20"], p.mapping)
    var, bd = ex.anchors[2], ex.bounds[2]
    print(f"var {var.min():.3g} ... {var.max():.3g}, bound / var {np.max(bd / var):.3g}, max bound {bd.max():.3g}")
    assert var.max() < 1e-5 and np.max(bd / var) < 1e-3 and bd.max() < 4e-5 * 1e-6
