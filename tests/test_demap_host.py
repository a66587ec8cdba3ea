"""CPU side of the demapper edge tests: the float64 anchor and the derived bound of tests/demap_f32.py against the pinned oracle and
against the NumPy float32 models of the two LLR kernels (tests/kernel_models.py ``demap_square_model``, ``demap_generic_model``), on
every case of tests/demap_cases.py - the inputs the GPU tests (tests/test_gpu_demap_edges.py) use.

Shown here, without a GPU:
- the anchor is the oracle's function: ``oracle.mapping.demapper`` in float64 within 1e-12 of |R_1| + |R_0| on every case;
- each model lies inside the bound on every case: the derivation has missed no rounding of the kernels' arithmetic;
- a seeded one-line fault in a model leaves the bound on a named case: the bound is tight enough to see it;
- the square kernel's former switch at 80 loses members of a set to the flush of exponentials below 2^-126 and leaves the bound;
- at the C2 operating point the bound is far below the former atol.
"""
import numpy as np
import pytest

import demap_cases as dc
import demap_f32 as df
import kernel_models as km
from oracle import mapping as om


@pytest.fixture(scope="module")
def mapping():
    import sionna_amd.phy as p
    return p.mapping


@pytest.fixture(scope="module")
def ref(mapping):
    """inputs, table, anchor and bound of a case, computed once and shared (read-only)"""
    cache = {}

    def get(case):
        if case.name not in cache:
            y, no, prior = dc.inputs(case, mapping)
            tab = dc.table(case, mapping)
            an = df.anchor(y, no, tab, case.method, prior)
            bd = df.bound(y, no, tab, case.method, prior)
            for x in (an, bd):
                x.setflags(write=False)
            cache[case.name] = (y, no, prior, tab, an, bd)
        return cache[case.name]
    return get


def _model(case, y, no, prior, tab, hard=False, **kw):
    if case.kernel == "square":
        return km.demap_square_model(y, no, tab, case.method, hard_out=hard, **kw)
    return km.demap_generic_model(y, no, tab, case.method, prior=prior, hard_out=hard, **kw)


@pytest.mark.parametrize("case", dc.ALL, ids=[c.name for c in dc.ALL])
def test_anchor_equals_oracle(mapping, ref, case):
    """float64 against float64: the two differ in the order of their sums and in |.|^2 formed through abs(); both errors are
    relative to the reductions that are subtracted, so the bar is 1e-12 (|R_1| + |R_0|)"""
    y, no, prior, tab, an, _ = ref(case)
    pts = dc.points(case, mapping)
    if case.kernel == "square":
        assert np.array_equal(df.points_from_levels(tab), pts.astype(np.complex128))
    _, r1, r0 = df.anchor(y, no, tab, case.method, prior, parts=True)
    no64 = np.maximum(no.astype(np.float64), df.TINY)            # the float32 formula clamps at float32's tiny
    o = om.demapper(y.astype(np.complex128), no64 if no.size > 1 else float(no64[0]), pts.astype(np.complex128),
                    case.method, prior=None if prior is None else prior.astype(np.float64))
    assert o.dtype == np.float64 and np.all(np.isfinite(o)) and np.all(np.isfinite(an))
    err = np.abs(o.reshape(an.shape) - an) / (np.abs(r1) + np.abs(r0) + 1e-300)
    print(f"{case.name}: anchor vs oracle {err.max():.2e}")
    assert err.max() <= 1e-12


@pytest.mark.parametrize("case", dc.ALL, ids=[c.name for c in dc.ALL])
def test_model_inside_the_bound(ref, case):
    y, no, prior, tab, an, bd = ref(case)
    assert np.all(bd > 0) and np.all(np.isfinite(bd))
    out = _model(case, y, no, prior, tab)
    q, at = df.ratio(out, an, bd)
    print(f"{case.name}: model {q:.4f} at {at}, max bound {bd.max():.3e}, max bound / |anchor| {np.max(bd / np.maximum(np.abs(an), 1e-300)):.2e}")
    assert q <= 1, (case.name, q, at)
    if case.hard:
        hard = _model(case, y, no, prior, tab, hard=True)
        sure = np.abs(an) > bd
        assert sure.any() and np.array_equal(hard[sure], (an > 0).astype(np.float32)[sure])


FAULTS = [("bit_order", "sq4_app_points"), ("axes_swapped", "sq6_app_c2"), ("no_threshold", "sq4_app_gap"), ("no_threshold", "sq6_app_gap"),
          ("neighbour_no", "sq6_app_random_alt"), ("neighbour_no", "g8_app_qam_random"), ("no0", "sq4_app_random_alt"),
          ("no0", "g1_app_pam_random"), ("level_4ulp", "sq10_app_points"), ("level_4ulp", "sq8_max_points"),
          ("prior_sign", "p2_app_vec1"), ("prior_sign", "p6_app_mat50"), ("no_tiny", "sq4_app_no_zero"), ("no_tiny", "sq4_max_no_zero"),
          ("no_tiny", "g4_app_no_zero"), ("no_clamp", "g4_app_no_zero")]


@pytest.mark.parametrize("fault,name", FAULTS, ids=[f"{f}-{n}" for f, n in FAULTS])
def test_seeded_fault_leaves_the_bound(ref, fault, name):
    """the bit order t for NB - 1 - t; the axes swapped; the switch to per-set maxima removed; the neighbour's no (what a wrong
    prefetch would use); no[0] where no is per symbol; one level 4 ulp off; the prior's sign; the clamp of no to finfo.tiny dropped
    at no = 0 with y on a point (0 * inf).  Eight faults, each outside the bound - and a ninth, ``no_clamp``: ``exp_core_f32`` on an
    argument of -1e28, where the residual of its extended product overflows exp2 (the generic kernel before its clamp at -104)"""
    case = dc.BY_NAME[name]
    y, no, prior, tab, an, bd = ref(case)
    q, at = df.ratio(_model(case, y, no, prior, tab, fault=fault), an, bd)
    print(f"fault {fault} on {name}: {q:.3g} at {at}")
    assert q > 1, (fault, name, q)


def test_plain_product_fault_is_below_the_bound(ref):
    """``demap_exp`` with a plain float32 product x log2(e): the high part of log2(e) is 0.22 u off, so the exponential moves by
    0.22 u |x| - beside the u |x| that the rounding of the product's sum costs in either form, and below the 5 u |e| the bound must
    grant the exponents.  No worst-case bound of this kernel can see it; it is recorded here, not counted among the eight"""
    worst = 0.0
    for name in ("sq4_app_gap", "sq6_app_gap", "sq10_app_points"):
        case = dc.BY_NAME[name]
        y, no, prior, tab, an, bd = ref(case)
        worst = max(worst, df.ratio(_model(case, y, no, prior, tab, fault="plain_product"), an, bd)[0])
    print(f"fault plain_product: {worst:.3g}")
    assert worst <= 1


@pytest.mark.parametrize("name", ["sq4_app_gap", "sq6_app_gap"])
def test_flush_at_threshold_80(ref, name):
    """The model with the former switch at 80 LEAVES the bound on the constructed gap cases, where a set's second member lies more
    than 126 ln 2 = 87.34 below the axis maximum while its best member lies within 80: the exponential is returned as 0 and the set's
    sum loses e^-D of its value.  Of the listed pairs that is (gap 79.5, D 12): e^-12 = 6e-6, inside the bound (4.6e-5 there) - and
    (79.5, 8), added for this: e^-8 = 3.4e-4, 7 times the bound.  (79.5, 7.3) stops 0.5 short of the flush point; the largest loss
    the switch at 80 admits is e^-7.34 = 6.5e-4 at gap 80.  With the switch at 64 every symbol is inside (0.34).  The bound is the
    one for the switch at 64: it grants nothing for lost members"""
    case = dc.BY_NAME[name]
    y, no, prior, tab, an, bd = ref(case)
    out = km.demap_square_model(y, no, tab, "app", threshold=80.0)
    q, at = df.ratio(out, an, bd)
    err = np.abs(out - an)
    gd = np.array([(g, d) for g in dc.GAPS for d in dc.DELTAS]).repeat(4, axis=0)
    print(f"{name}: switch at 80: {q:.3g} at {at} (gap, D) = {tuple(gd[at[0]])}, |error| {err[at]:.3g}, bound {bd[at]:.3g}; "
          f"switch at 64: {df.ratio(km.demap_square_model(y, no, tab, 'app'), an, bd)[0]:.3g}")
    assert q > 3 and tuple(gd[at[0]]) == (79.5, 8) and 1e-4 < err[at] < 1e-3
    outside = (err > bd).any(axis=1)
    assert np.array_equal(outside, (gd[:, 0] == 79.5) & (gd[:, 1] == 8)), "exactly the symbols with the flushed second member"


def test_bound_at_the_c2_operating_point(ref):
    """64-QAM, app, no = 0.05 (the C2 chain's demapper): the former bar of test_gpu_parity.py::test_demapper_vs_oracle is
    rtol 1e-5 |ref| + atol 1e-4 max(1, 0.01 max |ref|).  Square kernel: the largest bound over 6000 outputs is 4.6e-5 = atol / 2.2
    (an output with |e| of 70), the median 3.8e-6 = atol / 27 (generic kernel: atol / 3.3 and atol / 15); the bound is below the
    whole former bar on every output"""
    for name in ("sq6_app_c2", "g6_app_qam_c2"):
        y, no, prior, tab, an, bd = ref(dc.BY_NAME[name])
        atol = 1e-4 * max(1.0, 0.01 * np.abs(an).max())
        print(f"{name}: max bound {bd.max():.3e} = atol / {atol / bd.max():.1f}, median bound {np.median(bd):.3e} = atol / {atol / np.median(bd):.1f}")
        assert bd.max() < atol / 2 and np.median(bd) < atol / 10
        assert np.all(bd < 1e-5 * np.abs(an) + atol)


def test_every_axis_value_of_the_issue_appears():
    sq, ge, pr = dc.SQUARE, dc.GENERIC, dc.PRIOR
    assert {c.m for c in sq} == {2, 4, 6, 8, 10} and {c.m for c in ge} == {1, 2, 3, 4, 6, 8, 10}
    assert {c.table for c in ge} >= {"qam", "pam", "rot"} and {c.method for c in sq} == {c.method for c in ge} == {"app", "maxlog"}
    assert any(c.hard for c in sq) and any(c.hard for c in ge) and {c.n for c in dc.ALL} >= {1, 255, 256, 257, 1000}
    for lst in (sq, ge):
        assert {c.pos for c in lst} >= {"points", "midway", "axis", "far3", "far30", "random", "gap"}
        assert any(isinstance(c.no, str) and c.no.startswith("alt") for c in lst) and any(c.no == "span" for c in lst)
        assert {c.no for c in lst if isinstance(c.no, float)} >= {1e-4, 1e4}
    assert {c.m for c in sq if c.pos == "gap"} == {4, 6}
    assert {c.prior for c in pr} >= {("vec", 0.0), ("vec", 1.0), ("mat", 1.0), ("vec", 50.0), ("mat", 50.0), ("vec", 5000.0), ("mat", 5000.0)}
    assert all(c.hard for c in pr if c.prior[1] == 5000.0) and max(c.n for c in dc.ALL) <= 1000
