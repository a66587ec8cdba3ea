"""The two LLR kernels behind ``Demapper`` - ``demap_square_qam_kernel`` (csrc/demap_core.h ``square_qam_llr``) and the generic
``demap_kernel<M, MAXLOG>`` with and without a prior (csrc/mapping.hip) - through ``phy.mapping.Demapper`` against the float64 anchor
of tests/demap_f32.py, on EVERY output, within the bound derived there from the kernels' arithmetic (u = 2^-24).  The cases
(tests/demap_cases.py): m = 2 ... 10 / 1 ... 10, app and maxlog, hard output, 1 / 255 / 256 / 257 / 1000 symbols, y on points, midway
between levels, on an axis, far outside, random; no scalar, spanning 1e-4 ... 1e4, and per symbol with neighbours a factor 1e3 apart
(the square kernel fetches y and no one stride ahead); constructed gaps of 60 ... 120 between the axis maximum and a set's best
member (the switch of ``square_qam_llr`` to per-set maxima, and the exponentials the hardware exp2 returns as 0 below 2^-126);
no = 0; priors of 0, 1, 50 and - hard output only - 5000, [m] and [n, m].  The CPU side (tests/test_demap_host.py) shows on these
very inputs that the bound is neither too tight (NumPy models of both kernels inside it) nor too loose (eight seeded faults outside).

Every test prints its max |llr - anchor| / bound (run with -s); on failure the message carries the worst ratio and its index
(symbol, bit).

On an MI355X with ROCm's device library the largest ratios are those of the NumPy models to two digits: square kernel 0.04 ... 0.58
(sq8_app_midway_span), generic kernel 0.04 ... 0.70 (g1_app_pam_random), with a prior 0.07 ... 0.48; the constructed gap cases 0.38 and
0.34.  With the former switch of ``square_qam_llr`` at 80 the gap cases stood at 8.2 and 8.1 (LLR -79.56717 against -79.566837: a set's
second member returned as 0), and ``g4_app_no_zero`` returned NaN before the generic kernel's exponential was clamped."""
import numpy as np
import pytest

import demap_cases as dc
import demap_f32 as df

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _demapper(phy, case, pts, hard=False, separable=None):
    mp = phy.mapping
    if case.table in ("qam", "pam"):
        const = mp.Constellation(case.table, case.m)
    else:
        const = mp.Constellation("custom", case.m, points=pts)
    assert np.array_equal(_np(const.device_points(raw=True)), pts), "the table of the case is the table on the device"
    kw = {} if separable is None else {"separable": separable}
    return const, mp.Demapper(case.method, constellation=const, hard_out=hard, **kw)


def _run(phy, case, separable=None):
    """the kernel's soft output [n, m], anchor, bound and (where the case asks for it) the hard output"""
    mp = phy.mapping
    pts = dc.points(case, mp)
    y, no, prior = dc.inputs(case, mp)
    square = case.kernel == "square" if separable is None else separable
    const, dem = _demapper(phy, case, pts, separable=square)
    tab = pts
    if square:
        tab = df.levels_from_points(pts)
        assert np.array_equal(_np(const.pam_levels(raw=True)), tab), "the levels of the case are the levels on the device"
    args = (y.copy(), no.copy() if no.size > 1 else float(no[0])) + (() if prior is None else (prior.copy(),))       # (read-only inputs)
    out = _np(dem(*args))
    assert out.shape == (case.n * case.m,) and out.dtype == np.float32
    an = df.anchor(y, no, tab, case.method, prior)
    bd = df.bound(y, no, tab, case.method, prior)
    hard = None
    if case.hard:
        hard = _np(_demapper(phy, case, pts, hard=True, separable=square)[1](*args)).reshape(an.shape)
    return out.reshape(an.shape), an, bd, hard, y


def _hold(case, out, an, bd, what=""):
    q, at = df.ratio(out, an, bd)
    print(f"demap {case.name}{what}: max |llr - anchor| / bound = {q:.4f} at (symbol, bit) = {at}, |anchor| {abs(an[at]):.4g}, bound {bd[at]:.3g}")
    assert q <= 1, f"{case.name}{what}: worst |llr - anchor| / bound = {q:.3f} at (symbol, bit) = {at}: {out[at]!r} against {an[at]!r}"
    return q


@pytest.mark.parametrize("case", dc.ALL, ids=[c.name for c in dc.ALL])
def test_demapper_holds_the_bound(phy, case):
    out, an, bd, hard, y = _run(phy, case)
    _hold(case, out, an, bd)
    if case.pos == "midway" and case.prior is None:
        zero = np.abs(an) <= 1e-13 * np.abs(an).max()
        assert zero[: min(2, case.n)].any(), "y = 0: the sign bits' LLRs are 0 by symmetry"
        assert np.all(np.abs(out[zero]) <= bd[zero])
    if hard is not None:
        sure = np.abs(an) > bd
        assert sure.any() and set(np.unique(hard)) <= {0.0, 1.0}
        assert np.array_equal(hard[sure], (an > 0).astype(np.float32)[sure])


SQUARE_BOTH = [c for c in dc.SQUARE if c.table == "qam" and not c.hard and c.name not in
               ("sq10_app_points", "sq10_app_random_alt", "sq10_max_far30")] + [dc.BY_NAME["sq10_app_random_alt"]]


@pytest.mark.parametrize("case", SQUARE_BOTH, ids=[c.name for c in SQUARE_BOTH])
def test_generic_kernel_on_the_square_cases(phy, case):
    """``separable=False`` on the inputs of the square kernel's cases: the generic kernel meets ITS bound there (and
    ``g4_app_qam_gap`` & co. above run the other direction's inputs)"""
    out, an, bd, _, _ = _run(phy, case, separable=False)
    _hold(case, out, an, bd, " separable=False")


def test_default_path_of_a_qam_demapper_is_the_square_kernel(phy):
    """``Demapper("app", "qam", m)`` without ``separable`` takes the per-axis kernel: its output equals ``separable=True``'s bit
    for bit and differs from ``separable=False``'s"""
    case = dc.BY_NAME["sq6_app_c2"]
    mp = phy.mapping
    y, no, _ = dc.inputs(case, mp)
    y = y.copy()
    a = _np(mp.Demapper("app", "qam", 6)(y, float(no[0])))
    b = _np(mp.Demapper("app", "qam", 6, separable=True)(y, float(no[0])))
    c = _np(mp.Demapper("app", "qam", 6, separable=False)(y, float(no[0])))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
