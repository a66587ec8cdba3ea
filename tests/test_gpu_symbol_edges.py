"""The symbol-domain mapping kernels of csrc/mapping.hip (float32) and csrc/f64_mapping.hip (float64) through
``phy.mapping.SymbolDemapper``, ``SymbolLogits2LLRs``, ``LLRs2SymbolLogits``, ``SymbolLogits2Moments`` and ``PAM2QAM`` in
precision "single" and "double", against the anchors of tests/symbol_f32.py on EVERY output, within the bound derived there from the
kernels' arithmetic (u = 2^-24; the float64 kernels within 2^-29 times that, against an anchor in the host's long double).  The cases
(tests/symbol_cases.py): m = 1 ... 10, 0 / 1 / 255 / 256 / 257 rows (63 ... 129 around the 64-row tile of ``llrs2logits_kernel``), y on
points, midway, at exact ties and 1e3 away, no from finfo.tiny to 1e4, priors with -inf; logits with one dominant member, a common
offset of +-1e6, constructed gaps of 80 ... 150, members at -1e10, -FLT_MAX and -inf and whole sets at -inf; LLRs of 0 ... +-inf;
variances down to 0.  Where the anchor is +-inf the output must equal it; NaN is allowed only where the anchor is NaN.  Hard outputs
equal the anchor's decision wherever its margin exceeds the bounds, and the first maximum on the constructed exact ties.  The CPU side
(tests/test_symbol_host.py) shows on these very inputs that the bound is neither too tight nor too loose.

Every test prints its max |out - anchor| / bound (run with -s); on failure the message carries the worst ratio and its index.

On an MI355X with ROCm's device library the largest ratios over the 181 tests (single / double): SymbolDemapper 0.60 / 0.51
(sd10_hard_random), SymbolLogits2LLRs app 0.41 / 0.51 (l2l3_app_empty / l2l6_app_offset_p) and maxlog 0.99 / 0 (l2l3_max_normal: one
correctly rounded subtraction against u |llr| - the bound is attained by construction), LLRs2SymbolLogits 0.59 / 0.61
(l2s4_hard_normal), SymbolLogits2Moments 0.22 / 0.28 (mom3_c3_dom20; the dominant-logit variances 0.13 / 0.25), the round trip
0.14 / 0.13, PAM2QAM bit for bit.  Before ``logits2llrs_kernel`` clamped its exponential's argument and took a non-finite set maximum
as the reduction, l2l4_app_low_inf, l2l3_app_low_fltmax and l2l4_app_low_1e10 returned NaN in single precision (anchors -2.76, -3.33,
1.18), and l2l3_app_empty, l2l4_app_from_llrs and the round trip returned NaN in single AND double (anchor +-inf); the other 172 tests
passed unchanged."""
import numpy as np
import pytest

import symbol_cases as sc
import symbol_f32 as sf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _constellation(mp, case, pts, precision):
    if case.table in ("qam", "pam"):
        const = mp.Constellation(case.table, case.m, precision=precision)
    else:
        const = mp.Constellation("custom", case.m, points=pts, precision=precision)
    assert np.array_equal(np.asarray(const.points), pts), "the table of the case is the table of the block"
    return const


def run(phy, case, ex, precision, hard=False):
    """the block's outputs in the order of ``ex.anchors`` (hard: the decision), from writable copies of the float32 inputs"""
    mp, m = phy.mapping, case.m
    rt = np.float32 if precision == "single" else np.float64
    i = [None if x is None else x.astype(np.complex128 if np.iscomplexobj(x) and rt is np.float64 else (x.dtype if np.iscomplexobj(x) else rt))
         for x in ex.inputs]
    if case.op == "sd":
        blk = mp.SymbolDemapper(constellation=_constellation(mp, case, ex.pts, precision), hard_out=hard, precision=precision)
        no = i[1] if i[1].size > 1 else float(i[1][0])
        out = _np(blk(i[0], no) if i[2] is None else blk(i[0], no, i[2]))
        assert out.shape == ((case.n,) if hard else (case.n, 1 << m))
    elif case.op == "l2l":
        blk = mp.SymbolLogits2LLRs(case.method, m, hard_out=hard, precision=precision)
        out = _np(blk(i[0]) if i[1] is None else blk(i[0], i[1]))
        assert out.shape == (case.n, m)
    elif case.op == "l2s":
        out = _np(mp.LLRs2SymbolLogits(m, hard_out=hard, precision=precision)(i[0]))
        assert out.shape == ((case.n,) if hard else (case.n, 1 << m))
    elif case.op == "mom":
        mean, var = mp.SymbolLogits2Moments(constellation=_constellation(mp, case, ex.pts, precision), precision=precision)(i[0])
        mean, var = _np(mean), _np(var)
        assert mean.shape == var.shape == (case.n,) and var.dtype == rt
        return mean.real, mean.imag, var
    else:
        out = _np(mp.PAM2QAM(m, hard_in_out=False, precision=precision)(i[0], i[1]))
        assert out.shape == (case.n, 1 << m)
    if hard:
        return out
    assert out.dtype == rt
    return (out,)


def _hold(case, precision, outs, ex):
    q, at = sf.worst(outs, ex)
    k = at[0]
    if len(at) > 1:
        an, bd = np.asarray(ex.anchors[k], np.float64)[at[1:]], ex.bounds[k][at[1:]]
        print(f"symbol {case.name} {precision}: max |out - anchor| / bound = {q:.4f} at (output, row, ...) = {at}, anchor {an:.6g}, bound {bd:.3g}")
        assert q <= 1, f"{case.name} {precision}: worst |out - anchor| / bound = {q:.3f} at {at}: {np.asarray(outs[k]).reshape(ex.anchors[k].shape)[at[1:]]!r} against {an!r}"
    return q


@pytest.mark.parametrize("precision", ["single", "double"])
@pytest.mark.parametrize("case", sc.ALL, ids=[c.name for c in sc.ALL])
def test_block_holds_the_bound(phy, case, precision):
    ex = sc.expected(case, phy.mapping, precision)
    outs = run(phy, case, ex, precision)
    if case.op == "p2q":
        assert np.array_equal(outs[0], ex.anchors[0]), "one addition per entry: bit for bit"
    _hold(case, precision, outs, ex)
    if case.hard:
        hard = np.asarray(run(phy, case, ex, precision, hard=True), np.float64).reshape(ex.decision.shape)
        checked = ex.sure | (ex.tied if case.tie else False)
        assert checked.mean() >= 0.9 and (not case.tie or ex.tied.any())
        assert np.array_equal(hard[checked], ex.decision[checked]), np.flatnonzero((hard != ex.decision) & checked)[:8]


@pytest.mark.parametrize("precision", ["single", "double"])
def test_round_trip_returns_the_llrs(phy, precision):
    """LLRs2SymbolLogits -> SymbolLogits2LLRs("app") returns the LLRs within the sum of both bounds, +-inf preserved"""
    case = sc.BY_NAME["l2s4_roundtrip"]
    ex = sc.expected(case, phy.mapping, precision)
    mp, m = phy.mapping, case.m
    rt = np.float32 if precision == "single" else np.float64
    llrs = ex.inputs[0].astype(rt)
    logits = mp.LLRs2SymbolLogits(m, precision=precision)(llrs)
    back = _np(mp.SymbolLogits2LLRs("app", m, precision=precision)(logits))
    q = sf.round_trip_ratio(ex.inputs[0], _np(logits), back, ex.bounds[0], m, scale=sf.F64_SCALE if precision == "double" else 1.0)
    print(f"symbol round trip {precision}: {q:.4f}")
    assert np.array_equal(np.isinf(back), np.isinf(llrs)) and q <= 1


def test_no_zero_is_what_the_reference_leaves_undefined(phy):
    """no = 0: the reference returns NaN on every output (tests/golden/symbol_edges_ref_golden.npz), so nothing is required of the
    values; the call itself is legal and returns"""
    case = sc.BY_NAME["sd4_qam_no_zero"]
    ex = sc.expected(case, phy.mapping)
    assert np.all(np.isnan(np.asarray(ex.anchors[0], np.float64)))
    assert run(phy, case, ex, "single")[0].shape == (case.n, 16)
