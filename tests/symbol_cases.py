"""Inputs of the symbol-domain edge tests (tests/test_symbol_host.py on the NumPy models and the oracle, tests/test_gpu_symbol_edges.py
on the kernels): the same float32 arrays for both.  Every case is one launch of at most 257 rows (64 where P = 1024; the element-wise
PAM2QAM alone runs 257 rows at P = 1024); later grid trips are tests/test_gpu_grid_stride.py's.  Every case is a legal call of a
public block.

op "sd" (SymbolDemapper)   table "qam" / "pam" / "c3" (a custom, un-normalised 3-bit table) / "tiny" (qam times 1e-5, custom: with
        no = finfo.tiny the exponents stay finite in float32);  pos "points", "midway" (rows 0, 1: y = 0, an exact four-way tie on QAM),
        "far" (|e| of 1e6), "random" ("random0": the first eight rows at y = 0);  no: a scalar, "span" (per symbol, log-uniform 1e-4 ... 1e4), "tiny", "zero" (the reference
        returns NaN there: nothing is held, the case records it);  prior None, ("vec", a) [P], ("mat", a) [n, P] normal times a,
        ("pm", a) [n, P] +-a, ("inf",) [n, P] normal with -inf on some but never all points
op "l2l" (SymbolLogits2LLRs)   kind "normal" (times 5), ("dom", g) one logit g above the rest, "equal", ("offset", +-1e6), "gaps" (a set's
        other members 80 ... 120 and 150 below its maximum), ("low", v) members at v = -1e10 / -FLT_MAX / -inf, "empty" (one whole set at
        -inf), "from_llrs" (the logits LLRs2SymbolLogits gives for LLRs of +-inf, +-104, +-20);  prior None, ("vec", a) [m] +-a
        alternating, ("mat", a) [n, m] +-a random signs, ("rand", a) normal times a
op "l2s" (LLRs2SymbolLogits)   kind ("const", a): +-a with random signs (a = 0: all 0, every point tied), "normal", "mixed" (every listed
        magnitude 0, 1e-3, 20, 88, 104, 1e4, inf in one row set), "roundtrip" (through SymbolLogits2LLRs("app") and back)
op "mom" (SymbolLogits2Moments)   kind "uniform", ("dom", g), "two" (two equal dominant points), "offset" (1e6 on every logit), "low"
        (-inf members), "normal"
op "p2q" (PAM2QAM, logits)   m = 2 nbh
"""
from collections import namedtuple

import numpy as np

import symbol_f32 as sf

Case = namedtuple("Case", "name op m n kind table no prior method hard tie")
SEED = 11
FLT_MAX = float(np.finfo(np.float32).max)
GAPS = (80.0, 87.0, 88.0, 95.0, 103.0, 104.5, 120.0, 150.0)


def _c(name, op, m, n, kind, table=None, no=None, prior=None, method=None, hard=False, tie=False):
    return Case(name, op, m, n, kind, table, no, prior, method, hard, tie)


SD = [
    _c("sd1_pam_points_n1", "sd", 1, 1, "points", "pam", 0.5),
    _c("sd2_qam_random_span", "sd", 2, 255, "random", "qam", "span"),
    _c("sd2_qam_rows0", "sd", 2, 0, "random", "qam", 1.0),
    _c("sd2_qam_big_no", "sd", 2, 256, "random", "qam", 1e4),
    _c("sd3_c3_random", "sd", 3, 256, "random", "c3", 0.1),
    _c("sd3_pam_far", "sd", 3, 257, "far", "pam", 1.0),
    _c("sd4_qam_midway", "sd", 4, 257, "midway", "qam", 0.05),
    _c("sd4_qam_far", "sd", 4, 255, "far", "qam", 1.0),
    _c("sd4_qam_small_no", "sd", 4, 256, "random", "qam", 1e-4),
    _c("sd4_tiny_no_tiny", "sd", 4, 256, "points", "tiny", "tiny"),
    _c("sd4_qam_no_zero", "sd", 4, 32, "midway", "qam", "zero"),
    _c("sd6_qam_random_span", "sd", 6, 257, "random", "qam", "span"),
    _c("sd8_qam_points", "sd", 8, 256, "points", "qam", 1e-4),
    _c("sd10_qam_random", "sd", 10, 64, "random", "qam", 0.05),
    _c("sd4_prior_vec", "sd", 4, 257, "random", "qam", 0.05, ("vec", 2.0)),
    _c("sd6_prior_pm50", "sd", 6, 255, "random", "qam", "span", ("pm", 50.0)),
    _c("sd3_c3_prior_mat", "sd", 3, 256, "random", "c3", 0.5, ("mat", 2.0)),
    _c("sd4_prior_inf", "sd", 4, 257, "random", "qam", 0.1, ("inf",)),
    _c("sd4_hard_ties", "sd", 4, 257, "random0", "qam", 0.02, hard=True, tie=True),
    _c("sd6_hard_random", "sd", 6, 255, "random", "qam", 0.01, hard=True),
    _c("sd3_hard_c3_prior", "sd", 3, 63, "random", "c3", 0.05, ("mat", 1.0), hard=True),
    _c("sd10_hard_random", "sd", 10, 64, "random", "qam", 1e-3, hard=True),
]

L2L = [
    _c("l2l1_app_normal_n1", "l2l", 1, 1, "normal", method="app"),
    _c("l2l2_app_normal", "l2l", 2, 255, "normal", method="app"),
    _c("l2l2_app_rows0", "l2l", 2, 0, "normal", method="app"),
    _c("l2l3_max_normal", "l2l", 3, 256, "normal", method="maxlog"),
    _c("l2l4_app_dom100", "l2l", 4, 257, ("dom", 100.0), method="app"),
    _c("l2l6_app_dom1e4", "l2l", 6, 255, ("dom", 1e4), method="app"),
    _c("l2l4_app_equal", "l2l", 4, 256, "equal", method="app", hard=True, tie=True),
    _c("l2l6_app_offset_p", "l2l", 6, 257, ("offset", 1e6), method="app"),
    _c("l2l3_max_offset_m", "l2l", 3, 255, ("offset", -1e6), method="maxlog"),
    _c("l2l2_app_gaps", "l2l", 2, 256, "gaps", method="app"),
    _c("l2l4_app_gaps", "l2l", 4, 256, "gaps", method="app"),
    _c("l2l4_app_low_1e10", "l2l", 4, 257, ("low", -1e10), method="app"),
    _c("l2l3_app_low_fltmax", "l2l", 3, 255, ("low", -FLT_MAX), method="app"),
    _c("l2l4_app_low_inf", "l2l", 4, 256, ("low", -np.inf), method="app"),
    _c("l2l6_max_low_inf", "l2l", 6, 257, ("low", -np.inf), method="maxlog"),
    _c("l2l3_app_empty", "l2l", 3, 256, "empty", method="app"),
    _c("l2l3_max_empty", "l2l", 3, 255, "empty", method="maxlog"),
    _c("l2l4_app_from_llrs", "l2l", 4, 257, "from_llrs", method="app"),
    _c("l2l8_app_normal", "l2l", 8, 257, "normal", method="app"),
    _c("l2l8_max_dom100", "l2l", 8, 255, ("dom", 100.0), method="maxlog"),
    _c("l2l2_app_prior_zero", "l2l", 2, 256, "normal", prior=("vec", 0.0), method="app"),
    _c("l2l4_app_prior_vec1", "l2l", 4, 257, "normal", prior=("vec", 1.0), method="app"),
    _c("l2l4_max_prior_mat50", "l2l", 4, 255, "normal", prior=("mat", 50.0), method="maxlog"),
    _c("l2l6_app_prior_mat50", "l2l", 6, 256, "normal", prior=("mat", 50.0), method="app"),
    _c("l2l3_app_prior_rand", "l2l", 3, 257, ("dom", 100.0), prior=("rand", 3.0), method="app"),
    _c("l2l4_hard_prior_vec5000", "l2l", 4, 257, "normal", prior=("vec", 5000.0), method="app", hard=True),
    _c("l2l6_hard_prior_mat5000", "l2l", 6, 255, "normal", prior=("mat", 5000.0), method="maxlog", hard=True),
    _c("l2l6_hard_normal", "l2l", 6, 256, "normal", method="app", hard=True),
]

L2S = [
    _c("l2s1_normal_n1", "l2s", 1, 1, "normal"),
    _c("l2s2_zero", "l2s", 2, 63, ("const", 0.0), hard=True, tie=True),
    _c("l2s2_rows0", "l2s", 2, 0, "normal"),
    _c("l2s3_small", "l2s", 3, 64, ("const", 1e-3)),
    _c("l2s4_c20", "l2s", 4, 65, ("const", 20.0)),
    _c("l2s4_c88", "l2s", 4, 129, ("const", 88.0)),
    _c("l2s6_c104", "l2s", 6, 63, ("const", 104.0)),
    _c("l2s6_c1e4", "l2s", 6, 64, ("const", 1e4)),
    _c("l2s3_inf", "l2s", 3, 65, ("const", np.inf)),
    _c("l2s8_mixed", "l2s", 8, 129, "mixed"),
    _c("l2s8_normal", "l2s", 8, 65, "normal"),
    _c("l2s4_hard_normal", "l2s", 4, 129, "normal", hard=True),
    _c("l2s8_hard_mixed", "l2s", 8, 65, "mixed", hard=True),
    _c("l2s4_roundtrip", "l2s", 4, 129, "roundtrip"),
]

MOM = [
    _c("mom1_pam_normal_n1", "mom", 1, 1, "normal", "pam"),
    _c("mom2_qam_uniform", "mom", 2, 255, "uniform", "qam"),
    _c("mom2_qam_rows0", "mom", 2, 0, "normal", "qam"),
    _c("mom3_c3_normal", "mom", 3, 256, "normal", "c3"),
    _c("mom4_qam_dom20", "mom", 4, 257, ("dom", 20.0), "qam"),
    _c("mom4_qam_dom100", "mom", 4, 255, ("dom", 100.0), "qam"),
    _c("mom6_qam_dom1e4", "mom", 6, 256, ("dom", 1e4), "qam"),
    _c("mom3_c3_dom20", "mom", 3, 257, ("dom", 20.0), "c3"),
    _c("mom4_qam_two", "mom", 4, 256, "two", "qam"),
    _c("mom6_qam_offset", "mom", 6, 255, "offset", "qam"),
    _c("mom4_qam_low", "mom", 4, 257, "low", "qam"),
    _c("mom8_qam_normal", "mom", 8, 256, "normal", "qam"),
    _c("mom3_pam_uniform", "mom", 3, 257, "uniform", "pam"),
    _c("mom10_qam_normal", "mom", 10, 64, "normal", "qam"),
]

P2Q = [_c(f"p2q{2 * nbh}_n{n}", "p2q", 2 * nbh, n, "normal") for nbh in (1, 2, 3, 4, 5) for n in (1, 257)] + [_c("p2q4_rows0", "p2q", 4, 0, "normal")]

ALL = SD + L2L + L2S + MOM + P2Q
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

C3 = np.array([2 + 1j, -1 + 2.5j, 0.5 - 0.25j, -3 - 1j, 1.5 + 3j, -0.75 - 2j, 3 - 2j, -2 + 0.5j], np.complex64)


def points(case, mapping, precision="single"):
    """the table of the case as the block of that precision holds it: complex64, or complex128 for precision="double" (qam / pam are
    then computed in double; the custom tables are the same values)"""
    ct = np.complex64 if precision == "single" else np.complex128
    if case.table == "pam":
        return np.asarray(mapping.pam(case.m, precision=precision)).astype(ct)
    if case.table == "c3":
        return C3.astype(ct)
    base = np.asarray(mapping.qam(case.m, precision=precision)).astype(ct)
    if case.table == "tiny":
        return (mapping.qam(case.m, precision="single") * 1e-5).astype(np.complex64).astype(ct)
    return base


def _rng(case):
    return np.random.default_rng([SEED, sum(map(ord, case.name))])


def _freeze(*xs):
    for x in xs:
        if x is not None:
            x.setflags(write=False)
    return xs


def sd_inputs(case, mapping):
    """y [n] complex64, no float32 [1] or [n], prior None / float32 [P] / [n, P]"""
    rng = _rng(case)
    pts = points(case, mapping).astype(np.complex128)
    n, P = case.n, 1 << case.m
    if case.no == "span":
        no = (10.0 ** rng.uniform(-4, 4, n)).astype(np.float32)
    elif case.no == "tiny":
        no = np.full(1, np.finfo(np.float32).tiny, np.float32)
    elif case.no == "zero":
        no = np.zeros(1, np.float32)
    else:
        no = np.full(1, case.no, np.float32)
    on = pts[np.arange(n) % P]
    if case.kind == "points":
        y = on
    elif case.kind in ("random", "random0"):
        s = np.sqrt(np.broadcast_to(no, (n,)).astype(np.float64) / 2)
        y = on + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        if case.kind == "random0":
            y[: min(8, n)] = 0                                 # exact four-way ties of the innermost points
    elif case.kind == "far":
        top = np.abs(pts).max()
        y = 1e3 * top * np.exp(2j * np.pi * (np.arange(n) + 0.37) / max(n, 1)) * (1 + 0.01 * rng.standard_normal(n))
    elif case.kind == "midway":
        re_lev, im_lev = np.unique(pts.real), np.unique(pts.imag)
        mid_re, mid_im = (re_lev[:-1] + re_lev[1:]) / 2, (im_lev[:-1] + im_lev[1:]) / 2
        i = np.arange(n)
        y = np.where(i % 2 == 0, mid_re[(i // 2) % len(mid_re)] + 1j * on.imag, on.real + 1j * mid_im[(i // 2) % len(mid_im)])
        y[: min(2, n)] = 0
    else:
        raise AssertionError(case.kind)
    y = y.astype(np.complex64)
    prior = None
    if case.prior is not None:
        kind = case.prior[0]
        if kind == "vec":
            prior = (case.prior[1] * rng.standard_normal(P)).astype(np.float32)
        elif kind == "mat":
            prior = (case.prior[1] * rng.standard_normal((n, P))).astype(np.float32)
        elif kind == "pm":
            prior = (case.prior[1] * rng.choice([-1.0, 1.0], (n, P))).astype(np.float32)
        else:
            prior = rng.standard_normal((n, P)).astype(np.float32)
            prior[rng.random((n, P)) < 0.3] = -np.inf
            prior[np.arange(n), rng.integers(0, P, n)] = 0.25          # never every point
            prior[0, 1:] = -np.inf                                       # one row with a single admissible point
    if case.no != "zero" and n:
        d2 = np.abs(y.astype(np.complex128)[:, None] - pts[None, :]) ** 2
        assert np.all(d2 / np.broadcast_to(no, (n,)).astype(np.float64)[:, None] < 1e30), case.name
    return _freeze(y, no, prior)


def _bit_prior(case, rng, n, m):
    if case.prior is None:
        return None
    kind, a = case.prior
    if kind == "vec":
        return (a * (-1.0) ** np.arange(m)).astype(np.float32)
    if kind == "mat":
        return (a * rng.choice([-1.0, 1.0], (n, m))).astype(np.float32)
    return (a * rng.standard_normal((n, m))).astype(np.float32)


def l2l_inputs(case):
    """logits [n, 2^m] float32, prior None / [m] / [n, m]"""
    rng = _rng(case)
    n, m = case.n, case.m
    P = 1 << m
    lab = sf.label_bits(m)
    z = (5 * rng.standard_normal((n, P))).astype(np.float32)
    kind = case.kind if isinstance(case.kind, str) else case.kind[0]
    rows = np.arange(n)
    if kind == "dom":
        z = rng.standard_normal((n, P)).astype(np.float32)
        z[rows, rows % P] += np.float32(case.kind[1])
    elif kind == "equal":
        z = np.broadcast_to((rows % 7 - 3.0).astype(np.float32)[:, None], (n, P)).copy()
    elif kind == "offset":
        z = (z.astype(np.float64) + case.kind[1]).astype(np.float32)
    elif kind == "gaps":
        # bit i = row % m, value b = (row // m) % 2: the set {c: bit i of c = b} has its maximum at 0 (on point k) and every other
        # member exactly G or G + 1 below; the complementary set stays normal-sized
        for r in range(n):
            i, b, g = r % m, (r // m) % 2, GAPS[(r // (2 * m)) % len(GAPS)]
            sel = np.flatnonzero(lab[:, i] == b)
            z[r, sel] = -np.float32(g) - (np.arange(len(sel)) % 2).astype(np.float32)
            z[r, sel[r % len(sel)]] = 0
    elif kind == "low":
        z[rng.random((n, P)) < 0.4] = np.float32(case.kind[1])
        for r in range(n):                                   # every set of every bit keeps a finite member: points 0 and P - 1
            z[r, 0], z[r, P - 1] = np.float32(rng.standard_normal()), np.float32(rng.standard_normal())
    elif kind == "empty":
        for r in range(n):
            i, b = r % m, (r // m) % 2
            z[r, lab[:, i] == b] = -np.inf
    elif kind == "from_llrs":
        vals = np.array([np.inf, -np.inf, 104.0, -104.0, 20.0, -20.0, 1.5, -0.5, 0.0])
        llrs = vals[rng.integers(0, len(vals), (n, m))]
        llrs[rows, rows % m] = np.where(rows % 2 == 0, np.inf, -np.inf)         # at least one certain bit per row
        z = sf.anchor_llrs2logits(llrs.astype(np.float32), m).astype(np.float32)
    else:
        assert kind == "normal", case.kind
    return _freeze(z, _bit_prior(case, rng, n, m))


def l2s_inputs(case):
    """LLRs [n, m] float32"""
    rng = _rng(case)
    n, m = case.n, case.m
    kind = case.kind if isinstance(case.kind, str) else case.kind[0]
    if kind == "const":
        l = case.kind[1] * rng.choice([-1.0, 1.0], (n, m))
    elif kind == "mixed":
        vals = np.array([0.0, 1e-3, 20.0, 88.0, 104.0, 1e4, np.inf, 3.0, 0.7])
        l = vals[rng.integers(0, len(vals), (n, m))] * rng.choice([-1.0, 1.0], (n, m))
        if case.hard:                                         # (an LLR of 0 ties two points: the decided rows carry none)
            l = np.where(l == 0, 1e-3, l)
    elif kind == "roundtrip":
        vals = np.array([np.inf, -np.inf, 20.0, -3.0, 0.5, 0.0, -88.0])
        l = vals[rng.integers(0, len(vals), (n, m))] + 0.0
    else:
        l = 5 * rng.standard_normal((n, m))
    return _freeze(np.asarray(l, np.float32))


def mom_inputs(case):
    """logits [n, 2^m] float32"""
    rng = _rng(case)
    n, P = case.n, 1 << case.m
    rows = np.arange(n)
    kind = case.kind if isinstance(case.kind, str) else case.kind[0]
    z = (3 * rng.standard_normal((n, P))).astype(np.float32)
    if kind == "uniform":
        z = np.broadcast_to((rows % 5 - 2.0).astype(np.float32)[:, None], (n, P)).copy()
    elif kind == "dom":
        z = rng.standard_normal((n, P)).astype(np.float32)
        z[rows, rows % P] += np.float32(case.kind[1])
    elif kind == "two":
        z = rng.standard_normal((n, P)).astype(np.float32)
        z[rows, rows % P] = 30
        z[rows, (rows * 5 + 3) % P] = 30
    elif kind == "offset":
        z = (z.astype(np.float64) + 1e6).astype(np.float32)
    elif kind == "low":
        z[rng.random((n, P)) < 0.5] = -np.inf
        z[rows, rows % P] = 1.0
    else:
        assert kind == "normal", case.kind
    return _freeze(z)


def p2q_inputs(case):
    rng = _rng(case)
    P = 1 << (case.m // 2)
    return _freeze((2 * rng.standard_normal((case.n, P))).astype(np.float32), (2 * rng.standard_normal((case.n, P))).astype(np.float32))


# ------------------------------------------------------------------ what a case requires
Expected = namedtuple("Expected", "inputs pts anchors bounds decision sure tied")


def expected(case, mapping, precision="single"):
    """inputs (float32, read-only), the table, the anchors and bounds of the case's soft outputs (tuples: one entry, or Re mean,
    Im mean, var) and - hard cases - the anchor's decision, the rows (outputs) on which it is certain (its margin exceeds the bounds
    of the two values compared) and those that are exact ties of the anchor (decided as the first maximum / as 0).
    precision "double": the anchor in the host's long double, the bound 2^-29 times the float32 one"""
    dbl = precision == "double"
    wide = sf.WIDE if dbl else np.float64
    scale = sf.F64_SCALE if dbl else 1.0
    m = case.m
    pts = decision = sure = tied = None
    if case.op == "sd":
        pts = points(case, mapping, precision)
        y, no, prior = inp = sd_inputs(case, mapping)
        an = (sf.anchor_symbol_demap(y, no, pts, prior, wide=wide),)
        bd = (sf.bound_symbol_demap(y, no, pts, prior) * scale,)
        if case.hard:
            e, de = sf.sd_exponents(y, no, pts, prior, wide=np.float64, with_error=True)
            decision, sure = sf.first_argmax(e), sf.sure_argmax(e, de * scale)
            tied = np.sort(e, axis=-1)[:, -1] == np.sort(e, axis=-1)[:, -2]
    elif case.op == "l2l":
        z, prior = inp = l2l_inputs(case)
        an = (sf.anchor_logits2llrs(z, m, case.method, prior, wide=wide),)
        bd = (sf.bound_logits2llrs(z, m, case.method, prior) * scale,)
        if case.hard:
            a = np.asarray(an[0], np.float64)
            decision, sure, tied = (a > 0).astype(np.float64), np.abs(a) > bd[0], a == 0
    elif case.op == "l2s":
        (l,) = inp = l2s_inputs(case)
        an = (sf.anchor_llrs2logits(l, m, wide=wide),)
        bd = (sf.bound_llrs2logits(l, m) * scale,)
        if case.hard:
            a = np.asarray(an[0], np.float64)
            decision, sure = sf.first_argmax(a), sf.sure_argmax(a, bd[0])
            tied = np.sort(a, axis=-1)[:, -1] == np.sort(a, axis=-1)[:, -2]
    elif case.op == "mom":
        pts = points(case, mapping, precision)
        (z,) = inp = mom_inputs(case)
        an = sf.anchor_moments(z, pts, wide=wide)
        bd = tuple(b * scale for b in sf.bound_moments(z, pts))
    else:
        a, b = inp = p2q_inputs(case)
        an = (sf.anchor_pam2qam(a, b, m // 2, np.float64 if dbl else np.float32),)
        bd = (np.zeros(an[0].shape),)
    return Expected(inp, pts, an, bd, decision, sure, tied)
