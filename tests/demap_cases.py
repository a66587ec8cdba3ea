"""Inputs of the demapper edge tests (tests/test_demap_host.py on the NumPy models, tests/test_gpu_demap_edges.py on the kernels): the
same float32 arrays for both.  Every case is one launch of at most 1000 symbols (one grid trip: tests/test_gpu_grid_stride.py has the
later trips) and keeps every exponent finite in float32 (d^2 / no < 1e30, asserted in ``inputs``).

table   "qam" (the square kernel, or the generic one with ``separable=False``), "pam", "rot" (qam or 8 points turned by 0.3 rad: a
        custom constellation, generic kernel), "tiny" (qam scaled by 1e-5, custom: with no = 0 the clamp to finfo.tiny still leaves
        d^2 / tiny = 2.7e28 finite)
pos     "points": y on every point in turn;  "midway": one coordinate exactly midway between two neighbouring levels (the first
        symbols: y = 0, where every axis' MSB is 0 by symmetry);  "axis": on the real or the imaginary axis;  "far3" / "far30": 3 and
        30 times the outermost level;  "random": points plus noise of variance no;  "gap": see ``gap_inputs``
no      a scalar;  "alt:a": per symbol a, 1000 a, a, ... - a neighbour's value (the square kernel fetches y and no one stride ahead)
        is off by 1e3;  "span": per symbol, log-uniform over 1e-4 ... 1e4;  "zero": 0
prior   None;  ("vec", a): [m], +-a alternating;  ("mat", a): [n, m], +-a with random signs;  ("rand", a): [n, m] normal times a
"""
from collections import namedtuple

import numpy as np

import demap_f32 as df

Case = namedtuple("Case", "name kernel table m method hard n pos no prior")
SEED = 7
GAPS = (60, 70, 75, 79.5, 80.5, 85, 90, 120)
DELTAS = (1, 4, 7.3, 8, 12)       # 8: with gap 79.5 the first second member past the flush point 126 ln 2 = 87.34 (7.3 stops at 86.8)


def _c(name, kernel, table, m, method, n, pos, no, prior=None, hard=False):
    return Case(name, kernel, table, m, method, hard, n, pos, no, prior)


SQUARE = [
    _c("sq2_app_points_n1", "square", "qam", 2, "app", 1, "points", 0.5),
    _c("sq2_max_random_alt", "square", "qam", 2, "maxlog", 255, "random", "alt:1e-3"),
    _c("sq4_app_points", "square", "qam", 4, "app", 256, "points", 1e-2),
    _c("sq4_app_midway", "square", "qam", 4, "app", 257, "midway", 0.05),
    _c("sq4_max_midway", "square", "qam", 4, "maxlog", 257, "midway", 1e-4),
    _c("sq4_app_random_alt", "square", "qam", 4, "app", 1000, "random", "alt:1e-3"),
    _c("sq4_app_far30", "square", "qam", 4, "app", 255, "far30", "span"),
    _c("sq4_app_gap", "square", "qam", 4, "app", 160, "gap", "gap"),
    _c("sq6_app_c2", "square", "qam", 6, "app", 1000, "random", 0.05),
    _c("sq6_app_points_small_no", "square", "qam", 6, "app", 257, "points", 1e-4),
    _c("sq6_app_axis_span", "square", "qam", 6, "app", 256, "axis", "span"),
    _c("sq6_max_far3_alt", "square", "qam", 6, "maxlog", 255, "far3", "alt:1e-1"),
    _c("sq6_app_random_alt", "square", "qam", 6, "app", 1000, "random", "alt:1e-2"),
    _c("sq6_app_gap", "square", "qam", 6, "app", 160, "gap", "gap"),
    _c("sq6_hard_random", "square", "qam", 6, "app", 257, "random", "alt:1e-2", hard=True),
    _c("sq6_app_big_no", "square", "qam", 6, "app", 255, "random", 1e4),
    _c("sq8_app_midway_span", "square", "qam", 8, "app", 256, "midway", "span"),
    _c("sq8_max_points", "square", "qam", 8, "maxlog", 256, "points", 1.0),
    _c("sq8_app_far3", "square", "qam", 8, "app", 255, "far3", 1e-2),
    _c("sq10_app_points", "square", "qam", 10, "app", 1000, "points", 1e-3),
    _c("sq10_app_random_alt", "square", "qam", 10, "app", 257, "random", "alt:1e-3"),
    _c("sq10_max_far30", "square", "qam", 10, "maxlog", 255, "far30", "span"),
    _c("sq10_hard_midway", "square", "qam", 10, "maxlog", 256, "midway", 0.05, hard=True),
    _c("sq4_app_no_zero", "square", "tiny", 4, "app", 256, "points", "zero"),
    _c("sq4_max_no_zero", "square", "tiny", 4, "maxlog", 255, "points", "zero"),
]

GENERIC = [
    _c("g1_app_pam_random", "generic", "pam", 1, "app", 257, "random", "alt:1e-2"),
    _c("g1_max_pam_points_n1", "generic", "pam", 1, "maxlog", 1, "points", 1e-4),
    _c("g2_app_qam_random", "generic", "qam", 2, "app", 1000, "random", "span"),
    _c("g2_app_pam_midway", "generic", "pam", 2, "app", 255, "midway", 0.05),
    _c("g3_app_pam_far30", "generic", "pam", 3, "app", 256, "far30", "alt:1e-3"),
    _c("g3_app_rot_random", "generic", "rot", 3, "app", 257, "random", "alt:1e-2"),
    _c("g3_max_rot_points", "generic", "rot", 3, "maxlog", 255, "points", 1e4),
    _c("g4_app_qam_midway", "generic", "qam", 4, "app", 257, "midway", 0.05),
    _c("g4_app_qam_gap", "generic", "qam", 4, "app", 160, "gap", "gap"),
    _c("g4_app_rot_axis", "generic", "rot", 4, "app", 256, "axis", "span"),
    _c("g4_hard_rot_random", "generic", "rot", 4, "app", 255, "random", "alt:1e-2", hard=True),
    _c("g4_app_no_zero", "generic", "tiny", 4, "app", 256, "points", "zero"),
    _c("g6_app_qam_c2", "generic", "qam", 6, "app", 1000, "random", 0.05),
    _c("g6_max_qam_far3", "generic", "qam", 6, "maxlog", 255, "far3", "alt:1e-1"),
    _c("g6_app_qam_points", "generic", "qam", 6, "app", 256, "points", 1e-4),
    _c("g8_app_qam_random", "generic", "qam", 8, "app", 257, "random", "alt:1e-3"),
    _c("g8_max_qam_midway", "generic", "qam", 8, "maxlog", 256, "midway", 1.0),
    _c("g10_app_qam_random", "generic", "qam", 10, "app", 255, "random", "alt:1e-3"),
    _c("g10_max_qam_points", "generic", "qam", 10, "maxlog", 1000, "points", "span"),
]

PRIOR = [
    _c("p1_app_zero", "generic", "pam", 1, "app", 255, "random", 0.5, ("vec", 0.0)),
    _c("p2_app_vec1", "generic", "qam", 2, "app", 257, "random", "alt:1e-2", ("vec", 1.0)),
    _c("p2_max_mat50", "generic", "qam", 2, "maxlog", 256, "points", "span", ("mat", 50.0)),
    _c("p3_app_mat1", "generic", "rot", 3, "app", 1000, "random", "alt:1e-2", ("mat", 1.0)),
    _c("p4_app_vec50", "generic", "qam", 4, "app", 256, "random", 0.05, ("vec", 50.0)),
    _c("p4_app_rand_midway", "generic", "qam", 4, "app", 255, "midway", "alt:1e-2", ("rand", 3.0)),
    _c("p4_hard_vec5000", "generic", "qam", 4, "app", 257, "random", 0.05, ("vec", 5000.0), True),
    _c("p6_app_mat50", "generic", "qam", 6, "app", 257, "random", "span", ("mat", 50.0)),
    _c("p6_hard_mat5000", "generic", "qam", 6, "maxlog", 255, "far3", "alt:1e-2", ("mat", 5000.0), True),
    _c("p6_max_zero_mat", "generic", "qam", 6, "maxlog", 256, "axis", 1e-2, ("mat", 0.0)),
    _c("p8_app_rand", "generic", "qam", 8, "app", 255, "random", "alt:1e-2", ("rand", 3.0)),
    _c("p10_app_vec1", "generic", "qam", 10, "app", 255, "random", 0.05, ("vec", 1.0)),
]

ALL = SQUARE + GENERIC + PRIOR
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)


def points(case, mapping):
    """complex64 points of the case's table; ``mapping``: the module with ``qam`` and ``pam`` (sionna_amd.phy.mapping)"""
    if case.table == "pam":
        return mapping.pam(case.m, precision="single").astype(np.complex64)
    if case.table == "rot" and case.m % 2:
        base = mapping.pam(case.m, precision="single") * (1 + 0.5j * (-1.0) ** np.arange(2 ** case.m))
    else:
        base = mapping.qam(case.m, precision="single")
    if case.table == "rot":
        return (base * np.exp(0.3j)).astype(np.complex64)
    if case.table == "tiny":
        return (base * 1e-5).astype(np.complex64)
    return base.astype(np.complex64)


def table(case, mapping):
    """what the C entry of the case's kernel receives: float32 levels (square) or complex64 points (generic)"""
    pts = points(case, mapping)
    if case.kernel == "square":
        lev = df.levels_from_points(pts)
        assert lev is not None, case.name
        return lev
    return pts


def gap_inputs(lev):
    """For every gap G of GAPS, every distance D of DELTAS, each axis and each sign: a symbol at +-eps on that axis - between the two
    innermost levels +-a, nearer to one - with no chosen so that the set {+-c} of the next-to-innermost pair (for NB = 2: the outer
    levels; they share one label bit that the inner levels do not have) has its best member exactly G below the axis maximum and
    its other member D below that:  (c - eps)^2 - (a - eps)^2 = G no,  4 c eps = D no.  The other coordinate sits on a level."""
    lev = np.sort(np.asarray(lev, np.float64))
    k = len(lev) // 2
    a, c = lev[k], lev[k + 1]
    y, no = [], []
    for g in GAPS:
        for d in DELTAS:
            r = d / g
            eps = r * (c * c - a * a) / (4 * c + 2 * r * (c - a))
            n0 = 4 * c * eps / d
            for ax in range(2):
                for sg in (1.0, -1.0):
                    other = lev[(len(y) * 5) % len(lev)]
                    y.append(complex(sg * eps, other) if ax == 0 else complex(other, sg * eps))
                    no.append(n0)
    return np.asarray(y, np.complex64), np.asarray(no, np.float32)


def inputs(case, mapping):
    """y [n] complex64, no float32 [1] or [n], prior None / float32 [m] / [n, m]"""
    rng = np.random.default_rng([SEED, sum(map(ord, case.name))])
    pts = points(case, mapping)
    n, m = case.n, case.m
    if case.pos == "gap":
        y, no = gap_inputs(df.levels_from_points(pts))
        assert y.size == n
    else:
        if case.no == "span":
            no = (10.0 ** rng.uniform(-4, 4, n)).astype(np.float32)
        elif case.no == "zero":
            no = np.zeros(1, np.float32)
        elif isinstance(case.no, str):
            a = float(case.no.split(":")[1])
            no = np.where(np.arange(n) % 2 == 0, a, 1e3 * a).astype(np.float32)
        else:
            no = np.full(1, case.no, np.float32)
        on = pts[np.arange(n) % len(pts)].astype(np.complex128)
        re_lev, im_lev = np.unique(pts.real.astype(np.float64)), np.unique(pts.imag.astype(np.float64))
        top = max(np.abs(pts.real).max(), np.abs(pts.imag).max())
        if case.pos == "points":
            y = on
        elif case.pos == "random":
            s = np.sqrt(np.broadcast_to(no, (n,)).astype(np.float64) / 2)
            y = on + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        elif case.pos == "axis":
            y = np.where(np.arange(n) % 2 == 0, on.real, 1j * on.imag)
        elif case.pos in ("far3", "far30"):
            f = 3.0 if case.pos == "far3" else 30.0
            y = f * top * np.exp(2j * np.pi * np.arange(n) / n) * (1 + 0.01 * rng.standard_normal(n))
            y[: min(4, n)] = (f * top * np.array([1, 1j, -1, -1j]))[: min(4, n)]
        elif case.pos == "midway":
            mid_re = (re_lev[:-1] + re_lev[1:]) / 2 if len(re_lev) > 1 else re_lev
            mid_im = (im_lev[:-1] + im_lev[1:]) / 2 if len(im_lev) > 1 else im_lev
            i = np.arange(n)
            y = np.where(i % 2 == 0, mid_re[(i // 2) % len(mid_re)] + 1j * on.imag, on.real + 1j * mid_im[(i // 2) % len(mid_im)])
            y[: min(2, n)] = 0
        else:
            raise AssertionError(case.pos)
        y = y.astype(np.complex64)
    prior = None
    if case.prior is not None:
        kind, a = case.prior
        if kind == "vec":
            prior = (a * (-1.0) ** np.arange(m)).astype(np.float32)
        elif kind == "mat":
            prior = (a * rng.choice([-1.0, 1.0], (n, m))).astype(np.float32)
        else:
            prior = (a * rng.standard_normal((n, m))).astype(np.float32)
    d2 = np.abs(y.astype(np.complex128)[:, None] - pts.astype(np.complex128)[None, :]) ** 2
    assert np.all(d2 / np.maximum(np.broadcast_to(no, (n,)).astype(np.float64), df.TINY)[:, None] < 1e30), case.name
    for x in (y, no) + (() if prior is None else (prior,)):
        x.setflags(write=False)
    return y, no, prior
