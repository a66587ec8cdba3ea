"""CPU side of the time-domain channel bound (tests/time_channel_f32.py): the NumPy float32 restatements of
``cir_to_time_kernel`` and ``apply_time_kernel`` (tests/kernel_models.py: summation order and LDS index arithmetic) on every named
case of tests/time_channel_cases.py.

- the bound is not too tight: every restatement stays at ratio <= 1 on EVERY output, normalize off / on / deferred;
- the bound is not too loose: each seeded fault of a restatement (a tail tile reading the previous tile's weight, a stage stride
  of L - 1 or L + 1, a partial pass one row short, tau of the neighbouring transmitter, an unpadded sinc table, the mean taken
  over L as well, a tap window off by one at either end, x read one sample late, the scale of the other transmitter) leaves it on
  at least one named case;
- the anchor is the reference's: the reference-executed fixture (all four tags, both ``normalize`` values, and the received signal)
  lies within bound + its own float32 storage rounding of the anchor.

How the bound compares with the tolerances it replaces, np.allclose(rtol=1e-4, atol=2e-5) for cir_to_time_channel and rtol = atol
= 1e-4 for ApplyTimeChannel, per output as bound / (atol + rtol |anchor|), median and largest over a case:
- L*, T*, ant*, P1, P2, zero, tau0 (|tau W| <= 8, up to 3 paths), unnormalised: bound 2.6e-7 ... 4.6e-7 in the median, at most 4e-6:
  0.012 ... 0.017 of the old tolerance in the median, at most 0.084 - the old test was 12 to 80 times looser;
- the same normalised: 0.014 ... 0.1 in the median; the largest reach 0.97 (L8), 1.1 (T1), 2.4 (T513) and 6.7 (L1, a window of one
  lag 6 ... 14 lags before the delays: weights near the zeros of the sinc, a link energy that small errors move) - where the
  link is badly conditioned the honest figure is above the old tolerance;
- P = 23: 0.07 median, 0.30 at most; tdl (|tau W| up to 92): 0.09 / 0.30; tauint 0.025 / 0.16;
- lds801 (801 paths, there for the LDS limit): 5.1 / 36 - gamma(802) is far above what the old tolerance allowed;
- ApplyTimeChannel: 0.0015 (1 x 8) ... 0.12 (the Tout >= 255 cases) in the median, at most 0.43.
A statement, not an assertion."""
import os

import numpy as np
import pytest

from tests import kernel_models as km
from tests import time_channel_cases as tcc
from tests import time_channel_f32 as tcf

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ofdm_time_ref_golden.npz")
MODES = ("off", "on", "deferred")


@pytest.fixture(scope="module")
def cir():
    """inputs, anchors and bounds of a case, computed once and shared (read-only)"""
    cache = {}

    def get(name):
        if name not in cache:
            w, a, tau, l_min, l_max = tcc.make_cir(tcc.CIR_BY_NAME[name])
            args = (w, a, tau, l_min, l_max)
            d = dict(args=args)
            for norm in (False, True):
                d[norm] = (tcf.anchor_cir(*args, norm), tcf.bound_cir(*args, norm))
            d["scale"] = (tcf.anchor_scale(*args), tcf.bound_scale(*args))
            for v in (a, tau) + d[False] + d[True] + d["scale"]:
                v.setflags(write=False)
            cache[name] = d
        return cache[name]
    return get


def _cir_ratio(d, mode, mutation=None):
    """the largest ratio over everything the mode returns (h, and the scale when deferred)"""
    if mode == "deferred":
        h, s = km.c2t_model_f32(*d["args"], True, defer=True, mutation=mutation)
        return max(tcf.ratio(h, *d[False]), tcf.ratio(s, *d["scale"]))
    norm = mode == "on"
    return tcf.ratio(km.c2t_model_f32(*d["args"], norm, mutation=mutation), *d[norm])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c.name for c in tcc.CIR])
def test_cir_to_time_model_inside_the_bound(cir, name, mode):
    q = _cir_ratio(cir(name), mode)
    assert q <= 1.0, (name, mode, q)


@pytest.mark.parametrize("mutation", km.C2T_MUTATIONS)
def test_cir_to_time_seeded_faults_leave_the_bound(cir, mutation):
    mode = "on" if mutation == "mean_over_l" else "off"
    killers = [c.name for c in tcc.CIR if c.p < 100 and _cir_ratio(cir(c.name), mode, mutation) > 1.0]
    print(f"{mutation}: caught by {killers}")
    assert killers, mutation


def test_cir_to_time_faults_are_caught_where_the_case_list_says(cir):
    """the cases that exist FOR a fault catch it: a tail tile at L = 10 and 19, the stage stride wherever L > 1 and more than one
    lane is live, the short pass at every T that is no multiple of 64, tau of the neighbour at every case with delays, the
    unpadded table at odd P L with a second link, the mean at every L > 1"""
    def caught(name, mutation, mode="off"):
        return _cir_ratio(cir(name), mode, mutation) > 1.0
    assert caught("L10", "tail_tile_prev_weight") and caught("L19", "tail_tile_prev_weight") and caught("L31", "tail_tile_prev_weight")
    assert not caught("L9", "tail_tile_prev_weight") and not caught("L18", "tail_tile_prev_weight")      # no tail tile there
    for name in ("L8", "L9", "T63", "T513", "ant2x2"):
        assert caught(name, "stage_stride_minus") and caught(name, "stage_stride_plus"), name
    for name in ("T1", "T63", "T65", "T255", "T257", "T513"):
        assert caught(name, "cnt_short_row"), name
    assert not caught("T64", "cnt_short_row") and not caught("T256", "cnt_short_row")                    # no partial pass there
    for name in ("L1", "T1", "P1xL9", "ant1x1", "tdl", "tauint"):
        assert caught(name, "tau_next_tx"), name
    assert caught("P23xL9", "table_unpadded") and caught("ant2x2", "table_unpadded")                     # 207 and 57 weights
    assert not caught("P23xL10", "table_unpadded") and not caught("P2xL9", "table_unpadded")             # even: nothing moves
    for name in ("L8", "T1", "ant2x2"):
        assert caught(name, "mean_over_l", "on"), name
    assert not caught("L1", "mean_over_l", "on")


def test_cir_bound_edges(cir):
    """a link without energy: anchor, bound, model and scale exactly 0 under normalisation; x == 0 exactly: the weight's own
    error term is 0 and the model returns the tap itself where one path sits on the lag"""
    d = cir("zero")
    b, rx, tx = tcc.ZERO_LINK
    ref, bd = d[True]
    assert np.all(ref[b, rx, :, tx] == 0) and np.all(bd[b, rx, :, tx] == 0) and np.all(np.isfinite(ref)) and np.all(np.isfinite(bd))
    assert d["scale"][0][b, rx, tx] == 0 and d["scale"][1][b, rx, tx] == 0
    h = km.c2t_model_f32(*d["args"], True)
    _, s = km.c2t_model_f32(*d["args"], True, defer=True)
    assert np.all(h[b, rx, :, tx] == 0) and s[b, rx, tx] == 0 and np.all(np.isfinite(h.view(np.float32)))
    live = np.ones(ref.shape, bool)
    live[b, rx, :, tx] = False
    assert np.all(bd[live] > 0) and np.all(np.abs(ref[live]) > 0)
    # tau = 0 with one path: h[..., l] = a at l = -l_min and the bound there is the product's rounding and the anchor term alone
    w, a, tau, l_min, l_max = cir("tau0")["args"]
    a1, tau1 = np.ascontiguousarray(a[..., :1, :]), np.ascontiguousarray(tau[..., :1])
    hz = km.c2t_model_f32(w, a1, tau1, l_min, l_max, False)
    assert np.array_equal(hz[..., -l_min], a1[:, :, :, :, :, 0, :])
    bz = tcf.bound_cir(w, a1, tau1, l_min, l_max, False)[..., -l_min]
    assert np.allclose(bz, (tcf._gamma(2, tcf.U32) + 2.0 ** -50 * 3) * np.abs(a1[:, :, :, :, :, 0, :]), rtol=1e-12)
    assert tcf.ratio(np.zeros(3), np.zeros(3), np.zeros(3)) == 0.0 and tcf.ratio(np.ones(3), np.zeros(3), np.zeros(3)) == np.inf


def test_a_bandwidth_that_float32_does_not_hold():
    """the reference's W in single precision is float32(bandwidth) and so is the entry's: the anchor takes that value, and the
    model, which multiplies by it, stays inside the bound (the double would sit up to u |tau W| further away - one more unit of
    the argument term)"""
    _, a, tau, l_min, l_max = tcc.make_cir(tcc.CIR_BY_NAME["ant2x2"])
    w = 7.68e6 + 0.3
    assert float(np.float32(w)) != w
    h = km.c2t_model_f32(w, a, tau, l_min, l_max, False)
    ref = tcf.anchor_cir(w, a, tau, l_min, l_max, False)
    assert np.array_equal(ref, tcf.anchor_cir(float(np.float32(w)), a, tau, l_min, l_max, False))
    assert not np.array_equal(ref, tcf.anchor_cir(w, a, tau, l_min, l_max, False, tcf.U64))
    assert tcf.ratio(h, ref, tcf.bound_cir(w, a, tau, l_min, l_max, False)) <= 1.0


def test_cir_to_time_lds_accounting():
    """the entry's arithmetic restated: dynamic LDS (padded table + four wave stages) plus the static 1 KiB of red[256] against
    the 160 KiB of a workgroup, more than the 64 KiB default asked for explicitly"""
    for c in tcc.CIR:
        assert km.c2t_lds_bytes(c.p, c.l) <= 160 * 1024, c
    assert km.c2t_lds_bytes(8, 31) <= 64 * 1024 < km.c2t_lds_bytes(9, 31)
    assert km.c2t_lds_bytes(16, 31) - 1024 <= 64 * 1024                          # what the entry let through uncounted
    assert km.c2t_lds_bytes(801, 31) == 160 * 1024 < km.c2t_lds_bytes(tcc.CIR_REFUSED.p, tcc.CIR_REFUSED.l)
    assert 256 * 32 * 8 == 64 * 1024 < 256 * tcc.APPLY_REFUSED.l * 8             # apply_time_kernel: L = 32 fills its stage


@pytest.fixture(scope="module")
def apply_case():
    cache = {}

    def get(name, scaled):
        if (name, scaled) not in cache:
            x, h, s = tcc.make_apply(tcc.APPLY_BY_NAME[name])
            s = s if scaled else None
            cache[(name, scaled)] = (x, h, s, tcf.anchor_apply(x, h, s), tcf.bound_apply(x, h, s))
        return cache[(name, scaled)]
    return get


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("name", [c.name for c in tcc.APPLY])
def test_apply_time_model_inside_the_bound(apply_case, name, scaled):
    x, h, s, ref, bd = apply_case(name, scaled)
    y = km.apt_model_f32(x, h, s)
    q = tcf.ratio(y, ref, bd)
    assert q <= 1.0, (name, scaled, q)
    if scaled:                                                                   # the link with scale 0 contributes exact zeros
        x0, h0 = x.copy(), h.copy()
        h0[-1, -1, :, -1] = 0
        assert np.array_equal(y[-1, -1], km.apt_model_f32(x0, h0, s)[-1, -1])


@pytest.mark.parametrize("mutation", km.APT_MUTATIONS)
def test_apply_time_seeded_faults_leave_the_bound(apply_case, mutation):
    scaled = mutation == "scale_other_tx"
    killers = []
    for c in tcc.APPLY:
        x, h, s, ref, bd = apply_case(c.name, scaled)
        if tcf.ratio(km.apt_model_f32(x, h, s, mutation=mutation), ref, bd) > 1.0:
            killers.append(c.name)
    print(f"{mutation}: caught by {killers}")
    assert killers, mutation
    if mutation != "scale_other_tx":
        assert {"3x32", "7x8", "506x8"} <= set(killers)                          # Tn < L, and past one block


@pytest.mark.parametrize("tag", ["cp2", "cp20", "c4", "small"])
def test_reference_execution_lies_within_the_bound_of_the_anchor(tag):
    """ties the anchor to the reference's own code and not to our reading of it: the float32 outputs the reference computed are
    float32 computations of the same sums (another order: no more roundings than the bound counts) stored in float32"""
    g = np.load(GOLD)
    fft, nsym, cp, l_min, l_max, B, nrx, nra, ntx, nta, P = (int(v) for v in g[f"{tag}_meta"])
    bw = fft * float(g[f"{tag}_scs"])
    a, tau = g[f"{tag}_a"], g[f"{tag}_tau"]
    assert a.dtype == np.complex64 and tau.dtype == np.float32
    for norm in (False, True):
        h = g[f"{tag}_h_time_n{int(norm)}"]
        ref, bd = tcf.anchor_cir(bw, a, tau, l_min, l_max, norm), tcf.bound_cir(bw, a, tau, l_min, l_max, norm)
        q = tcf.ratio(h, ref, bd + tcf.U32 * np.abs(h))
        print(f"{tag} normalize={norm}: reference-executed h_time at {q:.3f} of the bound")
        assert q <= 1.0, (tag, norm, q)
    h = g[f"{tag}_h_time_n1"]
    x = g[f"{tag}_x_time"].reshape(B, ntx, nta, -1)
    y = g[f"{tag}_y_time"]
    q = tcf.ratio(y, tcf.anchor_apply(x, h), tcf.bound_apply(x, h) + tcf.U32 * np.abs(y))
    print(f"{tag}: reference-executed y_time at {q:.3f} of the bound")
    assert q <= 1.0, (tag, q)
