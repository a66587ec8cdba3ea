"""The time-domain channel kernels (csrc/ofdm_time.hip ``cir_to_time_kernel``, ``apply_time_kernel``; csrc/f64_time.hip
``cir_to_time128_kernel``, ``time_normalize128_kernel``, ``apply_time128_kernel``) through the public API against the float64
anchors of tests/time_channel_f32.py, on EVERY output, within the bounds derived there from the kernels' arithmetic: u = 2^-24
for complex64 inputs, u = 2^-53 for complex128.

The cases (tests/time_channel_cases.py) are the smallest that reach each path: lag tiles of 9 with and without a tail tile, wave
passes of 64 and block passes of 256 time steps with and without a partial pass, odd and even sinc tables, every antenna count,
delays that are 0, integers of the lag grid and up to 92 lags away, a link without energy, the LDS sizes at which the entry
asks for more than the default 64 KiB and the largest it accepts; for ApplyTimeChannel Tn < L (both window clips at once), the
largest tap stage and the block edges of Tout.  Each runs with ``normalize`` off, on and deferred.  The CPU side
(tests/test_time_channel_host.py) shows on these very inputs that the bound is neither too tight nor too loose.

Every test prints its max |out - anchor| / bound (run with -s).  On an MI355X with ROCm's device library, the largest ratio per
case family (over normalize off / on / deferred), complex64 | complex128:
  cir L* 0.35 | 0.020   T* 0.31 | 0.035   P* 0.36 | 0.018   ant* 0.28 | 0.007   tdl 0.38 | 0.0006   tau0 0.41 | 0.016
      tauint 0.23 | 0.003   zero 0.32 | 0.006   lds8 / 9 / 16 0.23 | 0.009   lds801 0.006 | 0.0000
  deferred factor (complex64 only) 0.003 (tdl) ... 0.16 (L1); lds801 0.0008
  apply 0.045 ... 0.22, with link_scale 0.050 ... 0.25 | 0.013
Nothing is above 1 and in complex64 the bound is not idle; the complex64 figures are those of the NumPy models on the CPU to two
digits.  Where a figure is below 0.01 the bound cannot be tightened from the inputs alone:
- complex128: the anchor is itself a float64 evaluation, and its own term 2^-50 (|tau W| + P + 2) sum |a_p| (2^-50 (N + 1) S for
  apply) is 10 to 100 times the kernel's terms at u = 2^-53 - the bar is the anchor's accuracy, about 1e-14 for unit taps where
  the former test asked 1e-9; a seeded fault moves an output by the size of a weak tap, 1e-2 and more;
- lds801: gamma(802) grows with P while 801 roundings of random sign add up like sqrt(P); the case is there for the LDS limit;
- the deferred factor at many terms (tdl, lds801): rho_d = c(B) / c64 takes every output at its bound at once."""
import numpy as np
import pytest
import torch

import time_channel_cases as tcc
import time_channel_f32 as tcf

pytestmark = pytest.mark.gpu

PREC = {"single": (tcf.U32, np.complex64, np.float32, torch.complex64), "double": (tcf.U64, np.complex128, np.float64, torch.complex128)}


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _hold(out, ref, bd, cdtype, what):
    """|out - anchor| <= bound on every output; returns the largest ratio"""
    out = np.asarray(out)
    assert out.shape == ref.shape and out.dtype == cdtype, (what, out.shape, out.dtype)
    assert np.all(np.isfinite(out.view(out.real.dtype))), what
    q = tcf.ratio(out, ref, bd)
    print(f"tc {what}: max |out - anchor| / bound = {q:.4f}")
    bad = np.abs(out.astype(ref.dtype) - ref) > bd
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs outside the bound, worst ratio {q:.3f}"
    return q


@pytest.fixture(scope="module")
def cir():
    """inputs, anchors and bounds of a case per precision, computed once and shared (read-only)"""
    cache = {}

    def get(case, prec):
        if (case.name, prec) not in cache:
            u, cdt, rdt, _ = PREC[prec]
            w, a, tau, l_min, l_max = tcc.make_cir(case)
            args = (w, a.astype(cdt), tau.astype(rdt), l_min, l_max)
            d = dict(args=args, scale=(tcf.anchor_scale(*args, u), tcf.bound_scale(*args, u)))
            for norm in (False, True):
                d[norm] = (tcf.anchor_cir(*args, norm, u), tcf.bound_cir(*args, norm, u))
            for v in args[1:3] + d[False] + d[True] + d["scale"]:
                v.setflags(write=False)
            cache[(case.name, prec)] = d
        return cache[(case.name, prec)]
    return get


def _run_cir(phy, case, prec, d):
    cdt = PREC[prec][1]
    run = phy.channel.cir_to_time_channel
    for norm in (False, True):
        h = _np(run(*d["args"], normalize=norm))
        _hold(h, *d[norm], cdt, f"cir {case.name} {prec} normalize={norm}")
    h, s = run(*d["args"], normalize=True, _defer_norm=True)
    if prec == "double":                                             # the float64 kernels normalise in place
        assert s is None
        _hold(_np(h), *d[True], cdt, f"cir {case.name} {prec} deferred")
    else:
        assert s.dtype == torch.float32
        _hold(_np(h), *d[False], cdt, f"cir {case.name} {prec} deferred")
        _hold(_np(s), *d["scale"], np.float32, f"cir {case.name} {prec} scale")
    if case.kind == "zero":
        b, rx, tx = tcc.ZERO_LINK
        hn = _np(run(*d["args"], normalize=True))
        assert np.all(hn[b, rx, :, tx] == 0) and (s is None or float(s[b, rx, tx]) == 0.0)


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("case", tcc.CIR, ids=[c.name for c in tcc.CIR])
def test_cir_to_time_holds_the_bound(phy, cir, case, prec):
    _run_cir(phy, case, prec, cir(case, prec))


def test_cir_to_time_refuses_what_the_lds_cannot_hold(phy, cir):
    """one path past the largest accepted table at L = 31: the project's error, raised by the entry before any launch - the
    device is untouched and the next call computes"""
    w, a, tau, l_min, l_max = tcc.make_cir(tcc.CIR_REFUSED)
    for norm in (False, True):
        with pytest.raises(ValueError, match="LDS sinc table"):
            phy.channel.cir_to_time_channel(w, a, tau, l_min, l_max, normalize=norm)
    torch.cuda.synchronize()
    case = tcc.CIR_BY_NAME["lds801"]
    d = cir(case, "single")
    _hold(_np(phy.channel.cir_to_time_channel(*d["args"], normalize=True)), *d[True], np.complex64, "cir lds801 after the refusal")


@pytest.fixture(scope="module")
def apply_case():
    cache = {}

    def get(case, prec, scaled):
        key = (case.name, prec, scaled)
        if key not in cache:
            u, cdt, _, _ = PREC[prec]
            x, h, s = tcc.make_apply(case)
            x, h, s = x.astype(cdt), h.astype(cdt), (s if scaled else None)
            cache[key] = (x, h, s, tcf.anchor_apply(x, h, s), tcf.bound_apply(x, h, s, u))
        return cache[key]
    return get


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("case", tcc.APPLY, ids=[c.name for c in tcc.APPLY])
def test_apply_time_holds_the_bound(phy, apply_case, case, prec):
    cdt = PREC[prec][1]
    blk = phy.channel.ApplyTimeChannel(case.tn, case.l, precision=prec)
    x, h, _, ref, bd = apply_case(case, prec, False)
    y = _np(blk(x, h))
    _hold(y, ref, bd, cdt, f"apply {case.name} {prec}")
    if prec == "single":                                             # the deferred factor exists in float32 only
        x, h, s, ref, bd = apply_case(case, prec, True)
        ys = _np(blk(x, h, _link_scale=torch.from_numpy(s).cuda()))
        _hold(ys, ref, bd, cdt, f"apply {case.name} {prec} link_scale")
        hz = h.copy()
        hz[-1, -1, :, -1] = 0                                        # the link whose scale is 0 adds exact zeros
        assert np.array_equal(ys[-1, -1], _np(blk(x, hz, _link_scale=torch.from_numpy(s).cuda()))[-1, -1])


def test_apply_time_refuses_a_stage_past_the_lds(phy):
    c = tcc.APPLY_REFUSED
    x, h, s = tcc.make_apply(c, batch=1)
    with pytest.raises(ValueError, match="LDS tap stage"):
        phy.channel.ApplyTimeChannel(c.tn, c.l)(x, h)
    torch.cuda.synchronize()
    y = phy.channel.ApplyTimeChannel(c.tn, c.l, precision="double")(x.astype(np.complex128), h.astype(np.complex128))
    _hold(_np(y), tcf.anchor_apply(x, h), tcf.bound_apply(x, h, u=tcf.U64), np.complex128, "apply 3x33 double (no stage)")


class _FixedCir:
    """channel-model stub: hands out the given taps and delays"""

    def __init__(self, a, tau):
        self.a, self.tau = a, tau

    def __call__(self, batch_size, num_time_steps, sampling_frequency=None):
        assert batch_size == self.a.shape[0] and num_time_steps == self.a.shape[-1]
        return self.a, self.tau


def test_time_channel_deferred_equals_two_passes_past_one_block(phy):
    """TimeChannel(return_channel=False) applies the normalisation factor to the taps while it applies the channel; with two
    receivers, two transmitters, 2 x 2 antennas and Tout = 259 (past one block) the received signal has the bits of the two-pass
    path, and both lie within the bound of the anchor on the returned channel"""
    tn, l_tot = 250, 10
    case = tcc.Cir("defer", 2, 2, 3, tn + l_tot - 1, l_tot, tcc.W_TIGHT, "zero")
    w, a, tau, l_min, l_max = tcc.make_cir(case)
    x = tcc.make_apply(tcc.Apply("defer", 2, 2, 2, 2, tn, l_tot))[0]
    a_t, tau_t, x_t = (torch.from_numpy(v).cuda() for v in (a, tau, x))
    mk = lambda ret: phy.channel.TimeChannel(_FixedCir(a_t, tau_t), w, tn, l_min=l_min, l_max=l_max, normalize_channel=True,
                                             return_channel=ret)
    y1 = _np(mk(False)(x_t))
    y2, h = mk(True)(x_t)
    y2, h = _np(y2), _np(h)
    assert y1.shape == (tcc.BATCH, 2, 2, tn + l_tot - 1)
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))
    b, rx, tx = tcc.ZERO_LINK
    assert np.all(h[b, rx, :, tx] == 0)
    _hold(h, tcf.anchor_cir(w, a, tau, l_min, l_max, True), tcf.bound_cir(w, a, tau, l_min, l_max, True), np.complex64, "cir defer block")
    _hold(y2, tcf.anchor_apply(x, h), tcf.bound_apply(x, h), np.complex64, "apply defer block")


@pytest.mark.parametrize("prec", list(PREC))
def test_empty_batch(phy, prec):
    """batch 0 through the four entry points: empty tensors of the right shape and dtype, as every other block returns"""
    _, cdt, rdt, tdt = PREC[prec]
    a, tau = np.zeros((0, 2, 1, 2, 2, 3, 5), cdt), np.zeros((0, 2, 2, 3), rdt)
    for norm in (False, True):
        h = phy.channel.cir_to_time_channel(tcc.W_TIGHT, a, tau, -6, 3, normalize=norm)
        assert tuple(h.shape) == (0, 2, 1, 2, 2, 5, 10) and h.dtype == tdt
    h, s = phy.channel.cir_to_time_channel(tcc.W_TIGHT, a, tau, -6, 3, normalize=True, _defer_norm=True)
    assert tuple(h.shape) == (0, 2, 1, 2, 2, 5, 10) and h.dtype == tdt
    assert s is None if prec == "double" else (tuple(s.shape) == (0, 2, 2) and s.dtype == torch.float32)
    x, ht = np.zeros((0, 2, 2, 7), cdt), np.zeros((0, 2, 1, 2, 2, 14, 8), cdt)
    y = phy.channel.ApplyTimeChannel(7, 8, precision=prec)(x, ht)
    assert tuple(y.shape) == (0, 2, 1, 14) and y.dtype == tdt
    torch.cuda.synchronize()
