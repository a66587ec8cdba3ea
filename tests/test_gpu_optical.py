"""Optical channels on the GPU (csrc/optical.hip) against the float64 specification tests/optical_f32.py.

Bars, from the fixture alone (tests/golden/optical_ref_golden.npz, the reference's own two precisions): complex64
4 e32 + 2^-23 max|y|, complex128 that times 2^-29 (row a19g's convention).  The noise, with no transform in the way, is
held to the specification's stream model at the tolerance test_awgn_matches_stream_spec uses for the same Box-Muller
(rtol 1e-5, atol 2e-6 on unit-variance draws, i.e. scaled by the noise's standard deviation)."""
import json
import os

import numpy as np
import pytest
import torch

import optical_cases as oc
import optical_f32 as spec

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "optical_ref_golden.npz"))
META = json.loads(str(G["meta"]))
V = np.load(os.path.join(GOLD, "optical_ref_vectors.npz"))


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def bar(name, precision):
    b = 4.0 * META[name]["e32"] + 2.0 ** -23 * META[name]["ymax"]
    return b if precision == "single" else b * 2.0 ** -29


_REF = {}


def reference(name):
    """the float64 specification's result of a case, computed once"""
    if name not in _REF:
        _REF[name] = spec.ssfm(oc.make_input(name), precision="double", **oc.parameters(name))
    return _REF[name]


def run(phy, name, precision, x=None):
    blk = phy.channel.SSFM(precision=precision, **oc.parameters(name))
    x = oc.make_input(name) if x is None else x
    y = _np(blk(x.astype(np.complex64 if precision == "single" else np.complex128) if isinstance(x, np.ndarray) else x))
    return y, blk.last_num_steps


@pytest.mark.parametrize("precision", ["single", "double"])
@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_ssfm_matches_the_specification(phy, name, precision):
    """Measured on the MI355X: every case inside its bar; the closest is `window_adaptive` in complex64, 9.2e-7 of 1.06e-6
    (complex128: 1.2e-15 of 2.0e-15).  The bar stays as the fixture gives it."""
    y, steps = run(phy, name, precision)
    want, want_steps = reference(name)
    err = float(np.max(np.abs(y.astype(np.complex128) - want)))
    print(f"{name} {precision}: steps {steps} ({want_steps}), error {err:.3e}, bar {bar(name, precision):.3e}")
    assert y.shape == want.shape and y.dtype == (np.complex64 if precision == "single" else np.complex128)
    assert np.all(np.isfinite(y.view(y.real.dtype)))
    assert steps == want_steps
    assert err <= bar(name, precision)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_empty_batch_and_one_row(phy, precision):
    cd = np.complex64 if precision == "single" else np.complex128
    blk = phy.channel.SSFM(precision=precision, **oc.parameters("fixed2"))
    assert tuple(blk(np.zeros((0, 64), cd)).shape) == (0, 64)
    assert tuple(phy.channel.SSFM(with_manakov=True, precision=precision)(np.zeros((0, 2, 64), cd)).shape) == (0, 2, 64)
    assert tuple(phy.channel.EDFA(precision=precision)(np.zeros((0, 64), cd)).shape) == (0, 64)
    x = oc.make_input("fixed2")
    y = _np(blk(x[1].astype(cd)))                                  # rank 1: one row
    assert y.shape == (64,)
    assert float(np.max(np.abs(y - reference("fixed2")[0][1]))) <= bar("fixed2", precision)


def test_strided_view(phy):
    x = oc.make_input("fixed2")
    wide = torch.zeros((3, 2, 128), dtype=torch.complex64, device="cuda")
    wide[:, 0, ::2] = torch.from_numpy(x).cuda()
    view = wide[:, 0, ::2]
    assert not view.is_contiguous()
    y = _np(phy.channel.SSFM(**oc.parameters("fixed2"))(view))
    assert float(np.max(np.abs(y - reference("fixed2")[0]))) <= bar("fixed2", "single")
    assert torch.equal(wide[:, 0, ::2].cpu(), torch.from_numpy(x))   # the input is left as it was


@pytest.mark.parametrize("scheme", ["fixed", "adaptive"])
def test_shipped_known_answers_in_double(phy, scheme):
    """test_optical.py:25-92 (length 5, n_ssfm = 2000 and the adaptive scheme): the reference's criterion
    mean((|u| - u_ref)^2) <= 1e-7 on the shipped five-digit vectors, and max | |u| - |u_double| | <= 1e-7 against the
    reference's own double-precision result of the same configuration"""
    par = dict(alpha=0.0, beta_2=1.0, gamma=1.0, half_window_length=0, length=5.0, sample_duration=float(V["sample_duration"]),
               with_amplification=False, with_attenuation=False, n_sp=1.0, precision="double")
    par.update(dict(n_ssfm=2000) if scheme == "fixed" else dict(n_ssfm="adaptive", phase_inc=1e-3))
    y = _np(phy.channel.SSFM(**par)(V["u0"].astype(np.complex128)))
    mse = float(np.mean((np.abs(y) - V["u_ref"]) ** 2))
    dev = float(np.max(np.abs(np.abs(y) - np.abs(V["y_" + scheme]))))
    print(f"{scheme}: mean square {mse:.3e}, against the reference's double result {dev:.3e}")
    assert mse <= 1e-7 and dev <= 1e-7
    u2 = np.sqrt(9 / 8 * 0.5) * np.tile(V["u0"], (3, 2, 1)).astype(np.complex128)
    y2 = _np(phy.channel.SSFM(with_manakov=True, **par)(u2))
    assert float(np.mean((np.linalg.norm(y2 * np.sqrt(8 / 9), axis=-2) - V["u_ref"]) ** 2)) <= 1e-7


def test_adaptive_step_that_does_not_advance_is_refused(phy):
    """an infinite sample makes phase_inc / gamma / max|q|^2 zero: the reference's loop would never end, the entry refuses"""
    x = oc.make_input("adaptive40").copy()
    x[1, 7] = np.inf
    with pytest.raises(ValueError, match="does not advance"):
        phy.channel.SSFM(**oc.parameters("adaptive40"))(x)


# ------------------------------------------------------------------ derived checks that need no fixture
@pytest.mark.parametrize("precision", ["single", "double"])
def test_dispersion_only_is_one_closed_form_transfer(phy, precision):
    name = "no_nonlinearity"
    x = oc.make_input(name)
    par = dict(oc.parameters(name), with_attenuation=False)
    n, L = x.shape[-1], par["length"]
    # the phase reaches 8.6e3 rad at the band edge: float64 defines it to 2^-53 * 8.6e3 = 1e-12 rad only, which is more than
    # the complex128 bar allows - so the closed form takes its products in the specification's order (c2 = -beta_2 / 2 w w)
    omega = 2.0 * np.pi * spec.bin_frequency(n, par["sample_duration"])
    h = np.exp(1j * ((-par["beta_2"] / 2.0 * omega * omega) * L))
    want = np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * h, axis=-1)
    cd = np.complex64 if precision == "single" else np.complex128
    y1 = _np(phy.channel.SSFM(precision=precision, **dict(par, n_ssfm=1))(x.astype(cd)))
    y8 = _np(phy.channel.SSFM(precision=precision, **dict(par, n_ssfm=8))(x.astype(cd)))
    b = bar(name, precision)
    assert np.max(np.abs(y1 - y8)) <= b and np.max(np.abs(y1 - want)) <= b and np.max(np.abs(y8 - want)) <= b


def test_nonlinearity_only_rotates(phy):
    x = oc.make_input("fixed1")
    par = dict(oc.parameters("fixed1"), with_dispersion=False, with_attenuation=False, n_ssfm=1, length=8)
    y = _np(phy.channel.SSFM(**par)(x))
    ulp = np.spacing(np.abs(x))
    assert np.all(np.abs(np.abs(y.astype(np.complex128)) - np.abs(x.astype(np.complex128))) <= 2 * ulp)
    phase = np.angle(y.astype(np.complex128) * np.conj(x.astype(np.complex128)))
    want = -par["gamma"] * np.abs(x.astype(np.complex128)) ** 2 * par["length"]
    assert np.max(np.abs(np.angle(np.exp(1j * (phase - want))))) <= 1e-5


@pytest.mark.parametrize("n_ssfm", [1, 4])
def test_attenuation_with_noiseless_amplification_is_transparent(phy, n_ssfm):
    x = oc.make_input("fixed1")
    par = dict(oc.parameters("fixed1"), with_dispersion=False, with_nonlinearity=False, with_amplification=True, n_sp=0.0,
               n_ssfm=n_ssfm)
    assert np.array_equal(_np(phy.channel.SSFM(**par)(x)), x)


# ------------------------------------------------------------------ noise
NOISY = dict(oc.BASE, with_amplification=True, n_sp=1.5, with_dispersion=False, n_ssfm=3, length=8)


@pytest.mark.parametrize("precision", ["single", "double"])
@pytest.mark.parametrize("manakov", [False, True])
def test_noise_matches_the_stream_model(phy, precision, manakov):
    shape = (3, 2, 37) if manakov else (5, 37)
    rng = np.random.default_rng(5)
    x = (1e-3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)
    par = dict(NOISY, with_manakov=manakov)
    phy.config.seed = 123
    phy.config.rng.call = 7
    cd = np.complex64 if precision == "single" else np.complex128
    y = _np(phy.channel.SSFM(precision=precision, **par)(x.astype(cd)))
    assert phy.config.rng.call == 7 + 3                            # one call of the stream per step
    want, _ = spec.ssfm(x, precision=precision, seed=123, call=7, **par)
    sigma = np.sqrt(spec.p_n_ase_ssfm(par["alpha"], par["f_c"], par["length"], par["n_sp"], 1.0, 1e-12, manakov) / 3 / 2)
    assert np.max(np.abs(want - x)) > 2 * sigma                    # the noise is there
    tol = (1e-5 * np.abs(want - x) + 2e-6 * sigma * 3) if precision == "single" else 1e-12 * sigma
    assert np.all(np.abs(y - want) <= tol + 2.0 ** -22 * np.abs(want))


@pytest.mark.parametrize("manakov", [False, True])
def test_ase_power_with_dispersion(phy, manakov):
    """about 1e6 samples of noise alone through dispersion and nonlinearity: the power is p_n_ase within 5 standard errors
    (the sample mean of |n|^2 of N complex Gaussians has the standard error p / sqrt(N))"""
    shape = (128, 2, 4096) if manakov else (256, 4096)
    par = dict(oc.BASE, with_amplification=True, n_sp=1.0, n_ssfm=4, with_manakov=manakov)
    y = _np(phy.channel.SSFM(**par)(np.zeros(shape, np.complex64))).astype(np.complex128)
    p = spec.p_n_ase_ssfm(par["alpha"], par["f_c"], par["length"], par["n_sp"], 1.0, 1e-12, manakov)
    got = float(np.mean(np.abs(y) ** 2))
    print(f"ASE power {got:.6e}, p_n_ase {p:.6e}, {abs(got - p) / (p / np.sqrt(y.size)):.2f} standard errors")
    assert abs(got - p) <= 5 * p / np.sqrt(y.size)


@pytest.mark.parametrize("precision", ["single", "double"])
@pytest.mark.parametrize("dual", [False, True])
def test_edfa_noise_power_and_stream(phy, precision, dual):
    shape = (128, 2, 4096) if dual else (256, 4096)
    cd = np.complex64 if precision == "single" else np.complex128
    phy.config.seed = 9
    amp = phy.channel.EDFA(g=4.0, f=7.0, f_c=193.55e12, dt=1e-12, with_dual_polarization=dual, precision=precision)
    y = _np(amp(np.zeros(shape, cd))).astype(np.complex128)
    _, _, p = spec.edfa_parameters(4.0, 7.0, 193.55e12, 1e-12, dual, precision)
    got = float(np.mean(np.abs(y) ** 2))
    print(f"EDFA noise power {got:.6e}, p_n_ase {p:.6e}, {abs(got - p) / (p / np.sqrt(y.size)):.2f} standard errors")
    assert abs(got - p) <= 5 * p / np.sqrt(y.size)
    # the stream model, on a signal
    x = oc.make_input("fixed1")[..., None, :].repeat(2, axis=-2) if dual else oc.make_input("fixed1")
    phy.config.seed = 31
    got = _np(amp(x.astype(cd)))
    want = spec.edfa(x, 4.0, 7.0, 193.55e12, 1e-12, dual, precision, seed=31, call=0)
    sigma = spec.edfa_parameters(4.0, 7.0, 193.55e12, 1e-12, dual, precision)[1]
    tol = (1e-5 * np.abs(want - 2 * x) + 2e-6 * sigma) if precision == "single" else 1e-12 * sigma
    assert np.all(np.abs(got - want) <= tol + 2.0 ** -22 * np.abs(want))


@pytest.mark.parametrize("precision", ["single", "double"])
def test_edfa_gain(phy, precision):
    cd = np.complex64 if precision == "single" else np.complex128
    x = oc.make_input("fixed1").astype(cd)
    assert np.array_equal(_np(phy.channel.EDFA(g=1.0, precision=precision)(x)), x)             # noiseless: exactly sqrt(g) = 1
    assert np.array_equal(_np(phy.channel.EDFA(g=4.0, f=0.0, precision=precision)(x)), 2 * x)
    # otherwise within one ulp of sqrt(g) x: the product with sqrt(g) rounded to the working precision, rounded once
    y = _np(phy.channel.EDFA(g=3.0, f=0.0, precision=precision)(x))
    assert np.array_equal(y, spec.edfa(x, 3.0, 0.0, precision=precision))
    want = x.astype(np.complex128) * np.sqrt(3.0)
    assert np.all(np.abs(y.real - want.real) <= np.spacing(np.abs(y.real))) and np.all(np.abs(y.imag - want.imag) <= np.spacing(np.abs(y.imag)))


def test_two_calls_differ_and_a_seed_reproduces(phy):
    x = np.zeros((4, 64), np.complex64)
    for make in (lambda: phy.channel.SSFM(**NOISY), lambda: phy.channel.EDFA()):
        phy.config.seed = 77
        blk = make()
        a, b = _np(blk(x)), _np(blk(x))
        phy.config.seed = 77
        a2 = _np(make()(x))
        assert not np.array_equal(a, b) and np.array_equal(a, a2)
        assert abs(np.corrcoef(a.real.ravel(), b.real.ravel())[0, 1]) < 0.2


# ------------------------------------------------------------------ the notebook's link
@pytest.mark.parametrize("precision", ["single", "double"])
def test_span_loop(phy, precision):
    sp = oc.SPAN
    cd = np.complex64 if precision == "single" else np.complex128
    span = phy.channel.SSFM(precision=precision, **sp["ssfm"])
    amp = phy.channel.EDFA(precision=precision, **sp["edfa"])
    u = oc.span_input().astype(cd)
    w = oc.span_input().astype(np.complex128)
    for _ in range(sp["n_span"]):
        u = amp(span(u))
        w = spec.edfa(spec.ssfm(w, precision="double", **sp["ssfm"])[0], precision="double", **sp["edfa"])
    err = float(np.max(np.abs(_np(u).astype(np.complex128) - w)))
    print(f"span loop {precision}: {err:.3e}, bar {bar('span', precision):.3e}; the reference's double result {np.max(np.abs(w - G['span/y64'])):.3e}")
    assert err <= bar("span", precision)
    assert np.max(np.abs(w - G["span/y64"])) <= bar("span", "double")
