"""Host side of the precoders (no GPU needed): the reference's signatures and import paths, the float32 specification
(tests/precoding_f32.py) against the complex128 oracle (oracle/precoding.py) and against both reference-executed fixtures,
and the argument errors that are raised before anything reaches the device."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import precoding_f32 as spec
from oracle import precoding as op

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "precoding_ref_golden.npz"))
MU = np.load(os.path.join(HERE, "golden", "precoding_mu_ref_golden.npz"))


def close(a, b, tol):
    return a.shape == b.shape and np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1.0)


# parameter names, order and defaults of the reference (src/sionna/phy/...)
REFERENCE_SIGNATURES = {
    "rzf_precoding_matrix": [("h", None), ("alpha", 0.), ("precision", None)],                       # mimo/precoding.py:12-14
    "cbf_precoding_matrix": [("h", None), ("precision", None)],                                        # mimo/precoding.py:91
    "rzf_precoder": [("x", None), ("h", None), ("alpha", 0.), ("return_precoding_matrix", False),
                     ("precision", None)],                                                             # mimo/precoding.py:157-161
    "RZFPrecoder": [("resource_grid", None), ("stream_management", None), ("return_effective_channel", False),
                    ("precision", None), ("kwargs", None)],                                            # ofdm/precoding.py:67-72
}


def _params(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        if p.name == "self":
            continue
        out.append((p.name, None if p.default is inspect.Parameter.empty else p.default))
    return out


def test_signatures_match_the_reference():
    from sionna_amd.phy import mimo, ofdm
    for name in ("rzf_precoding_matrix", "cbf_precoding_matrix", "rzf_precoder"):
        assert _params(getattr(mimo, name)) == REFERENCE_SIGNATURES[name], name
        assert getattr(mimo, name) is getattr(mimo.precoding, name)
    assert _params(ofdm.RZFPrecoder.__init__) == REFERENCE_SIGNATURES["RZFPrecoder"]
    assert ofdm.RZFPrecoder is ofdm.precoding.RZFPrecoder
    assert inspect.signature(ofdm.RZFPrecoder.call).parameters["alpha"].default == 0.


def test_notebook_import_line_resolves_under_install_as_sionna():
    """Cell 4 of MIMO_OFDM_Transmissions_over_CDL.ipynb, run in a fresh interpreter (install_as_sionna aliases modules)."""
    code = ("import sionna_amd; sionna_amd.install_as_sionna(tf_shim=True)\n"
            "from sionna.phy.ofdm import ResourceGrid, ResourceGridMapper, LSChannelEstimator, LMMSEEqualizer, \\\n"
            "    OFDMModulator, OFDMDemodulator, RZFPrecoder, RemoveNulledSubcarriers\n"
            "import sionna.phy.mimo.precoding as p\n"
            "from sionna.phy.mimo.precoding import rzf_precoder, rzf_precoding_matrix, cbf_precoding_matrix\n"
            "import sionna.phy.ofdm\n"
            "assert sionna.phy.ofdm.RZFPrecoder is RZFPrecoder and p.rzf_precoder is rzf_precoder\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def _conditioned(seed, lead, K, M, alpha):
    rng = np.random.default_rng(seed)
    h = ((rng.normal(size=lead + (K, M)) + 1j * rng.normal(size=lead + (K, M))) / np.sqrt(2)).astype(np.complex64)
    a = h.astype(np.complex128) @ np.conj(np.swapaxes(h, -1, -2)).astype(np.complex128) + np.asarray(alpha)[..., None, None] * np.eye(K)
    return h, np.linalg.cond(a)


@pytest.mark.parametrize("K,M,alpha", [(1, 2, 0.0), (2, 4, 0.0), (4, 8, 0.3), (8, 16, 0.0), (3, 7, 0.1), (4, 4, 0.05)])
def test_spec_within_conditioning_of_the_complex128_oracle(K, M, alpha):
    h, cond = _conditioned(K * 100 + M, (64,), K, M, alpha)
    rng = np.random.default_rng(7)
    x = ((rng.normal(size=(64, K)) + 1j * rng.normal(size=(64, K))) / np.sqrt(2)).astype(np.complex64)
    xp, g = spec.rzf_precoder(x, h, alpha)
    xo, go = op.rzf_precoder(x, h, alpha)
    bound = 8 * K * M * cond * 2.0 ** -24                               # per item: cond(A) 2^-24 times the operation count
    err = np.abs(g - go).max(axis=(-1, -2)) / np.abs(go).max(axis=(-1, -2))
    assert np.all(err <= bound), (err.max(), bound.max())
    assert np.all(np.abs(xp - xo).max(-1) <= bound * np.abs(xo).max(-1) * np.sqrt(K) + 1e-6)
    gc = spec.precoding_matrix(h, mode="cbf")
    hc = np.conj(np.swapaxes(h.astype(np.complex128), -1, -2))
    assert np.allclose(gc, hc / np.linalg.norm(hc, axis=-2, keepdims=True), rtol=0, atol=1e-6)


def test_spec_zero_column_is_zero():
    h = np.zeros((2, 2, 4), np.complex64)
    h[1, 0, :] = 1.0
    g = spec.precoding_matrix(h, mode="cbf")
    assert np.all(g[0] == 0) and np.all(g[1, :, 1] == 0) and np.allclose(np.abs(g[1, :, 0]) ** 2, 0.25)


@pytest.mark.parametrize("i", range(5))
def test_spec_matches_reference_execution(i):
    g = {k.split("/", 1)[1]: GOLD[k] for k in GOLD.files if k.startswith(f"m{i}/")}
    xp, gm = spec.rzf_precoder(g["x"], g["h"], g["alpha"])
    assert close(gm, g["g"], 2e-5) and close(xp, g["x_precoded"], 2e-5)


@pytest.mark.parametrize("tag,alpha", [("zf", 0.0), ("rzf", 0.2)])
def test_ofdm_spec_matches_reference_execution(tag, alpha):
    xp, heff = spec.ofdm_rzf_precoder(GOLD["o/x_rg"], GOLD["o/h"], GOLD["o/precoding_ind"], GOLD["o/effective_subcarrier_ind"], alpha)
    assert close(xp, GOLD[f"o_{tag}/x_precoded"], 1e-4) and close(heff, GOLD[f"o_{tag}/h_eff"], 1e-4)


@pytest.mark.parametrize("case", ["mu1", "mu2"])
def test_multi_user_spec_and_oracle_match_reference_execution(case):
    g = {k.split("/", 1)[1]: MU[k] for k in MU.files if k.startswith(case + "/")}
    xp, heff = spec.ofdm_rzf_precoder(g["x"], g["h"], g["precoding_ind"], g["effective_subcarrier_ind"], g["alpha"])
    assert close(xp, g["x_precoded"], 1e-4) and close(heff, g["h_eff"], 1e-4)
    xo, ho = op.ofdm_rzf_precoder(g["x"], g["h"], g["precoding_ind"], g["effective_subcarrier_ind"], g["alpha"])
    assert close(xo, g["x_precoded"], 1e-4) and close(ho, g["h_eff"], 1e-4)
    if case == "mu2":                                                           # interference: the other transmitter's entries
        assert np.abs(g["h_eff"][:, 0, :, 1]).max() > 0.1 and np.abs(g["h_eff"][:, 1, :, 0]).max() > 0.1


def test_matrix_level_multi_user_fixture():
    for i in range(3):
        assert close(spec.precoding_matrix(MU[f"cbf{i}/h"], mode="cbf"), MU[f"cbf{i}/g"], 2e-5)
    xp, g = spec.rzf_precoder(MU["rzf/x"], MU["rzf/h"], MU["rzf/alpha"])
    assert close(g, MU["rzf/g"], 2e-5) and close(xp, MU["rzf/x_precoded"], 2e-5)


def _grid(num_tx=1, streams=4):
    from sionna_amd.phy import ofdm
    return ofdm.ResourceGrid(num_ofdm_symbols=14, fft_size=72, subcarrier_spacing=15e3, num_tx=num_tx, num_streams_per_tx=streams,
                             cyclic_prefix_length=6, num_guard_carriers=[5, 6], dc_null=True, pilot_pattern=None)


def test_argument_errors():
    from sionna_amd.phy import mimo, ofdm
    z = lambda *s: np.zeros(s, np.complex64)
    with pytest.raises(ValueError, match="K <= M"):
        mimo.rzf_precoding_matrix(z(3, 5, 4))
    with pytest.raises(ValueError, match="K <= M"):
        mimo.cbf_precoding_matrix(z(3, 5, 4))
    with pytest.raises(ValueError, match="M = 32"):
        mimo.rzf_precoding_matrix(z(3, 4, 40))
    with pytest.raises(ValueError, match="x must have shape"):
        mimo.rzf_precoder(z(3, 3), z(3, 2, 4))
    rg, sm = _grid(), mimo.StreamManagement(np.array([[1]]), 4)
    pre = ofdm.RZFPrecoder(rg, sm, return_effective_channel=True)
    with pytest.raises(ValueError, match="x must have shape"):
        pre(z(2, 1, 4, 14, 64), z(2, 1, 4, 1, 8, 14, 64))                       # fft size of another grid
    with pytest.raises(ValueError, match="h must have shape"):
        pre(z(2, 1, 4, 14, 72), z(2, 2, 4, 1, 8, 14, 72))                       # two receivers, the StreamManagement has one
    with pytest.raises(ValueError, match="channel rows"):
        pre(z(2, 1, 4, 14, 72), z(2, 1, 2, 1, 8, 14, 72))                       # 2 receive antennas for 4 streams
    with pytest.raises(ValueError, match="K <= M"):
        pre(z(2, 1, 4, 14, 72), z(2, 1, 4, 1, 2, 14, 72))                       # 4 streams from 2 antennas
    with pytest.raises(ValueError, match="disagree"):
        ofdm.RZFPrecoder(_grid(streams=2), sm)(z(1, 1, 2, 14, 72), z(1, 1, 2, 1, 4, 14, 72))


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sionna_amd.phy import mimo, ofdm
    h = np.ones((2, 2, 4), np.complex64)
    with pytest.raises(RuntimeError):
        mimo.rzf_precoding_matrix(h)
    with pytest.raises(RuntimeError):
        mimo.rzf_precoder(np.ones((2, 2), np.complex64), h, 0.1, True)
    with pytest.raises(RuntimeError):
        mimo.cbf_precoding_matrix(h)
    rg, sm = _grid(), mimo.StreamManagement(np.array([[1]]), 4)
    with pytest.raises(RuntimeError):
        ofdm.RZFPrecoder(rg, sm)(np.ones((1, 1, 4, 14, 72), np.complex64), np.ones((1, 1, 4, 1, 8, 14, 72), np.complex64))
