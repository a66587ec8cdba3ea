"""The precoders on the MI355X (csrc/precoding.hip): bit for bit the float32 specification of tests/precoding_f32.py, within
the bars of tests/test_oracle_ref_exec_precoding.py of both reference-executed fixtures, complex128 within 1e-10 of
oracle/precoding.py, and the defining properties of zero forcing."""
import os

import numpy as np
import pytest
import torch

import precoding_f32 as spec
from oracle import precoding as op

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "precoding_ref_golden.npz"))
MU = np.load(os.path.join(HERE, "golden", "precoding_mu_ref_golden.npz"))
TEMPLATED = [(1, 2), (1, 4), (1, 8), (1, 16), (2, 2), (2, 4), (2, 8), (2, 16), (4, 4), (4, 8), (4, 16), (8, 8), (8, 16)]
RUNTIME = [(3, 5), (16, 32)]


def phy():
    import sionna_amd.phy as p
    return p


def cn(rng, shape, dtype=np.complex64):
    return ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)).astype(dtype)


def npy(t):
    return t.as_subclass(torch.Tensor).cpu().numpy()


def close(a, b, tol):
    return a.shape == b.shape and np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1.0)


def alphas(kind, lead, rng):
    return {"zero": 0.0, "scalar": 0.25, "per_item": (0.05 + rng.random(lead)).astype(np.float32)}[kind]


@pytest.mark.parametrize("K,M", TEMPLATED + RUNTIME)
@pytest.mark.parametrize("alpha", ["zero", "scalar", "per_item"])
def test_rzf_precoder_is_the_spec_bit_for_bit(K, M, alpha):
    rng = np.random.default_rng(K * 1000 + M)
    for lead in ((7,), (1,)) if alpha != "per_item" else ((7,),):
        h, x = cn(rng, lead + (K, M)), cn(rng, lead + (K,))
        a = alphas(alpha, lead, rng)
        xp, g = phy().mimo.rzf_precoder(x, h, a, return_precoding_matrix=True)
        xs, gs = spec.rzf_precoder(x, h, a)
        assert np.array_equal(npy(g), gs) and np.array_equal(npy(xp), xs)
        assert np.array_equal(npy(phy().mimo.rzf_precoding_matrix(h, a)), gs)
        assert np.array_equal(npy(phy().mimo.rzf_precoder(x, h, a)), xs)


@pytest.mark.parametrize("K,M", TEMPLATED + RUNTIME)
def test_cbf_precoding_matrix_is_the_spec_bit_for_bit(K, M):
    h = cn(np.random.default_rng(K + 17 * M), (7, K, M))
    assert np.array_equal(npy(phy().mimo.cbf_precoding_matrix(h)), spec.precoding_matrix(h, mode="cbf"))


@pytest.mark.parametrize("K,M", [(4, 8), (3, 5)])
def test_large_batch_and_leading_dimensions(K, M):
    rng = np.random.default_rng(5)
    h, x = cn(rng, (64, 64, K, M)), cn(rng, (64, 64, K))
    a = (0.1 * rng.random((64, 64))).astype(np.float32)
    xp, g = phy().mimo.rzf_precoder(x, h, a, return_precoding_matrix=True)
    xs, gs = spec.rzf_precoder(x, h, a)
    assert np.array_equal(npy(g), gs) and np.array_equal(npy(xp), xs)
    g1 = phy().mimo.rzf_precoding_matrix(h, a[:, :1])                       # alpha broadcast over a leading dimension
    assert np.array_equal(npy(g1), spec.precoding_matrix(h, np.broadcast_to(a[:, :1], (64, 64))))


def test_zero_forcing_properties():
    h = cn(np.random.default_rng(3), (4096, 4, 8))
    g = npy(phy().mimo.rzf_precoding_matrix(h)).astype(np.complex128)
    assert np.allclose(np.sum(np.abs(g) ** 2, axis=-2), 1.0, rtol=0, atol=1e-5)   # unit-norm columns
    hg = h.astype(np.complex128) @ g
    d = np.einsum("...kk->...k", hg)
    off = hg - d[..., None] * np.eye(4)
    assert np.abs(off).max() <= 1e-5 * np.abs(d).max()                             # H G diagonal to float32 precision
    assert np.array_equal(npy(phy().mimo.rzf_precoding_matrix(np.zeros((3, 2, 4), np.complex64), 0.5)), np.zeros((3, 4, 2), np.complex64))


@pytest.mark.parametrize("K,M,alpha", [(2, 4, 0.0), (4, 8, 0.3), (3, 5, 0.1), (8, 16, 0.02)])
def test_double_precision_matches_the_complex128_oracle(K, M, alpha):
    rng = np.random.default_rng(11)
    h, x = cn(rng, (64, K, M), np.complex128), cn(rng, (64, K), np.complex128)
    xp, g = phy().mimo.rzf_precoder(x, h, alpha, return_precoding_matrix=True, precision="double")
    assert xp.dtype == torch.complex128 and g.dtype == torch.complex128
    xo, go = op.rzf_precoder(x, h, alpha)
    assert close(npy(g), go, 1e-10) and close(npy(xp), xo, 1e-10)
    gc = npy(phy().mimo.cbf_precoding_matrix(h, precision="double"))
    hc = np.conj(np.swapaxes(h, -1, -2))
    assert close(gc, hc / np.linalg.norm(hc, axis=-2, keepdims=True), 1e-12)


@pytest.mark.parametrize("i", range(5))
def test_matrix_fixture(i):
    g = {k.split("/", 1)[1]: GOLD[k] for k in GOLD.files if k.startswith(f"m{i}/")}
    xp, gm = phy().mimo.rzf_precoder(g["x"], g["h"], g["alpha"], return_precoding_matrix=True)
    assert close(npy(gm), g["g"], 2e-5) and close(npy(xp), g["x_precoded"], 2e-5)


def test_multi_user_matrix_fixture():
    for i in range(3):
        assert close(npy(phy().mimo.cbf_precoding_matrix(MU[f"cbf{i}/h"])), MU[f"cbf{i}/g"], 2e-5)
    xp, g = phy().mimo.rzf_precoder(MU["rzf/x"], MU["rzf/h"], MU["rzf/alpha"], return_precoding_matrix=True)
    assert close(npy(g), MU["rzf/g"], 2e-5) and close(npy(xp), MU["rzf/x_precoded"], 2e-5)


def _grid(fft, guards, num_tx, streams, symbols=4):
    return phy().ofdm.ResourceGrid(num_ofdm_symbols=symbols, fft_size=fft, subcarrier_spacing=15e3, num_tx=num_tx,
                                   num_streams_per_tx=streams, cyclic_prefix_length=4, num_guard_carriers=guards, dc_null=True,
                                   pilot_pattern=None)


def _ofdm_case(case):
    """(ResourceGrid, StreamManagement, x, h, alpha) of a fixture case."""
    if case == "su":
        rg = _grid(38, [3, 2], 1, 4, 14)
        sm = phy().mimo.StreamManagement(np.array([[1]]), 4)
        return rg, sm, GOLD["o/x_rg"], GOLD["o/h"], 0.2, (GOLD["o_rzf/x_precoded"], GOLD["o_rzf/h_eff"])
    g = {k.split("/", 1)[1]: MU[k] for k in MU.files if k.startswith(case + "/")}
    ntx = g["x"].shape[1]
    rg = _grid(g["x"].shape[-1], [2, 3] if case == "mu1" else [2, 2], ntx, int(g["num_streams_per_tx"]))
    sm = phy().mimo.StreamManagement(g["rx_tx_association"], int(g["num_streams_per_tx"]))
    return rg, sm, g["x"], g["h"], g["alpha"], (g["x_precoded"], g["h_eff"])


@pytest.mark.parametrize("case", ["su", "mu1", "mu2"])
def test_rzf_precoder_block_is_the_spec_and_matches_reference_execution(case):
    rg, sm, x, h, alpha, (xr, hr) = _ofdm_case(case)
    assert np.array_equal(np.asarray(rg.effective_subcarrier_ind),
                          GOLD["o/effective_subcarrier_ind"] if case == "su" else MU[f"{case}/effective_subcarrier_ind"])
    xp, he = phy().ofdm.RZFPrecoder(rg, sm, return_effective_channel=True)(x, h, alpha)
    xs, hs = spec.ofdm_rzf_precoder(x, h, sm.precoding_ind, rg.effective_subcarrier_ind, alpha)
    assert np.array_equal(npy(xp), xs) and np.array_equal(npy(he), hs)
    assert close(npy(xp), xr, 1e-4) and close(npy(he), hr, 1e-4)
    assert np.array_equal(npy(phy().ofdm.RZFPrecoder(rg, sm)(x, h, alpha)), xs)          # without the effective channel


@pytest.mark.parametrize("batch", [1, 7])
def test_two_transmitters_per_re_alpha_and_effective_channel_from_g(batch):
    """Interfering transmitters (each receiver hears both): h_eff = RemoveNulledSubcarriers(H_r G) for every receiver, with G
    the RZF matrix of the gathered intended channel - formed here with the matrix entry from the returned G."""
    rng = np.random.default_rng(batch)
    rg = _grid(21, [2, 2], 2, 2)
    sm = phy().mimo.StreamManagement(np.array([[1, 0], [0, 1]]), 2)
    x, h = cn(rng, (batch, 2, 2, 4, 21)), cn(rng, (batch, 2, 2, 2, 4, 4, 21))
    alpha = (0.05 + rng.random((batch, 2, 4, 21))).astype(np.float32)
    xp, he = phy().ofdm.RZFPrecoder(rg, sm, return_effective_channel=True)(x, h, alpha)
    xs, hs = spec.ofdm_rzf_precoder(x, h, sm.precoding_ind, rg.effective_subcarrier_ind, alpha)
    assert np.array_equal(npy(xp), xs) and np.array_equal(npy(he), hs)
    hd = np.stack([h[:, sm.precoding_ind[t, 0], :, t] for t in range(2)], 1)          # [B, tx, rxa, M, T, F]
    hd = np.transpose(hd, [0, 1, 4, 5, 2, 3])                                          # [B, tx, T, F, K, M]
    g = npy(phy().mimo.rzf_precoding_matrix(hd, alpha))                                # [B, tx, T, F, M, K]
    heff = np.einsum("brxpmtf,bptfmk->brxpktf", h.astype(np.complex128), g.astype(np.complex128))
    heff = npy(phy().ofdm.RemoveNulledSubcarriers(rg)(heff.astype(np.complex64)))
    assert close(npy(he), heff, 1e-5)
    assert np.abs(npy(he)[:, 0, :, 1]).max() > 0.1                                     # non-intended entries are there
    assert np.array_equal(npy(xp), spec.ofdm_rzf_precoder(x, h, sm.precoding_ind, rg.effective_subcarrier_ind, alpha)[0])


def test_double_precision_block_matches_the_complex128_oracle():
    rg, sm, x, h, alpha, _ = _ofdm_case("mu1")
    xp, he = phy().ofdm.RZFPrecoder(rg, sm, return_effective_channel=True, precision="double")(x, h, alpha)
    assert xp.dtype == torch.complex128
    xo, ho = op.ofdm_rzf_precoder(x, h, sm.precoding_ind, rg.effective_subcarrier_ind, alpha)
    assert close(npy(xp), xo, 1e-10) and close(npy(he), ho, 1e-10)


def test_notebook_shape_at_batch_2048():
    """8 transmit antennas, 4 streams to one 4-antenna receiver, 14 x 72 grid with guards [5, 6] and a DC null: a strided
    sample of batch entries is the specification bit for bit; the rest agrees with the complex128 oracle."""
    rg = phy().ofdm.ResourceGrid(num_ofdm_symbols=14, fft_size=72, subcarrier_spacing=15e3, num_tx=1, num_streams_per_tx=4,
                                 cyclic_prefix_length=6, num_guard_carriers=[5, 6], dc_null=True, pilot_pattern="kronecker",
                                 pilot_ofdm_symbol_indices=[2, 11])
    sm = phy().mimo.StreamManagement(np.array([[1]]), 4)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((2048, 1, 4, 14, 72), dtype=torch.complex64, device="cuda", generator=g)
    h = torch.randn((2048, 1, 4, 1, 8, 14, 72), dtype=torch.complex64, device="cuda", generator=g)
    xp, he = phy().ofdm.RZFPrecoder(rg, sm, return_effective_channel=True)(x, h)
    sample = np.arange(3, 2048, 61)
    xs, hs = spec.ofdm_rzf_precoder(x.cpu().numpy(), h.cpu().numpy(), sm.precoding_ind, rg.effective_subcarrier_ind, 0.0, batch=sample)
    assert np.array_equal(npy(xp)[sample], xs) and np.array_equal(npy(he)[sample], hs)
    assert torch.isfinite(torch.view_as_real(xp.as_subclass(torch.Tensor))).all()
