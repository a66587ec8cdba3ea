"""The precoded channels (csrc/precoding.hip) and the post-equalisation SINR (csrc/post_eq_sinr.hip) on the MI355X: bit for
bit the specification of tests/precoded_channel_f32.py in complex64 and complex128, within the bars measured from the
reference itself of the reference-executed fixture, the launch edges, and consistency with RZFPrecoder's effective channel
and with the helper-method composition."""
import os

import numpy as np
import pytest
import torch

import precoded_channel_f32 as spec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "precoded_channel_ref_golden.npz"))
CASES = [str(c) for c in FIX["cases"]]
PRECISIONS = [("single", np.float32), ("double", np.float64)]
SINR_TEMPLATED = [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4)]
SINR_RUNTIME = [(3, 2), (5, 3), (16, 16)]


def phy():
    import sionna_amd.phy as p
    return p


def npy(t):
    return t.as_subclass(torch.Tensor).cpu().numpy()


def cn(rng, shape):
    return ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)).astype(np.complex64)


def grid(num_tx, streams, symbols=2):
    return phy().ofdm.ResourceGrid(num_ofdm_symbols=symbols, fft_size=16, subcarrier_spacing=15e3, num_tx=num_tx,
                                   num_streams_per_tx=streams, cyclic_prefix_length=2, num_guard_carriers=[2, 1], dc_null=True,
                                   pilot_pattern=None)


def families(name):
    return ["eye"] if name == "eye" else ["rzf", "cbf"]


_CACHE = {}


def case(name):
    """(fixture entries, ResourceGrid, StreamManagement) of a fixture case, built once"""
    if name not in _CACHE:
        g = {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.startswith(name + "/")}
        sm = phy().mimo.StreamManagement(g["rx_tx_association"], int(g["num_streams_per_tx"]))
        rg = grid(sm.num_tx, sm.num_streams_per_tx)
        assert np.array_equal(np.asarray(rg.effective_subcarrier_ind), g["effective_subcarrier_ind"]) and len(g["effective_subcarrier_ind"]) == 12
        _CACHE[name] = (g, rg, sm)
    return _CACHE[name]


def run(fam, rg, sm, h, p, h_hat=None, alpha=0., precision="single"):
    o = phy().ofdm
    if fam == "eye":
        return npy(o.EyePrecodedChannel(rg, sm, precision=precision)(h, p))
    if fam == "cbf":
        return npy(o.CBFPrecodedChannel(rg, sm, precision=precision)(h, p, h_hat=h_hat))
    return npy(o.RZFPrecodedChannel(rg, sm, precision=precision)(h, p, h_hat=h_hat, alpha=alpha))


def spec_h_eff(fam, g, rg, sm, dtype, **over):
    a = dict(h=g["h"], p=g["tx_power"], h_hat=g.get("h_hat"), alpha=g.get("alpha", 0.))
    a.update(over)
    return spec.precoded_channel(a["h"], a["p"], sm.precoding_ind, rg.effective_subcarrier_ind, fam, h_hat=a["h_hat"],
                                 alpha=a["alpha"], dtype=dtype)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("name", CASES)
def test_precoded_channel_is_the_spec_bit_for_bit_and_within_the_bars_of_the_fixture(name, precision, dtype):
    """su / mu4 (square) / mu8 / mc (h_hat != h, U > 0) / rt (run-time sizes) / s3 / eye; alpha 0, scalar, [B] and full;
    tx_power of rank 0, 2, 3 (one stream at power 0) and 5; RZF and CBF"""
    g, rg, sm = case(name)
    for fam in families(name):
        he = run(fam, rg, sm, g["h"], g["tx_power"], g.get("h_hat"), g.get("alpha", 0.), precision)
        assert he.dtype == (np.complex64 if dtype is np.float32 else np.complex128)
        assert np.array_equal(he, spec_h_eff(fam, g, rg, sm, dtype)), (name, fam)
        dev, bar = spec.rel_dev(he, g[f"h_eff_{fam}64"]), (spec.bar32 if dtype is np.float32 else spec.bar64)(fam)
        print(name, fam, precision, f"deviation from the reference's double result {dev:.3e}, bar {bar:.3e}")
        assert dev <= bar, (name, fam, dev, bar)
    if name == "mu8":
        assert np.all(he[:, :, :, :, 2] == 0)                                    # the stream without power


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha_kind", ["zero", "scalar", "batch", "full"])
def test_rzf_alpha_forms(alpha_kind, precision, dtype):
    g, rg, sm = case("mu8")                                                      # K = 4 < M = 8: alpha = 0 is well conditioned
    rng = np.random.default_rng(3)
    alpha = {"zero": 0.0, "scalar": 0.3, "batch": (0.05 + rng.random(3)).astype(np.float32),
             "full": (0.05 + rng.random((3, 1, 2, 16))).astype(np.float32)}[alpha_kind]
    he = run("rzf", rg, sm, g["h"], g["tx_power"], None, alpha, precision)
    assert np.array_equal(he, spec_h_eff("rzf", g, rg, sm, dtype, alpha=alpha))


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("rank", [0, 1, 2, 3, 4, 5])
def test_tx_power_of_every_rank_with_a_stream_at_power_zero(rank, precision, dtype):
    g, rg, sm = case("mc")
    full = (0.25 + np.random.default_rng(rank).random((3, 2, 4, 2, 16))).astype(np.float32)
    full[:, :, 1] = 0.0
    p = np.float32(0.5) if rank == 0 else np.ascontiguousarray(full[(slice(None),) * rank + (0,) * (5 - rank)])
    for fam in ("rzf", "cbf"):
        he = run(fam, rg, sm, g["h"], p, g["h_hat"], g["alpha"], precision)
        assert np.array_equal(he, spec_h_eff(fam, g, rg, sm, dtype, p=p))
        if rank >= 3:
            assert np.all(he[:, :, :, :, 1] == 0) and np.abs(he[:, :, :, :, 0]).min() > 0


def test_h_hat_only_shapes_the_precoder():
    """G comes from h_hat, the effective channel from the true h: both orders differ from each other and from h_hat = h"""
    g, rg, sm = case("mc")
    a = run("rzf", rg, sm, g["h"], g["tx_power"], g["h_hat"], g["alpha"])
    b = run("rzf", rg, sm, g["h_hat"], g["tx_power"], g["h"], g["alpha"])
    c = run("rzf", rg, sm, g["h"], g["tx_power"], None, g["alpha"])
    assert np.array_equal(c, run("rzf", rg, sm, g["h"], g["tx_power"], g["h"], g["alpha"]))
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(b, spec_h_eff("rzf", g, rg, sm, np.float32, h=g["h_hat"], h_hat=g["h"]))


def sinr(rg, sm, h_eff, no, h_eff_hat=None, whitening=True, precision="single"):
    return npy(phy().ofdm.LMMSEPostEqualizationSINR(rg, sm, precision=precision)(h_eff, no, h_eff_hat=h_eff_hat,
                                                                                 interference_whitening=whitening))


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("whitening", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_sinr_is_the_spec_bit_for_bit_and_within_the_bars_of_the_fixture(name, whitening, precision, dtype):
    """on the fixture's h_eff: no of rank 0 (su, rt), 1 (mu4, s3), 2 (eye), 3 (mu8) and 5 (mc); U = 0 (su, s3, eye) and
    U > 0; an estimated h_eff (mc); the run-time path (s3: 3 antennas, 3 streams)"""
    g, rg, sm = case(name)
    fam, tag = ("sinr_whitened", "w") if whitening else ("sinr_unwhitened", "u")
    bar = (spec.bar32 if dtype is np.float32 else spec.bar64)(fam)
    h_eff = g[f"h_eff_{families(name)[0]}32"]
    for hat in ([None, g["h_eff_hat"]] if "h_eff_hat" in g else [None]):
        s = sinr(rg, sm, h_eff, g["no"], hat, whitening, precision)
        assert s.dtype == dtype and s.shape == (3, 2, 12, sm.num_rx, sm.num_streams_per_rx)
        want = spec.lmmse_post_eq_sinr(h_eff if hat is None else hat, g["no"], sm.detection_desired_ind,
                                       sm.detection_undesired_ind, whitening, dtype=dtype)
        assert np.array_equal(s, want), (name, whitening)
        dev = spec.rel_dev(s, g[f"sinr_{'' if hat is None else 'hat_'}{tag}64"])
        print(name, fam, precision, f"deviation from the reference's double result {dev:.3e}, bar {bar:.3e}")
        assert dev <= bar, (name, fam, dev, bar)
    if name == "mu8":
        assert np.all(s[:, :, :, 2, 0] == 0) and np.all(s[:, :, :, 0, 0] > 0)      # the stream without power: exactly 0
    if name in ("su", "s3", "eye"):
        assert sm.num_interfering_streams_per_rx == 0
    if name == "mc":
        assert sm.num_interfering_streams_per_rx == 6


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("rank", [0, 1, 2, 3, 4, 5])
def test_sinr_no_of_every_rank(rank, precision, dtype):
    g, rg, sm = case("mc")
    full = (0.01 + np.random.default_rng(rank).random((3, 4, 2, 2, 12))).astype(np.float32)
    no = np.float32(0.2) if rank == 0 else np.ascontiguousarray(full[(slice(None),) * rank + (0,) * (5 - rank)])
    s = sinr(rg, sm, g["h_eff_rzf32"], no, precision=precision)
    assert np.array_equal(s, spec.lmmse_post_eq_sinr(g["h_eff_rzf32"], no, sm.detection_desired_ind, sm.detection_undesired_ind,
                                                     True, dtype=dtype))


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("rxa,s", SINR_TEMPLATED + SINR_RUNTIME)
def test_sinr_every_compiled_size_and_the_run_time_path(rxa, s, precision, dtype):
    """two transmitters with s streams each towards two receivers with rxa antennas: S = s desired and U = s interfering
    streams per receiver, on a random effective channel"""
    rng = np.random.default_rng(100 * rxa + s)
    sm = phy().mimo.StreamManagement(np.array([[1, 0], [0, 1]]), s)
    rg = grid(2, s)
    h_eff, no = cn(rng, (3, 2, rxa, 2, s, 2, 12)), (0.01 + rng.random((3, 2, rxa))).astype(np.float32)
    for whitening in (True, False):
        got = sinr(rg, sm, h_eff, no, whitening=whitening, precision=precision)
        assert np.array_equal(got, spec.lmmse_post_eq_sinr(h_eff, no, sm.detection_desired_ind, sm.detection_undesired_ind,
                                                           whitening, dtype=dtype)), (rxa, s, whitening)
        assert np.all(np.isfinite(got)) and np.all(got > 0)


@pytest.mark.parametrize("nrx,m", [(3, 5), (4, 8)])
@pytest.mark.parametrize("batch", [0, 1, 11])
def test_launch_edges_batch_sizes(batch, nrx, m):
    """an empty batch, one entry, and item counts that are no multiple of the block of 128 lanes (batch 1: 32 items of the
    precoded channel and 24 nrx of the SINR; batch 11: 352 and 264 nrx, more than one block), on the run-time-size path
    (3 receivers, 5 antennas) and on a compiled one (4 receivers, 8 antennas)"""
    rng = np.random.default_rng(batch)
    sm, rg = phy().mimo.StreamManagement(np.ones((nrx, 1), int), nrx), grid(1, nrx)
    h, p = cn(rng, (batch, nrx, 1, 1, m, 2, 16)), (0.25 + rng.random((batch, 1, nrx))).astype(np.float32)
    no = (0.01 + rng.random((batch, nrx))).astype(np.float32)
    assert (batch * 2 * 16) % 128 != 0 and (batch * nrx * 24) % 128 != 0 or batch == 0
    for fam in ("rzf", "cbf"):
        he = run(fam, rg, sm, h, p, alpha=0.1)
        assert he.shape == (batch, nrx, 1, 1, nrx, 2, 12)
        assert np.array_equal(he, spec.precoded_channel(h, p, sm.precoding_ind, rg.effective_subcarrier_ind, fam, alpha=0.1))
    s = sinr(rg, sm, he, no)
    assert s.shape == (batch, 2, 12, nrx, 1)
    assert np.array_equal(s, spec.lmmse_post_eq_sinr(he, no, sm.detection_desired_ind, sm.detection_undesired_ind))


def test_launch_edges_non_contiguous_views():
    g, rg, sm = case("mc")
    dev = torch.device("cuda")
    h2 = torch.zeros((3, 4, 2, 2, 8, 2, 32), dtype=torch.complex64, device=dev)
    h2[..., ::2] = torch.from_numpy(g["h"]).to(dev)
    hh2 = torch.from_numpy(np.ascontiguousarray(np.swapaxes(g["h_hat"], 1, 2))).to(dev).transpose(1, 2)
    p2 = torch.from_numpy(np.ascontiguousarray(np.swapaxes(g["tx_power"], 0, 1))).to(dev).transpose(0, 1)
    assert not h2[..., ::2].is_contiguous() and not hh2.is_contiguous() and not p2.is_contiguous()
    he = npy(phy().ofdm.RZFPrecodedChannel(rg, sm)(h2[..., ::2], p2, h_hat=hh2, alpha=g["alpha"]))
    assert np.array_equal(he, spec_h_eff("rzf", g, rg, sm, np.float32))
    e2 = torch.from_numpy(np.ascontiguousarray(np.swapaxes(he, 5, 6))).to(dev).transpose(5, 6)
    n2 = torch.from_numpy(np.ascontiguousarray(np.swapaxes(g["no"], 3, 4))).to(dev).transpose(3, 4)
    assert not e2.is_contiguous() and not n2.is_contiguous()
    s = npy(phy().ofdm.LMMSEPostEqualizationSINR(rg, sm)(e2, n2))
    assert np.array_equal(s, spec.lmmse_post_eq_sinr(he, g["no"], sm.detection_desired_ind, sm.detection_undesired_ind))


@pytest.mark.parametrize("name", ["su", "mu4", "mc", "rt"])
def test_unit_power_equals_the_effective_channel_of_rzf_precoder(name):
    """tx_power 1 and h_hat = None: the h_eff of RZFPrecoder(return_effective_channel=True), bit for bit (RZFPrecoder
    expands alpha with leading dimensions, so a scalar and a full alpha are compared)"""
    g, rg, sm = case(name)
    rng = np.random.default_rng(7)
    x = cn(rng, (3, sm.num_tx, sm.num_streams_per_tx, 2, 16))
    for alpha in (0.2, (0.05 + rng.random((3, sm.num_tx, 2, 16))).astype(np.float32)):
        _, want = phy().ofdm.RZFPrecoder(rg, sm, return_effective_channel=True)(x, g["h"], alpha)
        for p in (1.0, np.ones((3, sm.num_tx, sm.num_streams_per_tx, 2, 16), np.float32)):
            assert np.array_equal(run("rzf", rg, sm, g["h"], p, None, alpha), npy(want))


@pytest.mark.parametrize("name", ["mu8", "mc", "eye"])
def test_helper_method_composition_agrees_with_the_fused_launches(name):
    """a user's subclass composes its call from the public helpers, as the reference's subclasses do: the same result within
    the float32 bars"""
    g, rg, sm = case(name)
    p, o = phy(), phy().ofdm
    fam = families(name)[0]

    class HelperChannel(o.PrecodedChannel):
        def call(self, h, tx_power, h_hat=None, alpha=0.):
            if fam == "eye":
                b, _, _, ntx, m, t, f = h.shape
                gm = torch.eye(m, dtype=self.cdtype, device=h.device).expand(b, ntx, t, f, m, m)
            else:
                hd = self.get_desired_channels(h if h_hat is None else h_hat)
                a = torch.as_tensor(alpha, device=h.device)
                gm = p.mimo.rzf_precoding_matrix(hd, a.reshape(tuple(a.shape) + (1,) * (4 - a.dim())).expand(hd.shape[:4]))
            return self.compute_effective_channel(h, self.apply_tx_power(gm, tx_power))

    class HelperSINR(o.PostEqualizationSINR):
        def call(self, h_eff, no, h_eff_hat=None, interference_whitening=True):
            b, rx, rxa, _, _, t, fe = h_eff.shape
            no = no.reshape(tuple(no.shape) + (1,) * (5 - no.dim())).expand(b, rx, rxa, t, fe).permute(0, 1, 3, 4, 2)
            hd, hu = self.get_per_rx_channels(h_eff if h_eff_hat is None else h_eff_hat)
            s = self.compute_interference_covariance_matrix(no=no, h_eff_undesired=hu if interference_whitening else None)
            l_inv = p.utils.inv_cholesky(s.contiguous())
            hd, hu = torch.matmul(l_inv, hd), torch.matmul(l_inv, hu)
            return self.compute_sinr(hd, hu, torch.ones_like(no), p.mimo.lmmse_matrix(hd.contiguous()))

    kw = {} if fam == "eye" else dict(h_hat=g.get("h_hat"), alpha=g.get("alpha", 0.))
    he = npy(HelperChannel(rg, sm)(g["h"], g["tx_power"], **kw))
    fused = run(fam, rg, sm, g["h"], g["tx_power"], g.get("h_hat"), g.get("alpha", 0.))
    dev = spec.rel_dev(he, fused)
    print(name, fam, f"helpers against the fused launch {dev:.3e}, bar {spec.bar32(fam):.3e}")
    assert dev <= spec.bar32(fam)
    for whitening, sfam in ((True, "sinr_whitened"), (False, "sinr_unwhitened")):
        s = npy(HelperSINR(rg, sm)(fused, torch.from_numpy(g["no"]).cuda(), interference_whitening=whitening))
        dev = spec.rel_dev(s, sinr(rg, sm, fused, g["no"], whitening=whitening))
        print(name, sfam, f"helpers against the fused launch {dev:.3e}, bar {spec.bar32(sfam):.3e}")
        assert dev <= spec.bar32(sfam)
