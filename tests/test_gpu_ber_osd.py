"""The four published OSD curves of 5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb cell 17 ("Performance under Optimal
Decoding", n = 128, k = 64, ``OSDecoder(encoder=encoder, t=4)``) re-simulated with the criteria of
tests/test_gpu_ber_reference.py (notebook_curves.evaluate: every point within 4 sigma, chi-square p >= 1e-4, BLER / BER
crossings within 0.05 dB + 3 sigma):
  c17/t0 5G LDPC, c17/t1 5G Polar+CRC, c17/t2 Reed Muller, c17/t3 convolutional code (constraint length 8)
The cell's System_Model runs with ``cw_estimates=True``: OSD returns codeword estimates, so errors are counted on the n = 128
codeword bits (the model below).  c17/t4 needs Turbo codes and is not attempted.

Cost: one codeword is 679 120 candidates.  The four lowest Eb/N0 points (0 ... 1.5 dB) are simulated with a quarter of the
reference's block errors each (at least 200): at the reference's block error rates and with whole batches that is about
12 800 blocks = 8.7e9 candidates per curve (LDPC and Polar; 7 600 for RM, 3 000 for the conv code); MAX_WORK caps a point
at 1e10 / 679 121 blocks whatever its error rate.  Wall time per curve on one MI355X: 0.02 - 0.12 s
(profiles/osd_rate.txt).  Also runs the notebook's import line and the cell-17 construction through
``install_as_sionna(tf_shim=True)``."""
import json
import time

import numpy as np
import pytest

import notebook_curves as nc

pytestmark = pytest.mark.gpu

K, N, T = 64, 128, 4
CANDIDATES = 1 + sum(__import__("math").comb(K, i) for i in range(1, T + 1))     # 679 121 per codeword
MULT = 0.25
MAX_WORK = 1e10
POINTS = 4                                                           # 0, 0.5, 1.0, 1.5 dB
TABLES = nc.load_tables()


class _AwgnOsd(nc._AwgnFec):
    """System_Model(..., cw_estimates=True) of cell 6: the decoder's codeword estimate against the codeword"""

    def __call__(self, batch_size, ebno_db):
        phy = nc._phy()
        u = self.source([batch_size, self.k])
        c = self.encoder(u)
        no = phy.utils.ebnodb2no(ebno_db, num_bits_per_symbol=self.m, coderate=self.k / self.n)
        llr = self.demapper(self.channel(self.mapper(c), no), no)
        return c, self.decoder(llr)


def _osd(make_encoder):
    def build():
        phy = nc._phy()
        enc = make_encoder(phy)
        enc(np.zeros((1, K), np.float32))                            # the cell's dummy call: a conv encoder learns k
        return _AwgnOsd(K, N, 2, enc, phy.fec.linear.OSDecoder(encoder=enc, t=T))
    return build


def _rm(phy):
    from sionna_amd.phy.fec.polar.utils import generate_rm_code
    f, _, n, k, _ = generate_rm_code(3, 7)
    assert (k, n) == (K, N)
    return phy.fec.polar.PolarEncoder(f, n)


ENCODERS = [("5G LDPC OSD-4", lambda phy: phy.fec.ldpc.LDPC5GEncoder(k=K, n=N)),
            ("5G Polar+CRC OSD-4", lambda phy: phy.fec.polar.Polar5GEncoder(k=K, n=N)),
            ("RM OSD-4", _rm),
            ("Conv. Code OSD-4", lambda phy: phy.fec.conv.ConvEncoder(rate=1/2, constraint_length=8))]
CURVES = [nc.Curve(f"{nc.PVL}/c17/t{i}", name, _osd(mk), np.arange(0, 5, 0.5)[:POINTS], bits_per_block=N, work=CANDIDATES,
                   max_batch=4096, cite="cell 17") for i, (name, mk) in enumerate(ENCODERS)]


@pytest.mark.parametrize("curve", CURVES, ids=[c.key for c in CURVES])
def test_osd_curve_overlaps_reference(curve):
    ref = TABLES[curve.key]["rows"][:POINTS]
    t0 = time.perf_counter()
    ours = nc.run_curve(curve, ref, mult=MULT, max_work=MAX_WORK)
    wall = time.perf_counter() - t0
    blocks = sum(o["num_blocks"] for o in ours if o)
    print(f"OSD_CURVE {curve.key} {curve.name}: {blocks} blocks, {blocks * CANDIDATES:.3g} candidates, wall {wall:.2f} s")
    assert blocks * CANDIDATES <= 1.5 * MAX_WORK
    res = nc.evaluate(curve, ref, ours)
    detail = json.dumps({k: res[k] for k in ("max_abs_z", "n_z", "n_beyond_3sigma", "chi2_p", "crossings", "points") if k in res},
                        default=float)
    print("OSD_CURVE_DETAIL", curve.key, detail)
    assert res["n_z"] >= 2, f"{curve.name}: too few comparable points: {detail}"
    assert res["ok_points"], f"{curve.name}: a point is beyond {nc.Z_POINT} sigma of the reference: {detail}"
    assert res["ok_chi2"], f"{curve.name}: chi-square over the curve rejects agreement: {detail}"
    assert res["ok_crossings"], f"{curve.name}: Eb/N0 offset beyond 0.05 dB (+3 sigma MC): {detail}"
    if "ok_ber_crossings" in res:
        assert res["ok_ber_crossings"], f"{curve.name}: BER-curve offset beyond tolerance: {json.dumps(res['ber_crossings'], default=float)}"


def test_notebook_osd_cell_under_install_as_sionna():
    """the import line (cell 2) and the construction of cell 17, run as written against ``sionna``"""
    import sionna_amd
    sionna_amd.install_as_sionna(tf_shim=True)
    ns = {}
    exec("import tensorflow as tf\n"
         "from sionna.phy.fec.ldpc import LDPC5GEncoder\n"
         "from sionna.phy.fec.conv import ConvEncoder\n"
         "from sionna.phy.fec.linear import OSDecoder\n"
         "k, n = 64, 128\n"
         "decoders = []\n"
         "for encoder in (LDPC5GEncoder(k=k, n=n), ConvEncoder(rate=1/2, constraint_length=8)):\n"
         "    encoder(tf.zeros((1, k)))\n"
         "    decoder = OSDecoder(encoder=encoder, t=4)\n"
         "    decoders.append([encoder, decoder, f\" OSD-{decoder.t} \"])\n", ns)
    import sionna.phy as sp
    for enc, dec, legend in ns["decoders"]:
        assert legend == " OSD-4 " and (dec.k, dec.n) == (64, 128)
        c = enc(sp.mapping.BinarySource()([20, 64]))
        assert np.array_equal(dec(20.0 * (2 * c - 1)).cpu().numpy(), c.cpu().numpy())
