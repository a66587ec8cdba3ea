"""The two published convolutional-code curves re-simulated with ConvEncoder / ViterbiDecoder, with the criteria of
tests/test_gpu_ber_reference.py (notebook_curves.evaluate: every point within 4 sigma, chi-square p >= 1e-4, BLER / BER
crossings within 0.05 dB + 3 sigma):
  5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb cell 12, "Conv. Code Viterbi (constraint length 8)": rate 1/2, k = 64
  Evolution_of_FEC.ipynb cell 11, "GSM: Convolutional Codes": rate 1/2, K = 5, k = 512
Both cells build the code as ``ConvEncoder(rate=1/2, constraint_length=K)`` and ``ViterbiDecoder(gen_poly=enc.gen_poly,
method="soft_llr")`` over QPSK / AWGN (the System_Model of notebook_curves._AwgnFec).  Also runs the notebook's conv code
cell through ``install_as_sionna(tf_shim=True)``."""
import json

import numpy as np
import pytest

import notebook_curves as nc

pytestmark = pytest.mark.gpu

MULT = 2.0                    # error events per point relative to the reference's (as tests/test_gpu_ber_reference.py)
MAX_WORK = 6e10
TABLES = nc.load_tables()


def _conv(k, K):
    def build():
        phy = nc._phy()
        enc = phy.fec.conv.ConvEncoder(rate=1/2, constraint_length=K)
        dec = phy.fec.conv.ViterbiDecoder(gen_poly=enc.gen_poly, method="soft_llr")
        return nc._AwgnFec(k, 2 * k, 2, enc, dec)
    return build


CURVES = [
    nc.Curve(f"{nc.PVL}/c12/t4", "Conv. code Viterbi K=8 (64,128)", _conv(64, 8), np.arange(0, 5, 0.5), bits_per_block=64,
             cite="ipynb:476"),
    nc.Curve(f"{nc.EVO}/c11/t1", "GSM conv. code Viterbi K=5 (512,1024)", _conv(512, 5), np.arange(0, 8, 0.2),
             bits_per_block=512, cite="ipynb:428"),
]


@pytest.mark.parametrize("curve", CURVES, ids=[c.key for c in CURVES])
def test_conv_curve_overlaps_reference(curve):
    ref = TABLES[curve.key]["rows"]
    ours = nc.run_curve(curve, ref, mult=MULT, max_work=MAX_WORK)
    res = nc.evaluate(curve, ref, ours)
    detail = json.dumps({k: res[k] for k in ("max_abs_z", "n_z", "n_beyond_3sigma", "chi2_p", "crossings", "points") if k in res},
                        default=float)
    assert res["n_z"] >= 2, f"{curve.name}: too few comparable points: {detail}"
    assert res["ok_points"], f"{curve.name}: a point is beyond {nc.Z_POINT} sigma of the reference: {detail}"
    assert res["ok_chi2"], f"{curve.name}: chi-square over the curve rejects agreement: {detail}"
    assert res["ok_crossings"], f"{curve.name}: Eb/N0 offset beyond 0.05 dB (+3 sigma MC): {detail}"
    if "ok_ber_crossings" in res:
        assert res["ok_ber_crossings"], f"{curve.name}: BER-curve offset beyond tolerance: {json.dumps(res['ber_crossings'], default=float)}"


def test_notebook_conv_cell_under_install_as_sionna():
    """the import line and the conv code cell of 5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb (cells 2 and 8), run as
    written against ``sionna``"""
    import sionna_amd
    sionna_amd.install_as_sionna(tf_shim=True)
    ns = {}
    exec("from sionna.phy.fec.conv import ConvEncoder, ViterbiDecoder\n"
         "codes_under_test = []\n"
         "enc = ConvEncoder(rate=1/2, constraint_length=8)\n"
         "dec = ViterbiDecoder(gen_poly=enc.gen_poly, method=\"soft_llr\")\n"
         "name = \"Conv. Code Viterbi (constraint length 8)\"\n"
         "codes_under_test.append([enc, dec, name])\n", ns)
    enc, dec, _ = ns["codes_under_test"][0]
    import sionna.phy as sp
    u = sp.mapping.BinarySource()([100, 64])
    c = enc(u)
    assert tuple(c.shape) == (100, 128)
    assert np.array_equal(dec(20.0 * (2 * c - 1)).cpu().numpy(), u.cpu().numpy())
