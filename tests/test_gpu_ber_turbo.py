"""The published turbo-code curves re-simulated with TurboEncoder / TurboDecoder, with the criteria of
tests/test_gpu_ber_reference.py (notebook_curves.evaluate: every point within 4 sigma, chi-square p >= 1e-4, BLER / BER
crossings within 0.05 dB + 3 sigma) and the MULT and MAX_WORK of tests/test_gpu_ber_conv.py:
  5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb cell 12, "Turbo Code (constraint length 4)": k = 64, n = 128,
      TurboEncoder(rate=1/2, constraint_length=4, terminate=False), TurboDecoder(enc, num_iter=8)
  Evolution_of_FEC.ipynb cell 11, "UMTS/LTE: Turbo Codes": k = 512, n = 1024 (the model's rate; the terminated codeword has
      1032 bits), TurboEncoder(rate=1/2, constraint_length=4, terminate=True), TurboDecoder(encoder=enc, num_iter=8)
  Evolution_of_FEC.ipynb cell 18, "UMTS/LTE: Turbo Codes": k = 2048, n = 6156, rate=1/3, terminate=True, num_iter=8
The tables carry the label "<dtype: 'float32'>": the reference's TurboDecoder.call prints its input's dtype
(fec/turbo/decoding.py:366) and the table extraction took that line for the legend.  All over QPSK / AWGN (the System_Model of
notebook_curves._AwgnFec).  The fourth table, cell 17 of the first notebook (c17/t4, the same encoder under ordered-statistics
decoding), runs with the model and the cost limits of tests/test_gpu_ber_osd.py.  Also runs the notebooks' turbo cell through ``install_as_sionna(tf_shim=True)``."""
import json

import numpy as np
import pytest

import notebook_curves as nc

pytestmark = pytest.mark.gpu

MULT = 2.0                    # error events per point relative to the reference's (as tests/test_gpu_ber_conv.py)
MAX_WORK = 6e10
TABLES = nc.load_tables()


def _turbo(k, n, rate, terminate):
    def build():
        phy = nc._phy()
        enc = phy.fec.turbo.TurboEncoder(rate=rate, constraint_length=4, terminate=terminate)
        dec = phy.fec.turbo.TurboDecoder(enc, num_iter=8)
        return nc._AwgnFec(k, n, 2, enc, dec)
    return build


CURVES = [
    nc.Curve(f"{nc.PVL}/c12/t5", "Turbo code K=4 (64,128), unterminated", _turbo(64, 128, 1/2, False), np.arange(0, 5, 0.5),
             bits_per_block=64, work=16.0 * 3 * 64),
    nc.Curve(f"{nc.EVO}/c11/t2", "UMTS/LTE turbo code K=4 (512,1024), terminated", _turbo(512, 1024, 1/2, True),
             np.arange(0, 8, 0.2), bits_per_block=512, cite="ipynb:304", work=16.0 * 3 * 516),
    nc.Curve(f"{nc.EVO}/c18/t1", "UMTS/LTE turbo code K=4 (2048,6156), terminated", _turbo(2048, 6156, 1/3, True),
             np.arange(-1, 1.8, 0.1), bits_per_block=2048, cite="ipynb:690", work=16.0 * 3 * 2052),
]


def test_the_tables_are_the_turbo_rows():
    """the three keys are the tables between the convolutional code and the LDPC code of their cells"""
    assert TABLES[f"{nc.PVL}/c12/t4"]["label"].startswith("Conv. Code") and f"{nc.PVL}/c12/t6" not in TABLES
    assert TABLES[f"{nc.EVO}/c11/t1"]["label"].startswith("GSM") and TABLES[f"{nc.EVO}/c11/t3"]["label"] == "5G: LDPC"
    assert TABLES[f"{nc.EVO}/c18/t0"]["label"].startswith("Uncoded") and TABLES[f"{nc.EVO}/c18/t2"]["label"] == "5G: LDPC"
    for c in CURVES:
        assert "float32" in TABLES[c.key]["label"]


@pytest.mark.parametrize("curve", CURVES, ids=[c.key for c in CURVES])
def test_turbo_curve_overlaps_reference(curve):
    ref = TABLES[curve.key]["rows"]
    ours = nc.run_curve(curve, ref, mult=MULT, max_work=MAX_WORK)
    res = nc.evaluate(curve, ref, ours)
    detail = json.dumps({k: res[k] for k in ("max_abs_z", "n_z", "n_beyond_3sigma", "chi2_p", "crossings", "points") if k in res},
                        default=float)
    print(curve.key, detail)
    assert res["n_z"] >= 2, f"{curve.name}: too few comparable points: {detail}"
    assert res["ok_points"], f"{curve.name}: a point is beyond {nc.Z_POINT} sigma of the reference: {detail}"
    assert res["ok_chi2"], f"{curve.name}: chi-square over the curve rejects agreement: {detail}"
    assert res["ok_crossings"], f"{curve.name}: Eb/N0 offset beyond 0.05 dB (+3 sigma MC): {detail}"
    if "ok_ber_crossings" in res:
        assert res["ok_ber_crossings"], f"{curve.name}: BER-curve offset beyond tolerance: {json.dumps(res['ber_crossings'], default=float)}"


def test_turbo_osd_curve_overlaps_reference():
    """5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb cell 17, c17/t4 "Turbo Code OSD-4": the unterminated rate-1/2 turbo
    encoder of cell 8 under ``OSDecoder(encoder=encoder, t=4)``, errors counted on the codeword bits.  The model, the four
    points, MULT and MAX_WORK are those of tests/test_gpu_ber_osd.py (one codeword is 679 121 candidates)."""
    import test_gpu_ber_osd as osd
    key = f"{nc.PVL}/c17/t4"
    assert TABLES[key]["label"].startswith("Turbo Code")
    curve = nc.Curve(key, "Turbo code OSD-4", osd._osd(lambda phy: phy.fec.turbo.TurboEncoder(rate=1/2, constraint_length=4, terminate=False)),
                     np.arange(0, 5, 0.5)[:osd.POINTS], bits_per_block=osd.N, work=osd.CANDIDATES, max_batch=4096, cite="cell 17")
    ref = TABLES[key]["rows"][:osd.POINTS]
    ours = nc.run_curve(curve, ref, mult=osd.MULT, max_work=osd.MAX_WORK)
    res = nc.evaluate(curve, ref, ours)
    detail = json.dumps({k: res[k] for k in ("max_abs_z", "n_z", "n_beyond_3sigma", "chi2_p", "crossings", "points") if k in res},
                        default=float)
    print(key, detail)
    assert res["n_z"] >= 2, f"too few comparable points: {detail}"
    assert res["ok_points"], f"a point is beyond {nc.Z_POINT} sigma of the reference: {detail}"
    assert res["ok_chi2"], f"chi-square over the curve rejects agreement: {detail}"
    assert res["ok_crossings"], f"Eb/N0 offset beyond 0.05 dB (+3 sigma MC): {detail}"
    if "ok_ber_crossings" in res:
        assert res["ok_ber_crossings"], f"BER-curve offset beyond tolerance: {json.dumps(res['ber_crossings'], default=float)}"


def test_notebook_turbo_cell_under_install_as_sionna():
    """the import line and the turbo code cell of 5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb (cells 2 and 8), run as
    written against ``sionna``"""
    import sionna_amd
    sionna_amd.install_as_sionna(tf_shim=True)
    ns = {}
    exec("from sionna.phy.fec.turbo import TurboEncoder, TurboDecoder\n"
         "codes_under_test = []\n"
         "enc = TurboEncoder(rate=1/2, constraint_length=4, terminate=False) # no termination used due to the rate loss\n"
         "dec = TurboDecoder(enc, num_iter=8)\n"
         "name = \"Turbo Code (constraint length 4)\"\n"
         "codes_under_test.append([enc, dec, name])\n", ns)
    enc, dec, _ = ns["codes_under_test"][0]
    import sionna.phy as sp
    u = sp.mapping.BinarySource()([100, 64])
    c = enc(u)
    assert tuple(c.shape) == (100, 128)
    assert np.array_equal(dec(20.0 * (2 * c - 1)).cpu().numpy(), u.cpu().numpy())
