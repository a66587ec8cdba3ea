"""Downlink BLER of MIMO_OFDM_Transmissions_over_CDL.ipynb cell 70 (8-antenna base station precoding 4 streams with
RZFPrecoder (alpha = 0: zero forcing) to a 4-antenna terminal over CDL-A..E, perfect CSI = the effective channel the
precoder returns, LMMSE equaliser, QPSK, 5G LDPC rate 1/2) against the notebook's published tables, with the criteria of
tests/test_gpu_ber_reference.py (notebook_curves.evaluate: every point within 4 sigma, chi-square p >= 1e-4, BLER / BER
crossings within 0.05 dB + 3 sigma).  The uplink model of notebook_curves is reused with the downlink CDL and the precoder
inserted before ApplyOFDMChannel, as the notebook's Model (cell 65) does for direction="downlink"."""
import json

import numpy as np
import pytest

import notebook_curves as nc

pytestmark = pytest.mark.gpu

MULT = 2.0                    # error events per point relative to the reference's (as tests/test_gpu_ber_reference.py)
MAX_WORK = 6e10              # the bound of tests/test_gpu_ber_reference.py; the five tables take seconds on the MI355X
TABLES = nc.load_tables()


class _DownlinkCdlModel(nc._CdlModel):
    """Cell 65 ``Model`` with direction="downlink", domain="freq", perfect CSI (ipynb cell 70)."""

    def __init__(self, cdl_model):
        super().__init__("freq", cdl_model, True, 0.0, 6, [2, 11])
        phy = nc._phy()
        t = phy.channel.tr38901
        arr = lambda n: t.AntennaArray(num_rows=1, num_cols=n // 2, polarization="dual", polarization_type="cross",
                                       antenna_pattern="38.901", carrier_frequency=self.fc)
        self.cdl = t.CDL(model=cdl_model, delay_spread=100e-9, carrier_frequency=self.fc, ut_array=arr(self.n_ut),
                         bs_array=arr(self.n_bs), direction="downlink", min_speed=0.0)
        self.precoder = phy.ofdm.RZFPrecoder(self.rg, self.sm, return_effective_channel=True)

    def __call__(self, batch_size, ebno_db):
        phy = nc._phy()
        rg = self.rg
        no = phy.utils.ebnodb2no(ebno_db, self.m, self.coderate, rg)
        b = self.source([batch_size, 1, self.n_ut, self.k])
        x_rg = self.rg_mapper(self.mapper(self.encoder(b)))
        a, tau = self.cdl(batch_size, rg.num_ofdm_symbols, 1 / rg.ofdm_symbol_duration)
        h_freq = phy.channel.cir_to_ofdm_channel(self.freqs, a, tau, normalize=True)   # [B, 1, 4, 1, 8, T, F]
        x_rg, h_eff = self.precoder(x_rg, h_freq)
        y = self.channel_freq(x_rg, h_freq, no)
        x_hat, no_eff = self.lmmse(y, h_eff, 0.0, no)
        return b, self.decoder(self.demapper(x_hat, no_eff))


CURVES = [nc.Curve(f"MIMO_OFDM_Transmissions_over_CDL/c70/t{i}", f"8x4 downlink CDL-{mdl}, ZF precoding, perfect CSI, LMMSE, QPSK LDPC r=1/2",
                   (lambda mdl=mdl: _DownlinkCdlModel(mdl)), np.arange(-5, 20, 4.0), bits_per_block=768, corr=4.0, group="cdl",
                   max_batch=4096, cite="ipynb:2009-2060")
          for i, mdl in enumerate("ABCDE")]


def test_downlink_model_shapes():
    m = _DownlinkCdlModel("C")
    b, b_hat = m(8, 10.0)
    assert tuple(b.shape) == (8, 1, 4, m.k) and tuple(b_hat.shape) == tuple(b.shape)


@pytest.mark.parametrize("curve", CURVES, ids=[c.key for c in CURVES])
def test_downlink_curve_overlaps_reference(curve):
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
