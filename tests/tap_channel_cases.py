"""Inputs of the tap-generator edge tests (TDL, CDL): named cases shared by the CPU tests (tests/test_tap_channel_host.py, on the NumPy
models of tests/kernel_models.py) and the GPU tests (tests/test_gpu_tap_channel_edges.py).  Small, seeded, no full product: every
value of every axis appears at least once, and every LoS model meets every T edge.

Which case reaches which branch.

``tdl_cir_kernel`` (chunks of 16 steps, draws in registers up to N = 24):
  N <= 24 (register draws)             every case but N25 / N40 and the *n25 ones
  N > 24 (draws per chunk)             N25, N40, A_n25_b1, E_n40, aoa2_n25, still_n25, high_n25, D_T200_n25, second_A_n25, and all float64 N = 25
  one short chunk only                 *_T1, *_T15
  one full chunk, no tail              *_T16          kmax = 16, nothing re-anchored
  re-anchoring at t0 = 16              *_T17 (tail of 1), *_T32 (two full chunks), *_T33 (two full and a tail of 1)
  re-anchoring 12 times, tail of 8     *_T200
  LoS term, default angle              D_*, E_*;  other angles: aoa0 (cos = 1), aoa2 and aoa2_n25 (cos < 0)
  no LoS                               A_*, C_*
  a block that is not full             every B = 1 case: E_* has 14 live threads of 256, A_* 23; B RA TA P never a multiple of 256
  more than one block                  D_* at B = 7, (3, 5): 7 * 15 * 13 = 1365 threads
  doppler = 0                          still, still_n25: every step equals the first, w = 0
  arguments of ~1e3 rad                high, high_n25 (150 m/s at 28 GHz, fs = 1 kHz, t = 32 ms): the bound scales with |d t|
  the stream continues                 second_D, second_A_n25: call index 4

``tdl_cir128_kernel``: one lane per output, T = 1 / 17 / 200 x N = 20 / 25 on model D, (3, 5).

``cdl_cir_kernel`` (one thread per (b, u, s, cluster), blocks of 128, chunks of 16 steps of which the tail is not stored):
  LoS term                             D_*, E_* (both directions);  none: A_*, B_*, C_*
  T not a multiple of 16               T = 1, 15, 17, 33;  exactly one chunk: T = 16
  a block that is not full             siso at B = 1: model A 23 live threads, D 13, E 14
  several blocks, a partial last one   mimo (2 x 8) and panel (32 x 2 or 2 x 32) pairs
  uplink / downlink                    swaps the arrays, the tables' sides and the LoS angles
  orientation                          "rot": all three angles non-zero at both ends (psi and the LCS angles of the field tables)
  speed 0 (w = 0), fixed, drawn        still / v30 / 3 ... 30
  Doppler phases of hundreds of rad    high_*: fs = 1 kHz, 30 m/s at 3.5 GHz, t = 32 ms: |w t| up to 70 rad ... the w t term dominates
  the stream continues                 second_*: call index 8
"""
import collections

import numpy as np

FS_SYMBOL = 1 / 71.4e-6            # one sample per OFDM symbol, as the link-level chains use the generators
FS_SLOW = 1e3
DELAY_SPREAD = 300e-9

Tdl = collections.namedtuple("Tdl", "name model t n ra ta b speeds fc fs aoa call prec")


def _t(name, model="D", t=17, n=20, ant=(3, 5), b=7, speeds=(3.0, 30.0), fc=2.6e9, fs=FS_SYMBOL, aoa=np.pi / 4, call=0, prec="single"):
    return Tdl(name, model, t, n, ant[0], ant[1], b, speeds, fc, fs, aoa, call, prec)


T_EDGES = (1, 15, 16, 17, 32, 33, 200)
TDL = (
    [_t(f"D_T{t}", t=t) for t in T_EDGES]
    + [_t(f"E_T{t}", model="E", t=t, ant=(1, 1), b=1) for t in T_EDGES]
    + [_t("A_T17", model="A", t=17, ant=(1, 1), b=1), _t("A_T200", model="A", t=200, ant=(3, 5), b=1),
       _t("C_T33", model="C", t=33), _t("C_T16", model="C", t=16, ant=(1, 1), b=7)]
    + [_t(f"N{n}", t=33, n=n) for n in (1, 2, 24, 25, 40)]
    + [_t("A_n25_b1", model="A", t=33, n=25, ant=(1, 1), b=1), _t("E_n40", model="E", t=17, n=40, b=1),
       _t("D_T200_n25", t=200, n=25, b=1), _t("D_T200_n2_slow", t=200, n=2, b=7, ant=(1, 1), speeds=(0.01, 0.05))]
    + [_t("aoa0", aoa=0.0), _t("aoa2", aoa=2.0, t=33), _t("aoa2_n25", aoa=2.0, n=25)]
    + [_t("still", t=33, speeds=(0.0, 0.0)), _t("still_n25", n=25, speeds=(0.0, 0.0), b=1)]
    + [_t("high", t=33, speeds=(150.0, 150.0), fc=28e9, fs=FS_SLOW), _t("high_n25", t=33, n=25, speeds=(150.0, 150.0), fc=28e9, fs=FS_SLOW, b=1)]
    + [_t("second_D", call=4), _t("second_A_n25", model="A", t=33, n=25, call=4, b=1)]
)
TDL64 = [_t(f"f64_T{t}_N{n}", t=t, n=n, b=2, prec="double") for t in (1, 17, 200) for n in (20, 25)]
TDL_BY_NAME = {c.name: c for c in TDL + TDL64}
TDL_STANDARD = _t("standard", model="A", t=14, ant=(4, 2), b=64)       # tests/test_gpu_ofdm.py::test_tdl_matches_oracle_and_statistics


def tdl_object(mod, case, **kw):
    """the public class (``mod`` = sionna_amd.phy.channel.tr38901) for a case; constructing it touches no device"""
    return mod.TDL(case.model, DELAY_SPREAD, case.fc, num_sinusoids=case.n, los_angle_of_arrival=case.aoa, min_speed=case.speeds[0],
                   max_speed=case.speeds[1], num_rx_ant=case.ra, num_tx_ant=case.ta, precision=case.prec, **kw)


def tdl_args(tdl, case, seed, call=None, batch=None):
    """positional / keyword arguments shared by ``tdl_f32.anchor_and_bound``, ``kernel_models.tdl_cir_model`` and (with the delays
    inserted) ``oracle.ofdm.tdl_cir``"""
    return (seed, case.call if call is None else call, case.b if batch is None else batch, case.t, case.fs, tdl._mean_powers,
            tdl._min_doppler, tdl._max_doppler), dict(num_rx_ant=case.ra, num_tx_ant=case.ta, num_sinusoids=case.n,
                                                       los_power=tdl._los_power if tdl.los else None, los_aoa=case.aoa)


def corr_matrices(ra, ta):
    """Hermitian positive definite receive / transmit correlation matrices (exponential model with a complex coefficient)"""
    def expo(n, rho):
        i = np.arange(n)
        m = np.abs(rho) ** np.abs(i[:, None] - i[None, :]) * np.exp(1j * np.angle(rho) * (i[:, None] - i[None, :]))
        return m
    return expo(ra, 0.7 * np.exp(0.4j)), expo(ta, 0.5 * np.exp(-1.1j))


# ------------------------------------------------------------------ CDL
FC_CDL = 3.5e9
ROT = ([0.4, 0.1, -0.2], [0.1, 0.2, 0.05])           # (ut, bs): bearing, downtilt, slant all non-zero at both ends
Cdl = collections.namedtuple("Cdl", "name model direction kind t b orient speeds fs call prec")


def _c(name, model="A", direction="downlink", kind="mimo", t=17, b=3, orient=None, speeds=(3.0, 30.0), fs=15e3 * 14, call=0, prec="single"):
    return Cdl(name, model, direction, kind, t, b, orient, speeds, fs, call, prec)


def cdl_arrays(mod, kind):
    """(ut_array, bs_array) from ``mod`` = sionna_amd.phy.channel.tr38901 or oracle.cdl"""
    if kind == "siso":
        return mod.Antenna("single", "V", "omni", FC_CDL), mod.Antenna("single", "V", "omni", FC_CDL)
    if kind == "mimo":
        return mod.Antenna("dual", "cross", "omni", FC_CDL), mod.AntennaArray(2, 2, "dual", "cross", "38.901", FC_CDL)
    assert kind == "panel"
    return mod.Antenna("dual", "VH", "omni", FC_CDL), mod.PanelArray(4, 4, "dual", "cross", "38.901", FC_CDL)


CDL = (
    [_c(f"D_T{t}", model="D", t=t, direction="downlink" if i % 2 else "uplink", kind=("siso", "mimo", "panel")[i % 3], b=1 if i % 3 == 0 else 3)
     for i, t in enumerate((1, 15, 16, 17, 33))]
    + [_c(f"E_T{t}", model="E", t=t, direction="uplink" if i % 2 else "downlink", kind=("mimo", "panel", "siso")[i % 3], b=1 if i % 3 == 2 else 3)
       for i, t in enumerate((1, 15, 16, 17, 33))]
    + [_c("A_siso_b1", kind="siso", b=1, t=17), _c("A_siso_T1", kind="siso", b=1, t=1, direction="uplink"),
       _c("A_panel_T16", kind="panel", t=16), _c("A_mimo_T33", t=33, direction="uplink"),
       _c("B_mimo_T15", model="B", t=15), _c("B_panel_T17_up", model="B", kind="panel", direction="uplink", b=1),
       _c("C_mimo_T33", model="C", t=33, direction="uplink"), _c("C_siso_T16", model="C", kind="siso", t=16)]
    + [_c("rot_A", orient=ROT, t=17), _c("rot_D_up", model="D", orient=ROT, direction="uplink", t=33),
       _c("rot_E_panel", model="E", orient=ROT, kind="panel", t=15, b=1)]
    + [_c("still_B", model="B", speeds=(0.0, None), t=33), _c("still_D", model="D", speeds=(0.0, None), t=17, kind="siso", b=1),
       _c("v30_C", model="C", speeds=(30.0, None), t=17), _c("v30_E_up", model="E", speeds=(30.0, 30.0), direction="uplink", t=16)]
    + [_c("high_A", speeds=(30.0, None), fs=FS_SLOW, t=33), _c("high_D", model="D", speeds=(30.0, None), fs=FS_SLOW, t=33, direction="uplink")]
    + [_c("second_A", call=8), _c("second_D_panel", model="D", kind="panel", call=8, t=33, b=1)]
)
CDL64 = [_c(f"f64_{m}_T{t}", model=m, kind="panel", t=t, b=2, prec="double", direction="downlink" if t == 1 else "uplink")
         for m in ("B", "D") for t in (1, 17)]
CDL_BY_NAME = {c.name: c for c in CDL + CDL64}
CDL_STANDARD = _c("standard", model="A", kind="mimo", direction="uplink", t=14, b=33)     # tests/test_gpu_cdl.py::test_cdl_vs_oracle


def cdl_kwargs(case):
    uo, bo = case.orient if case.orient is not None else (None, None)
    return dict(ut_orientation=uo, bs_orientation=bo, min_speed=case.speeds[0], max_speed=case.speeds[1])
