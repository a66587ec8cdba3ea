"""Inputs of the time-domain channel edge tests: named cases shared by the CPU tests (tests/test_time_channel_host.py, on the
NumPy models of tests/kernel_models.py) and the GPU tests (tests/test_gpu_time_channel_edges.py), seeded and small.

Layout: batch 2, two receivers, two transmitters - tau is indexed by (b, rx, tx) and the taps by the full link, so a wrong stride
shows at every shape.  Delays are distinct per (b, rx, tx, p); path amplitudes fall by 40 dB of power over the paths (one path:
none), so that a weak tap matters.

cir_to_time_channel (``CIR``): what each family reaches in ``cir_to_time_kernel``
  L*     L = 1, 8, 9, 10, 18, 19, 27, 31 at T = 65: register tiles of 9 lags under the l0 + j < L guard, full and tail tiles
  T*     T = 1, 63, 64, 65, 255, 256, 257, 513 at L = 10: wave passes of 64 and block passes of 256 time steps, the partial pass
  P*     P = 1, 2, 23 with P L odd and even: the sinc table is padded to an even count before the float2 stage
  ant*   (RA, TA) = (1, 1), (2, 1), (1, 2), (2, 2): link addressing; the stage is reused from link to link
  tdl    W = 30.72 MHz, delays up to 3 us (|tau W| up to 92): the regime where the argument term is most of the bound
  tau0, tauint   tau = 0, and tau W an integer exactly (W = 2^23 Hz, tau = k 2^-23 s): weights exactly 1 and 0 in the anchor
  zero   one link without energy among live ones
  lds*   L = 31: P = 8 (below 64 KiB with the static 1 KiB), 9 and 16 (above), 801 (the largest the entry accepts); 802 is refused
All of them |tau W| <= 8 unless said otherwise (the tight regime).  Every case runs with ``normalize`` off, on, and deferred.

ApplyTimeChannel (``APPLY``): (Tn, L) = (1, 1), (1, 8), (3, 32), (7, 8) - Tn < L: both window clips active at once, L = 32 the
largest stage - and (248, 8), (249, 8), (250, 8), (506, 8): Tout = 255, 256, 257, 513, the block edges.  (TX, TA), (RX, RA) up to
(2, 2); with and without ``link_scale``, one link's scale 0."""
import collections

import numpy as np

BATCH, NUM_RX, NUM_TX = 2, 2, 2
W_TIGHT = 7.68e6
W_TDL = 30.72e6
W_INT = float(2 ** 23)
L_MIN = -6

Cir = collections.namedtuple("Cir", "name ra ta p t l w kind")


def _c(name, ra=1, ta=1, p=3, t=65, l=10, w=W_TIGHT, kind="tight"):
    return Cir(name, ra, ta, p, t, l, w, kind)


CIR = (
    [_c(f"L{l}", l=l, ra=2) for l in (1, 8, 9, 10, 18, 19, 27, 31)]
    + [_c(f"T{t}", t=t, ta=2) for t in (1, 63, 64, 65, 255, 256, 257, 513)]
    + [_c("P1xL9", p=1, l=9), _c("P2xL9", p=2, l=9), _c("P23xL9", p=23, l=9, ra=2), _c("P23xL10", p=23, l=10)]
    + [_c(f"ant{ra}x{ta}", ra=ra, ta=ta, l=19, t=70) for ra, ta in ((1, 1), (2, 1), (1, 2), (2, 2))]
    + [_c("tdl", ra=2, ta=2, p=23, t=65, l=31, w=W_TDL, kind="tdl"),
       _c("tau0", ra=2, ta=2, l=10, kind="tau0"),
       _c("tauint", ra=2, ta=2, p=5, l=19, w=W_INT, kind="tauint"),
       _c("zero", ra=2, ta=2, l=19, t=70, kind="zero")]
    + [_c(f"lds{p}", p=p, t=3, l=31) for p in (8, 9, 16, 801)]
)
CIR_BY_NAME = {c.name: c for c in CIR}
CIR_REFUSED = _c("lds802", p=802, t=3, l=31)                 # 4 (802 * 31) + 2048 * 31 + 1024 bytes: 120 past 160 KiB
ZERO_LINK = (1, 0, 1)                                        # (b, rx, tx) of the "zero" case

Apply = collections.namedtuple("Apply", "name rx ra tx ta tn l")
APPLY = [Apply(f"{tn}x{l}", 2, 2, 2, 2, tn, l) for tn, l in ((1, 1), (1, 8), (3, 32), (7, 8), (248, 8), (249, 8), (250, 8), (506, 8))]
APPLY += [Apply("1tx_7x8", 2, 2, 1, 1, 7, 8), Apply("1rx_250x8", 1, 1, 2, 2, 250, 8)]
APPLY_BY_NAME = {c.name: c for c in APPLY}
APPLY_REFUSED = Apply("3x33", 1, 1, 1, 1, 3, 33)             # 256 * 33 * 8 bytes: past the 64 KiB tap stage


def _cplx(rng, shape):
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)


def make_cir(case, batch=BATCH):
    """-> bandwidth (float), a complex64 [batch, 2, RA, 2, TA, P, T], tau float32 [batch, 2, 2, P], l_min, l_max"""
    rng = np.random.default_rng([7, case.ra, case.ta, case.p, case.t, case.l, len(case.name)])
    shp = (batch, NUM_RX, case.ra, NUM_TX, case.ta, case.p, case.t)
    prof = 10.0 ** (-2.0 * np.arange(case.p) / max(case.p - 1, 1))               # amplitude: 40 dB of power over the paths
    a = _cplx(rng, shp) * prof[:, None]
    tshape = (batch, NUM_RX, NUM_TX, case.p)
    if case.kind == "tdl":
        hi = np.where(np.arange(case.p) % 2 == 0, 0.8e-6, 3e-6)                  # half the paths inside the lag window
        tau = rng.uniform(0, 1, size=tshape) * hi
    elif case.kind == "tau0":
        tau = np.zeros(tshape)
    elif case.kind == "tauint":                                                 # k 2^-23 s at W = 2^23 Hz: tau W = k exactly
        tau = rng.permutation(np.arange(batch * NUM_RX * NUM_TX * case.p) % 13).reshape(tshape) / case.w
    else:
        tau = rng.uniform(0, 8.0 / case.w, size=tshape)
    if case.kind == "zero":
        b, rx, tx = ZERO_LINK
        a[b, rx, :, tx] = 0
    return case.w, a.astype(np.complex64), tau.astype(np.float32), L_MIN, L_MIN + case.l - 1


def make_apply(case, batch=BATCH):
    """-> x complex64 [batch, TX, TA, Tn], h complex64 [batch, RX, RA, TX, TA, Tn + L - 1, L], link_scale float32 [batch, RX, TX]
    with one link's scale 0 (the last (b, rx, tx))"""
    rng = np.random.default_rng([11, case.rx, case.ra, case.tx, case.ta, case.tn, case.l])
    x = _cplx(rng, (batch, case.tx, case.ta, case.tn))
    h = _cplx(rng, (batch, case.rx, case.ra, case.tx, case.ta, case.tn + case.l - 1, case.l))
    h = h * 10.0 ** (-2.0 * np.arange(case.l) / max(case.l - 1, 1))              # 40 dB over the taps
    s = rng.uniform(0.5, 2.0, size=(batch, case.rx, case.tx))
    s[-1, -1, -1] = 0.0
    return x.astype(np.complex64), h.astype(np.complex64), s.astype(np.float32)
