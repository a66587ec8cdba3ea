"""Inputs of the cir_to_ofdm_channel edge tests (tests/test_gpu_channel_edges.py) and of the CPU restatements
(tests/test_kernel_models.py): the shape table with the kernel family each row was computed to reach
(``kernel_models.c2o_dispatch`` is asserted against it), and seeded inputs.

Layout: batch 3, two receivers, two transmitters - link addressing (b, rx, tx) is exercised at every shape.  ``tau`` is
distinct per (b, rx, tx, p) in 0 ... 2 us; the taps are complex normal times a power profile that decays by 20 dB over the
paths (the weakest path stays ~1e4 above the bound, so a dropped path is seen)."""
import numpy as np

BATCH, NUM_RX, NUM_TX = 3, 2, 2
SPACING = 15e3

# (RA, TA, P, T, F): family, then the properties of c2o_dispatch that must hold
TABLE = [
    ((4, 2, 23, 14, 76), "pass", dict(RPT=24, grouped=True, spare=4)),
    ((1, 1, 1, 1, 12), "pass", dict(RPT=8, G=32, grouped=True)),                 # every divisor 1, 255 padded rows
    ((2, 3, 8, 3, 12), "pass", dict(grouped=False, MAXP=8)),                    # P at a class edge
    ((2, 3, 9, 3, 12), "pass", dict(grouped=False, MAXP=16)),                   # one past it
    ((1, 3, 5, 14, 24), "pass", dict(grouped=False)),                           # T > G wrap
    ((3, 5, 17, 2, 48), "pass", dict(grouped=False, MAXP=24)),
    ((1, 7, 3, 2, 36), "pass", dict(grouped=False, G=7, spare=4)),
    ((2, 2, 32, 5, 100), "pass", dict(MAXP=32, spare=12)),
    ((1, 1, 4, 2, 300), "pass", dict(G=1, spare=20)),
    ((1, 1, 4, 2, 512), "pass", dict(G=1, nt=512, spare=0)),
    ((1, 2, 4, 7, 256), "pass", dict(G=1, RPT=16)),
    ((3, 2, 30, 15, 72), "pass", dict(RPT=16, G=7)),
    ((4, 2, 12, 12, 128), "pass", dict(RPT=32, grouped=True)),                  # RPT class 32 on the pass kernel
    ((5, 3, 6, 7, 128), "pass", dict(RPT=40, grouped=False)),                   # RPT class 40 on the pass kernel
    ((1, 1, 1, 1, 1), "reg", dict(G=256)),
    ((5, 4, 32, 9, 64), "reg", dict(RPT=40)),
    ((2, 2, 25, 41, 80), "reg", dict(spare=32)),
    ((2, 2, 33, 2, 24), "two_pass", dict(MAXP=64)),
    ((2, 1, 64, 2, 24), "two_pass", dict(MAXP=64)),
    ((2, 1, 65, 2, 24), "two_pass", dict(MAXP=0)),
    ((1, 1, 4, 2, 513), "two_pass", dict(G=1)),
    ((2, 2, 24, 14, 257), "two_pass", dict(G=1)),
]
SHAPES = [s for s, _, _ in TABLE]


def sid(shape):
    return "x".join(str(v) for v in shape)


def frequencies(num, spacing=SPACING):
    """``subcarrier_frequencies`` in float32; a single subcarrier sits three spacings off the carrier (at f = 0 every phase is
    zero and neither a wrong delay nor a wrong sign of sin could show)"""
    if num == 1:
        return np.array([3 * spacing], np.float32)
    return (np.arange(-(num // 2), num // 2 + num % 2, dtype=np.float32) * np.float32(spacing)).astype(np.float32)


def make(shape, seed=0, tau_max=2e-6, spacing=SPACING, num_tx=NUM_TX, batch=BATCH):
    """-> freqs float32 [F], a complex64 [batch, 2, RA, num_tx, TA, P, T], tau float32 [batch, 2, num_tx, P]"""
    ra, ta, p, t, f = shape
    rng = np.random.default_rng([seed, ra, ta, p, t, f])
    shp = (batch, NUM_RX, ra, num_tx, ta, p, t)
    prof = 10.0 ** (-np.arange(p) / max(p, 1))                                   # amplitude: 20 dB of power over the paths
    a = (rng.normal(size=shp) + 1j * rng.normal(size=shp)) / np.sqrt(2 * p) * prof[:, None]
    tau = rng.uniform(0, tau_max, size=(batch, NUM_RX, num_tx, p))
    return frequencies(f, spacing), a.astype(np.complex64), tau.astype(np.float32)
