"""The cases of the optical fixtures, shared by tools/gen_optical_ref_golden.py (which runs the reference on them) and the
tests (which look their bars up by name): SSFM parameters, the input shape and the seed of the input."""
import numpy as np

BASE = dict(alpha=0.046, beta_2=-21.67, f_c=193.55e12, gamma=1.27, half_window_length=0, length=80, n_ssfm=1, n_sp=1.0,
            sample_duration=1.0, t_norm=1e-12, with_amplification=False, with_attenuation=True, with_dispersion=True,
            with_manakov=False, with_nonlinearity=True, phase_inc=1e-4)

GRID_TRIP_ROWS = 256 * 32 * 256 // 64 + 1          # [rows, 64]: one row past a full trip of the streaming kernels' grid

# name -> (shape, overrides of BASE)
CASES = {
    "fixed1": ((3, 64), dict(n_ssfm=1)),
    "fixed2": ((3, 64), dict(n_ssfm=2)),
    "fixed50": ((3, 64), dict(n_ssfm=50)),
    "adaptive1": ((3, 64), dict(n_ssfm="adaptive", phase_inc=10.0, length=8)),
    "adaptive40": ((3, 64), dict(n_ssfm="adaptive", phase_inc=0.034, length=8)),   # 40 steps; not at the edge of the loop's 1e-3 end
    "adaptive_nodisp": ((3, 64), dict(n_ssfm="adaptive", phase_inc=0.05, length=8, with_dispersion=False)),
    "adaptive_zero": ((3, 64), dict(n_ssfm="adaptive", phase_inc=0.05, length=8)),                 # all-zero input
    "adaptive_gamma0": ((3, 64), dict(n_ssfm="adaptive", phase_inc=0.05, length=8, gamma=0.0)),
    "window1": ((3, 64), dict(n_ssfm=4, half_window_length=1)),
    "window8": ((3, 64), dict(n_ssfm=4, half_window_length=8)),
    "window_half": ((3, 64), dict(n_ssfm=4, half_window_length=32)),
    "window_adaptive": ((3, 64), dict(n_ssfm="adaptive", phase_inc=0.05, length=8, half_window_length=8)),
    "alpha0": ((3, 64), dict(n_ssfm=4, alpha=0.0)),
    "amplified_nsp0": ((3, 64), dict(n_ssfm=4, with_amplification=True, n_sp=0.0)),
    "manakov": ((3, 2, 64), dict(n_ssfm=4, with_manakov=True)),
    "manakov_adaptive": ((3, 2, 64), dict(n_ssfm="adaptive", phase_inc=0.05, length=8, with_manakov=True)),
    "no_attenuation": ((3, 64), dict(n_ssfm=4, with_attenuation=False)),
    "no_dispersion": ((3, 64), dict(n_ssfm=4, with_dispersion=False)),
    "no_dispersion1": ((3, 64), dict(n_ssfm=1, with_dispersion=False)),
    "no_nonlinearity": ((3, 64), dict(n_ssfm=4, with_nonlinearity=False)),
    "no_nonlinearity_window": ((3, 64), dict(n_ssfm=4, with_nonlinearity=False, half_window_length=8)),
    "n1": ((3, 1), dict(n_ssfm=2)),
    "n2": ((3, 2), dict(n_ssfm=2)),
    "n15": ((3, 15), dict(n_ssfm=2)),
    "n16": ((1, 16), dict(n_ssfm=2)),
    "n1000": ((3, 1000), dict(n_ssfm=2, half_window_length=100)),
    "n4096": ((1, 4096), dict(n_ssfm=2)),
    "grid_trip": ((GRID_TRIP_ROWS, 64), dict(n_ssfm=2, length=8)),
    "grid_trip_nodisp": ((GRID_TRIP_ROWS, 64), dict(n_ssfm=2, length=8, with_dispersion=False)),
}

# the notebook's link (Optical_Lumped_Amplification_Channel.ipynb): spans of SSFM + EDFA on a Gaussian pulse, small n
SPAN = dict(n=256, n_span=3, sample_duration=1.0, t0=20.0, p0=0.03,
            ssfm=dict(alpha=0.046, beta_2=-21.67, f_c=193.55e12, gamma=1.27, half_window_length=16, length=20, n_ssfm=20,
                      sample_duration=1.0, t_norm=1e-12, with_amplification=False, with_attenuation=True, with_dispersion=True,
                      with_nonlinearity=True),
            edfa=dict(g=float(np.exp(0.046 * 20)), f=0.0, f_c=193.55e12, dt=1e-12))


def parameters(name):
    return dict(BASE, **CASES[name][1])


def make_input(name):
    """complex64 input of a case: a smooth pulse per row plus a little broadband content, peak power about 0.2 W"""
    shape = CASES[name][0]
    if name == "adaptive_zero":
        return np.zeros(shape, np.complex64)
    rng = np.random.default_rng(sum(map(ord, name)))
    n = shape[-1]
    t = (np.arange(n) - n // 2) / max(n / 8.0, 1.0)
    pulse = np.sqrt(0.2) * np.exp(-t * t / 2.0)
    lead = shape[:-1]
    amp = rng.uniform(0.5, 1.0, lead + (1,))
    phase = np.exp(1j * rng.uniform(0, 2 * np.pi, lead + (1,)))
    x = amp * phase * pulse + 0.02 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    return x.astype(np.complex64)


def span_input():
    n = SPAN["n"]
    t = (np.arange(n) - n // 2) * SPAN["sample_duration"]
    return (np.sqrt(SPAN["p0"]) * np.exp(-(t / SPAN["t0"]) ** 2 / 2.0)).astype(np.complex64)[None, :]
