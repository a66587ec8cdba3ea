"""Optical channels without a GPU: the NumPy specification tests/optical_f32.py against the reference's own results
(tests/golden/optical_ref_golden.npz, optical_ref_vectors.npz: the reference's fiber.py / edfa.py executed by
tools/gen_optical_ref_golden.py), the windows and time / frequency vectors, the signatures and the refusals.

Bars.  float32 specification against the reference's double result: 4 e32 + 2^-23 max|y|, e32 = max |single - double| over
the reference's own two results of the case (the margin of rows a19g / a19h of COVERAGE.md).  float64 specification: 2^-29
times that.  Shipped known answers (test_optical.py:25-92): the reference's criterion there is
mean((|u| - u_ref)^2) <= 1e-7 - the vectors carry five digits, so the reference's own double result is 4.2e-4 (fixed) and
4.6e-4 (adaptive) away from them at the worst sample while its mean square is 2.6e-8; the specification is held to that
criterion against the shipped vectors AND to a maximum absolute deviation of 1e-7 against the reference's own double
result for the same configuration."""
import json
import os

import numpy as np
import pytest
import torch

import optical_cases as oc
import optical_f32 as spec
from sionna_amd.phy.channel import EDFA, SSFM, time_frequency_vector

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "optical_ref_golden.npz"))
META = json.loads(str(G["meta"]))
V = np.load(os.path.join(GOLD, "optical_ref_vectors.npz"))
STORED = [n for n in oc.CASES if META[n]["stored"]]


def bar32(name):
    return 4.0 * META[name]["e32"] + 2.0 ** -23 * META[name]["ymax"]


_SPEC = {}


def spec_result(name, precision, fault=None):
    key = (name, precision, fault)
    if key not in _SPEC:
        _SPEC[key] = spec.ssfm(oc.make_input(name), precision=precision, fault=fault, **oc.parameters(name))
    return _SPEC[key]


def test_fixture_covers_the_cases():
    assert set(oc.CASES) | {"span"} == set(META)
    for name in oc.CASES:
        x = oc.make_input(name)
        assert np.array_equal(G[name + "/x"] if META[name]["stored"] else G[name + "/x_head"], x if META[name]["stored"] else x[:2])
    n_ssfm = {oc.parameters(n)["n_ssfm"] for n in oc.CASES}
    assert {1, 2, 50, "adaptive"} <= n_ssfm
    assert {0, 1, 32} <= {oc.parameters(n)["half_window_length"] for n in oc.CASES if oc.CASES[n][0][-1] == 64}


@pytest.mark.parametrize("name", STORED)
def test_float32_specification_within_the_reference_bar(name):
    y, _ = spec_result(name, "single")
    err = float(np.max(np.abs(y.astype(np.complex128) - G[name + "/y64"]))) if y.size else 0.0
    print(f"{name}: |spec32 - ref64| {err:.3e}, bar {bar32(name):.3e}")
    assert y.dtype == np.complex64 and err <= bar32(name)


@pytest.mark.parametrize("name", STORED)
def test_float64_specification_reproduces_the_reference(name):
    y, _ = spec_result(name, "double")
    err = float(np.max(np.abs(y - G[name + "/y64"])))
    print(f"{name}: |spec64 - ref64| {err:.3e}, bar {bar32(name) * 2.0 ** -29:.3e}")
    assert err <= bar32(name) * 2.0 ** -29


@pytest.mark.parametrize("name", ["grid_trip", "grid_trip_nodisp"])
def test_large_case_heads(name):
    """the large cases keep their first rows only: rows are independent in the fixed scheme"""
    x = oc.make_input(name)[:2]
    y, _ = spec.ssfm(x, precision="double", **oc.parameters(name))
    assert float(np.max(np.abs(y - G[name + "/y64_head"]))) <= bar32(name) * 2.0 ** -29


@pytest.mark.parametrize("scheme", ["fixed", "adaptive"])
def test_shipped_known_answers(scheme):
    par = dict(alpha=0.0, beta_2=1.0, gamma=1.0, half_window_length=0, length=5.0, sample_duration=float(V["sample_duration"]),
               with_amplification=False, with_attenuation=False, n_sp=1.0)
    par.update(dict(n_ssfm=2000) if scheme == "fixed" else dict(n_ssfm="adaptive", phase_inc=1e-3))
    y, _ = spec.ssfm(V["u0"], precision="double", **par)
    mse = float(np.mean((np.abs(y) - V["u_ref"]) ** 2))
    dev = float(np.max(np.abs(np.abs(y) - np.abs(V["y_" + scheme]))))
    print(f"{scheme}: mean (|u| - u_ref)^2 {mse:.3e}; max | |u| - |u_reference_double| | {dev:.3e}")
    assert mse <= 1e-7
    assert dev <= 1e-7
    # dual polarisation (test_optical.py:273-388): half the power in each polarisation, Manakov's 8/9 compensated
    u2 = np.sqrt(9 / 8 * 0.5) * np.tile(V["u0"], (1, 2, 1))
    y2, _ = spec.ssfm(u2, precision="double", with_manakov=True, **par)
    u = np.linalg.norm(y2 * np.sqrt(8 / 9), axis=-2)
    assert float(np.mean((u - V["u_ref"]) ** 2)) <= 1e-7


def test_windows_are_exact():
    for n, h in ((64, 0), (64, 1), (64, 8), (64, 32), (15, 3)):
        w = spec.window(n, h, "double")
        assert np.array_equal(w[h:n - h], np.ones(n - 2 * h))
        k = np.arange(2 * h)
        assert np.array_equal(np.concatenate([w[:h], w[n - h:]]), 0.54 - 0.46 * np.cos(2.0 * np.pi * k / max(2 * h, 1)))
        # the reference's window in double precision: the same values, bit for bit
        assert np.array_equal(w, G[f"window/{n}/{h}/double"])
        # in single precision equality cannot hold: the reference (tf.signal.hamming_window, here its NumPy stand-in of
        # tools/ref_exec/tf_numpy.py) takes the cosine of a float32 argument and the products in float32, while the kernels'
        # table is the double value rounded once - the two differ by at most one ulp at 1 (2^-23), and the table is the
        # nearer one: it is within half a float32 ulp of the double window
        single = spec.window(n, h, "single")
        assert np.max(np.abs(single - G[f"window/{n}/{h}/single"])) <= 2.0 ** -23
        assert np.array_equal(single, w.astype(np.float32))
        assert np.all(np.abs(single.astype(np.float64) - w) <= np.abs(G[f"window/{n}/{h}/single"].astype(np.float64) - w))


@pytest.mark.parametrize("prec", ["single", "double"])
def test_time_frequency_vector_is_exact(prec):
    for n in (64, 15):
        for fn in (time_frequency_vector, spec.time_frequency_vector):
            t, f = fn(n, 0.5, precision=prec)
            assert t.dtype == G[f"tf/{n}/{prec}/t"].dtype
            assert np.array_equal(t, G[f"tf/{n}/{prec}/t"]) and np.array_equal(f, G[f"tf/{n}/{prec}/f"])
    t, f = time_frequency_vector(4, 2.0)
    assert t.dtype == np.float32 and np.array_equal(t, [-4, -2, 0, 2]) and np.array_equal(f, [-0.25, -0.125, 0, 0.125])


# ------------------------------------------------------------------ seeded faults land outside the bar
@pytest.mark.parametrize("name,fault", [("adaptive40", "adaptive_order"), ("manakov", "no_8_9"), ("fixed2", "no_1_n"),
                                        ("window8", "taper_in_middle")])
def test_seeded_fault_lands_outside_the_bar(name, fault):
    y, _ = spec_result(name, "double", fault)
    err = float(np.max(np.abs(y - G[name + "/y64"])))
    print(f"{name} with {fault}: {err:.3e} against the bar {bar32(name):.3e}")
    assert err > bar32(name)


# ------------------------------------------------------------------ interface
def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "optical_api_signatures.json")) as f:
        sig = json.load(f)["signatures"]
    assert set(sig) == {"channel.SSFM", "channel.EDFA", "channel.time_frequency_vector"}
    for cls in (SSFM, EDFA):
        _check(sig["channel." + cls.__name__]["__init__"], cls.__init__, cls.__name__ + ".__init__")
        _check(sig["channel." + cls.__name__]["call"], cls.call, cls.__name__ + ".call")
    _check(sig["channel.time_frequency_vector"]["params"], time_frequency_vector, "time_frequency_vector")


def test_names_resolve_under_install_as_sionna():
    import sionna_amd
    sionna_amd.install_as_sionna()
    import sionna.phy.channel as c
    from sionna.phy.channel.optical import SSFM as S2, EDFA as E2
    from sionna.phy import constants
    assert c.SSFM is S2 is SSFM and c.EDFA is E2 is EDFA and c.time_frequency_vector is time_frequency_vector
    assert constants.H == 6.62607015e-34


def test_noise_powers():
    s = SSFM(alpha=0.046, f_c=193.55e12, length=80, n_sp=1.2, sample_duration=2.0, t_norm=1e-12, with_manakov=True)
    assert np.isclose(s._p_n_ase, 6.62607015e-34 * 193.55e12 * 0.046 * 80 * 1.2 / 2.0 / 1e-12 / 2.0, rtol=1e-14)
    e = EDFA(g=4.0, f=7.0, f_c=193.55e12, dt=1e-12, precision="double")
    assert np.isclose(e._p_n_ase, 2 * (3.5 * 4 / 3) * 3 * 6.62607015e-34 * 193.55e12 / 1e-12, rtol=1e-14)
    assert EDFA(g=1.0)._p_n_ase == 0.0 and EDFA(g=1.0)._sqrt_g == 1.0
    assert EDFA(with_dual_polarization=True, precision="double")._p_n_ase == EDFA(precision="double")._p_n_ase / 2


# ------------------------------------------------------------------ refusals, one test each
def test_refuses_n_ssfm_of_another_type():
    with pytest.raises(ValueError, match="Unsupported parameter for n_ssfm"):
        SSFM(n_ssfm=2.5)
    with pytest.raises(ValueError, match="Unsupported parameter for n_ssfm"):
        SSFM(n_ssfm="auto")


def test_refuses_non_positive_n_ssfm():
    with pytest.raises(ValueError):
        SSFM(n_ssfm=0)


def test_refuses_wrong_precision():
    with pytest.raises(ValueError):
        SSFM(precision="half")
    with pytest.raises(ValueError):
        EDFA(precision="half")


def test_refuses_non_bool_dual_polarization():
    with pytest.raises(AssertionError, match="with_dual_polarization must be bool."):
        EDFA(with_dual_polarization=1)


def test_refuses_wrong_rank_for_manakov():
    with pytest.raises(ValueError):
        SSFM(with_manakov=True).call(torch.zeros(3, 64, dtype=torch.complex64))
    with pytest.raises(ValueError):
        SSFM(with_manakov=True).call(torch.zeros(64, dtype=torch.complex64))


def test_refuses_rank_zero_input():
    with pytest.raises(ValueError):
        SSFM().call(torch.zeros((), dtype=torch.complex64))


def test_refuses_window_longer_than_the_signal():
    with pytest.raises(ValueError, match="half_window_length"):
        SSFM(half_window_length=33).call(torch.zeros(3, 64, dtype=torch.complex64))
    SSFM(half_window_length=32)                                   # n / 2 itself is allowed (fixture case window_half)


# the C-ABI's own refusals come before any device work: exercised here with host addresses that are never read
def _abi_ssfm(rows=1, n=64, n_ssfm=1, h=0, ws_bytes=None, x=True, length=80.0, sample_duration=1.0, p_n_ase=0.0, dbl=False):
    import ctypes as C
    from sionna_amd import _ffi
    lib = _ffi.lib()
    buf = C.create_string_buffer(64)
    addr = C.c_void_p(C.addressof(buf))
    need = lib.samd_ssfm_workspace_bytes(n, int(dbl))
    steps = C.c_int64(-1)
    fn = lib.samd_ssfm_c128 if dbl else lib.samd_ssfm_c64
    rc = fn(addr if x else None, rows, n, 0, 0.046, -21.67, 1.27, length, sample_duration, n_ssfm, 1e-4, h, p_n_ase, 0, 1, 1, 1, 0, 0,
            C.byref(steps), addr, need if ws_bytes is None else ws_bytes, addr, None)
    return rc, lib.samd_last_error().decode(), steps.value


def test_abi_refuses_bad_n_ssfm():
    from sionna_amd import _ffi
    for bad in (0, -2):
        rc, msg, _ = _abi_ssfm(n_ssfm=bad)
        assert rc == _ffi.ERR_INVALID and "n_ssfm" in msg


def test_abi_refuses_small_workspace():
    from sionna_amd import _ffi
    for dbl in (False, True):
        need = _ffi.lib().samd_ssfm_workspace_bytes(64, int(dbl))
        assert need >= 3 * 64 * (16 if dbl else 8) + 64 * (8 if dbl else 4)
        rc, msg, _ = _abi_ssfm(ws_bytes=need - 1, dbl=dbl)
        assert rc == _ffi.ERR_WORKSPACE and "workspace" in msg
    assert _ffi.lib().samd_ssfm_workspace_bytes(0, 0) == 0


def test_abi_refuses_bad_shapes_and_parameters():
    from sionna_amd import _ffi
    for kw, word in ((dict(n=0), "shape"), (dict(rows=-1), "shape"), (dict(h=33), "half_window_length"), (dict(h=-1), "half_window_length"),
                     (dict(x=False), "null"), (dict(sample_duration=0.0), "parameter"), (dict(length=-1.0), "parameter"),
                     (dict(p_n_ase=-1.0), "parameter"), (dict(rows=1 << 31), "rows")):
        rc, msg, _ = _abi_ssfm(**kw)
        assert rc == _ffi.ERR_INVALID and word in msg, (kw, rc, msg)


def test_abi_empty_batch_takes_no_step():
    from sionna_amd import _ffi
    rc, _, steps = _abi_ssfm(rows=0)
    assert rc == _ffi.OK and steps == 0


def test_abi_edfa_refusals():
    import ctypes as C
    from sionna_amd import _ffi
    lib = _ffi.lib()
    buf = C.create_string_buffer(64)
    addr = C.c_void_p(C.addressof(buf))
    assert lib.samd_edfa_c64(None, 8, 2.0, 0.0, 0, 0, addr, None) == _ffi.ERR_INVALID
    assert lib.samd_edfa_c64(addr, -1, 2.0, 0.0, 0, 0, addr, None) == _ffi.ERR_INVALID
    assert lib.samd_edfa_c128(addr, 8, 2.0, -1.0, 0, 0, addr, None) == _ffi.ERR_INVALID
    assert lib.samd_edfa_c64(addr, 0, 2.0, 0.0, 0, 0, addr, None) == _ffi.OK


def test_refuses_wrong_rank_for_dual_polarization():
    with pytest.raises(ValueError):
        EDFA(with_dual_polarization=True).call(torch.zeros(3, 64, dtype=torch.complex64))


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError):
        SSFM()(np.zeros((1, 8), np.complex64))
    with pytest.raises(RuntimeError):
        EDFA()(np.zeros((1, 8), np.complex64))


def test_swap_memory_and_unknown_kwargs_are_accepted():
    s = SSFM(swap_memory=False, some_keras_kwarg=1)
    assert s._n_ssfm == 1 and SSFM(n_ssfm="adaptive")._n_ssfm == -1
