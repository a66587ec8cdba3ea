"""The tap generators ``TDL`` (csrc/ofdm.hip ``tdl_cir_kernel``, csrc/f64_ofdm.hip ``tdl_cir128_kernel``) and ``CDL`` (csrc/cdl.hip
``cdl_cir_kernel`` in float32 and float64) through the public classes against the float64 anchors of tests/tdl_f32.py and
tests/cdl_f32.py, on EVERY output, within the bounds derived there from the kernels' arithmetic (u = 2^-24; 2^-53 with
``precision="double"``).  The cases (tests/tap_channel_cases.py, which says which case reaches which branch) are the smallest
that reach every path: full and short chunks of 16 time steps, re-anchoring, register and per-chunk draws (N <= 24, N > 24), LoS with
other angles of arrival, blocks that are not full, 32-antenna panels, both directions, orientations, arguments of hundreds of rad.
The CPU side (tests/test_tap_channel_host.py) shows on these very inputs that the bounds are neither too tight nor too loose.

Every test prints its max |a - anchor| / bound (run with -s); on failure the message carries the worst ratio and its index
(b, u, s, n, t).  On top of the cases: ``delay_spread`` changed between two calls, ``batch_size = 0``, and a TDL with receive and
transmit correlation (the path from the N > 24 branch into ``samd_spatial_corr_c64``).

On an MI355X with ROCm's device library the largest ratios are those of the NumPy models to two digits: TDL float32 0.02 ... 0.044
at N >= 20, 0.09 at N = 1 and 2, 0.14 on D_T200_n2_slow; TDL float64 0.003 ... 0.021; CDL float32 0.01 ... 0.043; CDL float64 0.003 ...
0.004 (there the bar is the anchor's own float64 accuracy, as in tests/test_gpu_time_channel_edges.py).  The TDL outputs are also held
per component (``bound_re``, ``bound_im``, item 10 of tests/tdl_f32.py; not behind the correlation matrix, which mixes the
components): float32 0.03 ... 0.08, 0.12 ... 0.15 at N = 1 and 2, 0.23 on D_T200_n2_slow; float64 at most 0.026.  Nothing is above 1."""
import numpy as np
import pytest

import cdl_f32 as cf
import tap_channel_cases as tc
import tdl_f32 as tf
from oracle import cdl as oc

pytestmark = pytest.mark.gpu

SEED = 11
PREC = {"single": (tf.U32, np.complex64, np.float32), "double": (tf.U64, np.complex128, np.float64)}


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _hold(ratio, a, an, bd, cdtype, what):
    a = np.asarray(a)
    assert a.shape == an.shape and a.dtype == cdtype, (what, a.shape, an.shape, a.dtype)
    assert np.all(np.isfinite(a.view(a.real.dtype))), what
    q, at = ratio(a, an, bd)
    print(f"tap {what}: max |a - anchor| / bound = {q:.4f}")
    b, _, u, _, s, n, t = at if at else (0,) * 7
    assert q <= 1, f"{what}: worst |a - anchor| / bound = {q:.3f} at (b, u, s, n, t) = {(b, u, s, n, t)}"
    return q


def _seed(phy, call):
    """the stream at ``call``: a fresh seed puts it at 0"""
    phy.config.seed = SEED
    for _ in range(call):
        phy.config.rng.next_call()


# ------------------------------------------------------------------ TDL
def _tdl_check(phy, tdl, case, call=None, batch=None, corr=None):
    u, cdt, rdt = PREC[case.prec]
    b = case.b if batch is None else batch
    a, tau = tdl(b, case.t, case.fs)
    assert tuple(a.shape) == (b, 1, case.ra, 1, case.ta, tdl.num_clusters, case.t) and tuple(tau.shape) == (b, 1, 1, tdl.num_clusters)
    assert _np(tau).dtype == rdt
    assert np.array_equal(_np(tau), np.broadcast_to(tdl.delays.astype(rdt), tau.shape))
    args, kw = tc.tdl_args(tdl, case, SEED, call=call, batch=batch)
    an, bd, b_re, b_im = tf.anchor_and_bounds(*args, **kw, u=u)
    what = f"tdl {case.name} {case.prec}"
    if corr is not None:                                    # the matrix mixes the components: held in modulus
        an, bd = tf.correlate(an, bd, corr, u)
        return _hold(tf.ratio, _np(a), an, bd, cdt, what)
    _hold(lambda o, r, _: tf.ratio_parts(o, r, b_re, b_im), _np(a), an, bd, cdt, what + " per component")
    return _hold(tf.ratio, _np(a), an, bd, cdt, what)


@pytest.mark.parametrize("case", tc.TDL + tc.TDL64, ids=[c.name for c in tc.TDL + tc.TDL64])
def test_tdl_holds_the_bound(phy, case):
    _seed(phy, case.call)
    _tdl_check(phy, tc.tdl_object(phy.channel.tr38901, case), case)


def test_tdl_second_call_continues_on_the_stream(phy):
    """two calls on one object: call indices 0 and 4"""
    case = tc.TDL_BY_NAME["second_D"]
    tdl = tc.tdl_object(phy.channel.tr38901, case)
    _seed(phy, 0)
    _tdl_check(phy, tdl, case, call=0)
    _tdl_check(phy, tdl, case, call=4)


def test_tdl_delay_spread_changed_between_calls(phy):
    """the device copy of tau is kept per batch size: a new delay spread must not return the former delays"""
    case = tc.TDL_BY_NAME["D_T17"]
    tdl = tc.tdl_object(phy.channel.tr38901, case)
    _seed(phy, 0)
    _, tau1 = tdl(case.b, case.t, case.fs)
    first = tdl.delays.copy()
    tdl.delay_spread = 2 * tc.DELAY_SPREAD
    _, tau2 = tdl(case.b, case.t, case.fs)
    assert np.array_equal(_np(tau1)[0, 0, 0], first.astype(np.float32))
    assert np.array_equal(_np(tau2), np.broadcast_to(tdl.delays.astype(np.float32), tau2.shape))
    assert np.array_equal(_np(tau2)[0, 0, 0], (tdl._delays * np.float32(2 * tc.DELAY_SPREAD)).astype(np.float32))
    assert not np.array_equal(_np(tau1), _np(tau2))


@pytest.mark.parametrize("prec", list(PREC))
def test_tdl_batch_zero(phy, prec):
    """empty tensors of the right shape, no launch; the stream advances by 4 as for any call: the next call is call index 4"""
    case = tc.TDL_BY_NAME["D_T17"]._replace(prec=prec)
    tdl = tc.tdl_object(phy.channel.tr38901, case)
    _seed(phy, 0)
    a, tau = tdl(0, case.t, case.fs)
    assert tuple(a.shape) == (0, 1, case.ra, 1, case.ta, tdl.num_clusters, case.t) and tuple(tau.shape) == (0, 1, 1, tdl.num_clusters)
    assert _np(a).dtype == PREC[prec][1] and _np(tau).dtype == PREC[prec][2]
    assert phy.config.rng.call == 4
    _tdl_check(phy, tdl, case, call=4)


def test_tdl_with_spatial_correlation(phy):
    """rx_corr_mat / tx_corr_mat at T = 17, N = 25: the anchor times the float64 correlation square root, the bound extended by the
    gamma of that matrix-vector product"""
    case = tc.TDL_BY_NAME["aoa2_n25"]
    r_rx, r_tx = tc.corr_matrices(case.ra, case.ta)
    tdl = tc.tdl_object(phy.channel.tr38901, case, rx_corr_mat=r_rx, tx_corr_mat=r_tx)
    w, v = np.linalg.eigh(r_rx)
    s_rx = (v * np.sqrt(w)) @ v.conj().T
    w, v = np.linalg.eigh(r_tx)
    s_tx = (v * np.sqrt(w)) @ v.conj().T
    mat = np.kron(s_rx, s_tx.conj())
    assert np.allclose(mat, tdl._corr_sqrt, rtol=0, atol=1e-13)
    _seed(phy, 0)
    _tdl_check(phy, tdl, case, corr=tdl._corr_sqrt)


# ------------------------------------------------------------------ CDL
def _cdl_pair(phy, case):
    t38 = phy.channel.tr38901
    cdl = t38.CDL(case.model, tc.DELAY_SPREAD, tc.FC_CDL, *tc.cdl_arrays(t38, case.kind), case.direction, precision=case.prec,
                  **tc.cdl_kwargs(case))
    ref = oc.CDL(case.model, tc.DELAY_SPREAD, tc.FC_CDL, *tc.cdl_arrays(oc, case.kind), case.direction, **tc.cdl_kwargs(case))
    return cdl, ref


def _cdl_check(phy, cdl, ref, case, call, batch=None):
    u, cdt, rdt = PREC[case.prec]
    b = case.b if batch is None else batch
    a, tau = cdl(b, case.t, case.fs)
    an, bd, _, _, tau_ref = cf.anchor_and_bound(ref, SEED, call, b, case.t, case.fs, u)
    assert tuple(tau.shape) == (b, 1, 1, ref.num_clusters) and _np(tau).dtype == rdt
    assert np.array_equal(_np(tau), np.broadcast_to(tau_ref.astype(rdt), tau.shape))
    return _hold(cf.ratio, _np(a), an, bd, cdt, f"cdl {case.name} {case.prec}")


@pytest.mark.parametrize("case", tc.CDL + tc.CDL64, ids=[c.name for c in tc.CDL + tc.CDL64])
def test_cdl_holds_the_bound(phy, case):
    cdl, ref = _cdl_pair(phy, case)
    _seed(phy, case.call)
    _cdl_check(phy, cdl, ref, case, case.call)


def test_cdl_second_call_continues_on_the_stream(phy):
    case = tc.CDL_BY_NAME["second_A"]
    cdl, ref = _cdl_pair(phy, case)
    _seed(phy, 0)
    _cdl_check(phy, cdl, ref, case, 0)
    _cdl_check(phy, cdl, ref, case, 8)


def test_cdl_delay_spread_changed_between_calls(phy):
    case = tc.CDL_BY_NAME["D_T17"]
    cdl, ref = _cdl_pair(phy, case)
    _seed(phy, 0)
    _, tau1 = cdl(case.b, case.t, case.fs)
    cdl.delay_spread = 2 * tc.DELAY_SPREAD
    _, tau2 = cdl(case.b, case.t, case.fs)
    srt = np.sort(ref.delays)
    assert np.array_equal(_np(tau1)[0, 0, 0], (srt * tc.DELAY_SPREAD).astype(np.float32))
    assert np.array_equal(_np(tau2)[0, 0, 0], (srt * (2 * tc.DELAY_SPREAD)).astype(np.float32))


@pytest.mark.parametrize("prec", list(PREC))
def test_cdl_batch_zero(phy, prec):
    """empty tensors of the right shape, no launch; the stream advances by 8: the next call is call index 8"""
    case = tc.CDL_BY_NAME["D_T15"]._replace(prec=prec)
    cdl, ref = _cdl_pair(phy, case)
    _seed(phy, 0)
    a, tau = cdl(0, case.t, case.fs)
    u_, s_ = cdl._rx_array.num_ant, cdl._tx_array.num_ant
    assert tuple(a.shape) == (0, 1, u_, 1, s_, ref.num_clusters, case.t) and tuple(tau.shape) == (0, 1, 1, ref.num_clusters)
    assert _np(a).dtype == PREC[prec][1] and _np(tau).dtype == PREC[prec][2]
    assert phy.config.rng.call == 8
    _cdl_check(phy, cdl, ref, case, 8)
