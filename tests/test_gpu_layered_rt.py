"""GPU: the running-total layered engine (csrc/ldpc5g_onchip_lyrt.hip, ``LDPC5GDecoder.layered_totals = "running"``) is
bit-identical to its float32 specification tests/ldpc_layered_rt_f32.py - soft and hard output, information bits and
codeword, 1 / 3 / 10 iterations, min-sum and offset-min-sum - on lifting sizes below 64, not a multiple of 64 and C2's own
code; batch edges around the codewords one workgroup holds and past one grid trip; the engine attribute shows which kernel
ran, the codes and rules it does not cover run as before, and going back to "resum" gives today's bits back."""
import functools
import itertools

import numpy as np
import pytest

from oracle.ldpc5g import LDPC5GCode
from oracle import ldpc_bp as obp
from ldpc_layered_rt_f32 import LayeredRunningTotal

pytestmark = pytest.mark.gpu

CODES = [(64, 128, None, None),          # Z = 11: one partly filled chunk
         (200, 600, "bg2", 2),           # Z = 26
         (500, 1000, None, 4),           # Z = 64
         (1024, 2048, "bg1", None),      # Z = 48
         (2816, 8448, "bg1", 6)]         # C2: Z = 128, two chunks per row
BATCH = 6


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as phy
    return phy


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(k, n, bg, m):
    """the inputs of test_layered_on_chip_bit_exact (noisy LLRs, a run of exact zeros, one row rounded to integers: ties)
    and one row scaled past llr_max"""
    code = LDPC5GCode(k, n, m, bg)
    rng = np.random.default_rng(k + 3 * n)
    u = rng.integers(0, 2, (BATCH, k)).astype(np.float32)
    c = code.encode(u)
    sigma = 0.7
    y = (2 * c - 1) + sigma * rng.normal(size=c.shape)
    llr = (2 * y / sigma ** 2).astype(np.float32)
    llr[0, :9] = 0
    llr[1] = np.round(llr[1])
    llr[2] *= 7.0                                               # most of the row beyond llr_max = 20
    return code, llr


@functools.lru_cache(maxsize=None)
def _spec(k, n, bg, m, cn, it, infobits, hard):
    code, llr = _inputs(k, n, bg, m)
    ref = LayeredRunningTotal(code, cn_update=cn, num_iter=it, hard_out=hard, return_infobits=infobits).decode5g(llr)
    ref.setflags(write=False)
    return ref


def _decoder(phy, k, n, bg, m, **kw):
    enc = phy.fec.ldpc.LDPC5GEncoder(k, n, num_bits_per_symbol=m, bg=bg)
    dec = phy.fec.ldpc.LDPC5GDecoder(enc, cn_schedule="layered", **kw)
    dec.layered_totals = "running"
    return enc, dec


@pytest.mark.parametrize("cn", ["minsum", "offset-minsum"])
@pytest.mark.parametrize("k,n,bg,m", CODES)
def test_kernel_equals_the_specification(phy, k, n, bg, m, cn):
    code, llr = _inputs(k, n, bg, m)
    for it, infobits, hard in itertools.product((1, 3, 10), (True, False), (False, True)):
        enc, dec = _decoder(phy, k, n, bg, m, cn_update=cn, num_iter=it, hard_out=hard, return_infobits=infobits)
        got = _np(dec(llr))
        assert dec.layered_engine == "running", (k, n, dec.layered_engine)
        ref = _spec(k, n, bg, m, cn, it, infobits, hard)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (f"{cn} it={it} infobits={infobits} hard={hard}: {np.mean(got != ref):.3e} differ, "
                                          f"max {np.max(np.abs(got - ref))}")


def _slots(dec, enc):
    from sionna_amd import _ffi
    return int(_ffi.lib().samd_ldpc5g_decode_layered_rt_slots(enc._handle(dec._nb_pruned_nodes)))


@pytest.mark.parametrize("k,n,bg,m", [(64, 128, None, None), (200, 600, "bg2", 2), (1024, 2048, "bg1", None)])
def test_batch_edges_around_one_workgroup(phy, k, n, bg, m):
    """0, 1, one less and one more than the codewords a workgroup holds: a masked tail still reaches every barrier"""
    code, llr = _inputs(k, n, bg, m)
    enc, dec = _decoder(phy, k, n, bg, m, cn_update="minsum", num_iter=3, hard_out=False)
    ref = _spec(k, n, bg, m, "minsum", 3, True, False)
    s = _slots(dec, enc)
    assert s >= 1
    assert tuple(dec(llr[:0]).shape) == (0, k)
    for b in sorted({1, max(1, s - 1), s, s + 1, 2 * s + 1}):
        big = np.tile(llr, (b // BATCH + 1, 1))[:b]
        want = np.tile(ref, (b // BATCH + 1, 1))[:b]
        got = _np(dec(big))
        assert dec.layered_engine == "running"
        assert np.array_equal(got, want), (b, s)


@pytest.mark.parametrize("k,n,bg,m", [(200, 600, "bg2", 2), (2816, 8448, "bg1", 6)])
def test_batch_past_one_grid_trip(phy, k, n, bg, m):
    """a grid of 5 workgroups takes several trips over 11 x 6 codewords: same bits as the unrestricted grid, and tiled
    copies of a codeword decode alike"""
    from sionna_amd import _ffi
    code, llr = _inputs(k, n, bg, m)
    big = np.tile(llr, (11, 1))
    enc, dec = _decoder(phy, k, n, bg, m, cn_update="offset-minsum", num_iter=3, hard_out=False)
    full = _np(dec(big))
    assert dec.layered_engine == "running"
    with _ffi.option("SAMD_ONCHIP_GRID", 5):
        part = _np(dec(big))
        assert dec.layered_engine == "running"
    assert np.array_equal(part, full)
    assert np.array_equal(full[:BATCH], full[BATCH:2 * BATCH]) and np.array_equal(full[:BATCH], full[-BATCH:])
    assert np.array_equal(full[:BATCH], _spec(k, n, bg, m, "offset-minsum", 3, True, False))


def test_uncovered_code_and_rule_run_as_before(phy):
    """boxplus-phi with "running": today's layered engine, today's bits.  A handle with a partially pruned base row (the
    layered decoder rounds its pruning to whole rows, so such a handle comes from a flooding decoder): the entry declines.
    A flooding decoder ignores the property."""
    k, n, bg, m = 1024, 2048, "bg1", None
    code, llr = _inputs(k, n, bg, m)
    kw = dict(cn_update="boxplus-phi", num_iter=3, hard_out=False)
    enc, dec = _decoder(phy, k, n, bg, m, **kw)
    got = _np(dec(llr))
    assert dec.layered_engine == "resum"
    dec2 = phy.fec.ldpc.LDPC5GDecoder(enc, cn_schedule="layered", **kw)
    assert np.array_equal(got, _np(dec2(llr)))
    # a code the running-total engine does not take: handle with a partially pruned base row
    from sionna_amd import _ffi
    lib = _ffi.lib()
    enc3 = phy.fec.ldpc.LDPC5GEncoder(500, 1000, num_bits_per_symbol=4)
    dec3 = phy.fec.ldpc.LDPC5GDecoder(enc3, cn_update="minsum", num_iter=3, hard_out=False)       # flooding: pruning not rounded to Z
    h = enc3._handle(dec3._nb_pruned_nodes)
    assert dec3._nb_pruned_nodes % enc3.z != 0
    assert lib.samd_ldpc5g_decode_layered_rt_supported(h, 2) == 0
    assert lib.samd_ldpc5g_decode_layered_rt_slots(h) == 0
    _, llr3 = _inputs(500, 1000, None, 4)
    import torch
    o = torch.empty((BATCH, 500), dtype=torch.float32, device=_ffi.device())
    rc = lib.samd_ldpc5g_decode_layered_rt_f32(h, _ffi.ptr(_ffi.to_device(llr3, torch.float32)), _ffi.ptr(o), BATCH, 3, 2, 20.0, 0.5,
                                               0, 1, None, 0, _ffi.stream())
    assert rc == _ffi.ERR_UNSUPPORTED
    dec3.layered_totals = "running"                               # flooding: the property changes nothing
    ref3 = phy.fec.ldpc.LDPC5GDecoder(enc3, cn_update="minsum", num_iter=3, hard_out=False)
    _, llr3 = _inputs(500, 1000, None, 4)
    assert np.array_equal(_np(dec3(llr3)), _np(ref3(llr3)))
    assert dec3.layered_engine is None


def test_resum_after_running_gives_todays_bits(phy):
    k, n, bg, m = 200, 600, "bg2", 2
    code, llr = _inputs(k, n, bg, m)
    kw = dict(cn_update="minsum", num_iter=10, hard_out=False)
    enc, dec = _decoder(phy, k, n, bg, m, **kw)
    run = _np(dec(llr))
    assert dec.layered_engine == "running"
    dec.layered_totals = "resum"
    back = _np(dec(llr))
    assert dec.layered_engine == "resum"
    ref = obp.LDPC5GDecoder(code, cn_schedule="layered", **kw).decode5g(llr)
    assert np.array_equal(back, ref)
    assert run.shape == ref.shape
    assert dec.layered_totals == "resum"
    with pytest.raises(ValueError):
        dec.layered_totals = "total"
