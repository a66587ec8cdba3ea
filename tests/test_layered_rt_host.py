"""CPU: the running-total layered specification (tests/ldpc_layered_rt_f32.py, what csrc/ldpc5g_onchip_lyrt.hip is held to bit
for bit) computes the reference's layered decoder.

* same function: in float64 the specification and a literal model of the re-summing form (check-node update of a layer,
  then EVERY variable node re-summed - first shown array_equal to oracle.ldpc_bp in float32) agree to 1e-9 on every soft
  output of every word after 1 and 3 iterations; after 10 the words that do not converge drift further, and the bar is
  what the re-summing form's own drift under another summation order allows (asserted control, see the test);
* float32 closeness: each side's distance to that float64 anchor.  The bar for the specification is set against the
  oracle's own figures: a fresh re-sum of a variable node of degree d_v rounds d_v + 1 times (d_v additions of messages,
  one of the channel LLR); a running total has been through two roundings (t = xtot - c, xtot = t + c_new) per edge and
  iteration, 2 it d_v after `it` iterations.  FACTOR(it, d_v) = 2 it d_v / (d_v + 1) is allowed on the 99.9th percentile
  of |out32 - out64| / (1 + |out64|), and twice the oracle's share of words with another hard decision plus one word;
* the (a1, a2, word) record gives back every sent message bit for bit, rows with a zero minimum and with two equal minima
  included;
* LDPC5GDecoder.layered_totals: values, and what it never reaches (boxplus, flooding, return_state).

Measured on this file's inputs (both noise levels pooled; the tests print every figure), 99.9th percentile oracle / specification
and the allowed factor, min-sum: (500, 1000) 3.0e-7 / 3.1e-7 x 1.78 (1 iteration), 3.7e-6 / 5.1e-6 x 5.33 (3), 5.1e-2 / 1.0e-1 x 17.78
(10: the words that do not converge dominate both); (200, 600) 5.2e-7 / 5.3e-7, 3.0e-5 / 3.3e-5, 3.3 / 4.3; (768, 1536) 3.8e-7 / 3.9e-7,
8.9e-6 / 9.8e-6, 1.39 / 1.37.  Words with another hard decision than the anchor (of 48): at most one more than the oracle's."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.ldpc5g import LDPC5GCode
from oracle import ldpc_bp as obp
import ldpc_layered_rt_f32 as spec

CODES = [(64, 128, None, None), (200, 600, None, 2), (500, 1000, None, 4), (768, 1536, "bg2", None)]
# noise: one comfortable level and the one where 10 layered min-sum iterations leave a block error rate near 0.1 (scanned
# with the specification itself: 0.31 / 0.21 / 0.02-0.77 / 0-0.9 between the neighbouring 0.1 steps) - near-ties live there
SIGMA = {(64, 128): (0.6, 0.68), (200, 600): (0.7, 0.93), (500, 1000): (0.7, 0.78), (768, 1536): (0.7, 0.79)}
WORDS = 24
EPS32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _inputs(k, n, bg, m):
    code = LDPC5GCode(k, n, m, bg)
    rng = np.random.default_rng(7 * k + n)
    rows = []
    for sigma in SIGMA[(k, n)]:
        u = rng.integers(0, 2, (WORDS, k)).astype(np.float32)
        y = (2 * code.encode(u) - 1) + sigma * rng.normal(size=(WORDS, n))
        rows.append(2 * y / sigma ** 2)                              # continuous random LLRs, float64
    llr = np.concatenate(rows)
    llr.setflags(write=False)
    return code, llr


def literal_resum(dec, llr5g, num_iter, reverse=False):
    """The re-summing form written out: per layer v2c = clip(-c + xtot) on the layer's edges, check-node update, then every
    variable node summed anew over all its edges (ascending check node, from 0) plus its channel LLR.  dec: an
    oracle LDPC5GDecoder(cn_schedule="layered") of the wanted precision (graph, schedule and node update come from it).
    reverse: the CONTROL - the same form with another, equally valid summation order (channel LLR first, then the edges in
    descending check-node order).  Returns the soft output of all variable nodes."""
    dt, lm = dec.dtype, dec.llr_max
    llr = np.clip(np.asarray(llr5g, dt), -lm, lm).reshape(-1, dec.num_vns).T * dt(-1.)
    vn_of = dec.vn_idx[dec.v2c_perm]
    rag = dec._vn_rag
    c = np.zeros((dec.num_edges, llr.shape[1]), dt)                  # check-node view
    xtot = llr.copy()
    for _ in range(num_iter):
        for pos, lrag in dec._sched:
            v2c = np.clip(dt(-1.) * c[pos] + xtot[vn_of[pos]], -lm, lm)
            c[pos] = dec._cn_update(lrag, v2c, lm)
            msg_vn = c[dec.v2c_perm_inv]
            if not reverse:
                xtot = obp._sum0(rag, msg_vn) + llr
            else:
                xtot = llr.copy()
                for j in range(rag.max_deg - 1, -1, -1):
                    e = rag.by_pos[j]
                    xtot[rag.ids[e]] = xtot[rag.ids[e]] + msg_vn[e]
    return np.clip(xtot, -lm, lm).T * dt(-1.)


@functools.lru_cache(maxsize=None)
def _run(k, n, bg, m, cn, it):
    """soft outputs of all variable nodes: anchor (float64 literal), float64 spec, float32 oracle, float32 spec; the largest
    variable-node degree; beyond 3 iterations the float64 control (literal form, other summation order)"""
    code, llr = _inputs(k, n, bg, m)
    kw = dict(cn_update=cn, num_iter=it, hard_out=False, return_infobits=False)
    o64 = obp.LDPC5GDecoder(code, cn_schedule="layered", precision="double", **kw)
    o32 = obp.LDPC5GDecoder(code, cn_schedule="layered", **kw)
    s64 = spec.LayeredRunningTotal(code, precision="double", **kw)
    s32 = spec.LayeredRunningTotal(code, check_packing=True, **kw)
    l32 = llr.astype(np.float32)
    lit32 = literal_resum(o32, o32.rate_recover(l32), it)
    assert np.array_equal(lit32, o32.decode(o32.rate_recover(l32))), "the literal model is not the oracle"
    ctl = literal_resum(o64, o64.rate_recover(llr), it, reverse=True) if it > 3 else None
    return (literal_resum(o64, o64.rate_recover(llr), it), s64.decode(s64.rate_recover(llr)),
            lit32, s32.decode(s32.rate_recover(l32)), int(o64._vn_rag.deg.max()), ctl)


@pytest.mark.parametrize("cn", ["minsum", "offset-minsum"])
@pytest.mark.parametrize("it", [1, 3, 10])
@pytest.mark.parametrize("k,n,bg,m", CODES)
def test_same_function_in_float64(k, n, bg, m, cn, it):
    """All 48 words, every soft output.  1 and 3 iterations: the 1e-9 of the issue.  10 iterations: 1e-9 does NOT hold on
    the words near a block error rate of 0.1 (measured 1.6e-7 at (200, 600), 1.6e-8 at (768, 1536) min-sum) - a decision,
    recorded in DESIGN.md 4.0f: a word that does not converge makes the min-sum iteration a piecewise-linear map with gain
    above 1, in which ANY rounding difference grows geometrically until the clip stops it.  That claim is asserted, not
    assumed: the CONTROL is the re-summing form itself with another summation order, whose totals differ from the
    anchor's by roundings of d_v + 1 additions.  A running total carries FACTOR(it, d_v) times as many roundings (below),
    the growth is linear in a small perturbation, so the specification may be FACTOR x the control's drift from the
    anchor and no further; where the control stays below 1e-9 / FACTOR the bar is the issue's 1e-9.  Measured, min-sum,
    specification / control: (200, 600) 1.6e-7 / 6.9e-8, (500, 1000) 1.0e-9 / 1.4e-9, (768, 1536) 1.6e-8 / 2.2e-8."""
    anchor, s64, _, _, dv, ctl = _run(k, n, bg, m, cn, it)
    assert anchor.shape == s64.shape == (2 * WORDS, anchor.shape[1]) and anchor.dtype == np.float64
    d = float(np.max(np.abs(anchor - s64)))
    if it <= 3:
        print(f"({k},{n}) {cn} it={it}: max |literal64 - spec64| = {d:.3e}")
        assert d <= 1e-9
        return
    dc = float(np.max(np.abs(anchor - ctl)))
    unsat = np.abs(anchor) < 20.0
    bar = max(1e-9, factor(it, dv) * dc)
    print(f"({k},{n}) {cn} it={it}: max |literal64 - spec64| = {d:.3e}, control (other summation order) {dc:.3e}, "
          f"factor {factor(it, dv):.2f}, bar {bar:.3e}; {int(unsat.sum())} of {unsat.size} outputs not at the clip")
    assert unsat.sum() > 0                                            # the comparison is not all saturated values
    assert d <= bar


def factor(it, dv):
    return 2.0 * it * dv / (dv + 1.0)


def _distance(x32, x64):
    r = np.abs(x32.astype(np.float64) - x64) / (1.0 + np.abs(x64))
    words = float(np.mean(((x32 > 0) != (x64 > 0)).any(axis=1)))
    return float(r.max()), float(np.percentile(r, 99.9)), words


# FACTOR: 2 it d_v roundings behind a running total against d_v + 1 behind a fresh re-sum (module docstring); measured ratios of
# the two 99.9th percentiles stay below 1.95 (docstring), the bar is 1.7 (1 iteration) ... 18.7 (10 iterations, d_v = 14)
# What constrains: the 1- and 3-iteration cases (oracle percentile 2e-7 ... 3e-5, bar 1.7 ... 5.6 times that) and the
# word-share bar.  At 10 iterations the comfortable words sit on the +-llr_max clip (distance ~5e-8 on both sides) and
# the words that do not converge put the ORACLE's own percentile at 5e-2 ... 3.3; times 18 that bar cannot fail.  It is
# kept because the issue sets it, and says nothing there beyond "no worse than the oracle by an order of magnitude".


@pytest.mark.parametrize("cn", ["minsum", "offset-minsum"])
@pytest.mark.parametrize("it", [1, 3, 10])
@pytest.mark.parametrize("k,n,bg,m", CODES)
def test_float32_closeness_against_the_oracles_own(k, n, bg, m, cn, it):
    anchor, _, o32, s32, dv, _ = _run(k, n, bg, m, cn, it)
    omax, op, ow = _distance(o32, anchor)
    smax, sp_, sw = _distance(s32, anchor)
    f = factor(it, dv)
    print(f"({k},{n}) {cn} it={it} d_v={dv}: oracle max {omax:.3e} p99.9 {op:.3e} words {ow:.4f} | "
          f"spec max {smax:.3e} p99.9 {sp_:.3e} words {sw:.4f} | factor {f:.2f}")
    assert sp_ <= f * max(op, EPS32), "running total is further from float64 than its extra roundings explain"
    assert sw <= 2.0 * ow + 1.0 / anchor.shape[0]


def test_record_gives_back_zero_and_equal_minima():
    """the packing on hand-made rows: minimum 0 (sent magnitude 0 on every other edge, signed zeros), two equal minima (one
    magnitude), a unique minimum on the first / last edge, degree 19"""
    rng = np.random.default_rng(3)
    for d in (3, 10, 19):
        v = rng.normal(size=(64, d, 4)).astype(np.float32) * 5
        v[0, 1] = 0.0                                                # minimum 0
        v[1, 0] = 0.0
        v[1, d - 1] = -0.0
        v[2, 0] = 1.5
        v[2, 2] = -1.5                                               # two equal minima ...
        v[2, 1] = 0.25 * np.sign(v[2, 1] + 0.1)
        v[3] = np.abs(v[3]) + 1
        v[3, 0] = 0.5                                                # unique minimum first / last
        v[4] = -np.abs(v[4]) - 1
        v[4, d - 1] = -0.5
        v[5] = np.round(v[5])                                        # integer ties
        rag = obp._Ragged(np.repeat(np.arange(64), d), 64)
        for fn in (obp.cn_update_minsum, obp.cn_update_offset_minsum):
            c = fn(rag, v.reshape(64 * d, 4), np.float32(20.)).reshape(64, d, 4)
            a1, a2, word = spec.pack_records(c)
            assert a1.dtype == np.float32 and word.dtype == np.uint32
            back = spec.unpack_records(a1, a2, word, d)
            assert np.array_equal(back.view(np.uint32), c.view(np.uint32))


def test_layered_totals_property_and_what_it_never_reaches():
    from sionna_amd.phy.fec.ldpc import LDPC5GEncoder, LDPC5GDecoder
    enc = LDPC5GEncoder(200, 600, num_bits_per_symbol=2)
    dec = LDPC5GDecoder(enc, cn_update="minsum", cn_schedule="layered")
    assert dec.layered_totals == "resum" and dec.layered_engine is None
    assert not dec._layered_rt_wanted(False, None)                   # default: today's engine
    for bad in ("total", "", None, 1, "Running"):
        with pytest.raises(ValueError):
            dec.layered_totals = bad
    dec.layered_totals = "running"
    assert dec.layered_totals == "running" and dec._layered_rt_wanted(False, None)
    assert not dec._layered_rt_wanted(True, None)                    # float64
    assert not dec._layered_rt_wanted(False, np.zeros(1))            # msg_v2c
    dec.layered_totals = "resum"
    assert not dec._layered_rt_wanted(False, None)
    for kw in (dict(cn_update="boxplus-phi", cn_schedule="layered"), dict(cn_update="boxplus", cn_schedule="layered"),
               dict(cn_update="minsum"), dict(cn_update="minsum", cn_schedule="layered", return_state=True)):
        d = LDPC5GDecoder(enc, **kw)
        d.layered_totals = "running"
        assert not d._layered_rt_wanted(False, None), kw


def test_entry_declines_rules_and_partially_pruned_rows():
    """samd_ldpc5g_decode_layered_rt_supported on handles built without a device"""
    from sionna_amd import _ffi
    from sionna_amd.phy.fec.ldpc import LDPC5GEncoder, LDPC5GDecoder
    lib = _ffi.lib()

    def handle(enc, nb_pruned):
        h = C.c_void_p()
        with _ffi.option("SAMD_HOST_ONLY", "1"):
            _ffi.check(lib.samd_ldpc5g_create(
                1 if enc._bg == "bg1" else 2, enc._z, enc._bg_rows.ctypes.data_as(C.c_void_p),
                enc._bg_cols.ctypes.data_as(C.c_void_p), enc._bg_shifts.ctypes.data_as(C.c_void_p), len(enc._bg_rows),
                enc._k, enc._n, 0 if enc._num_bits_per_symbol is None else int(enc._num_bits_per_symbol), int(nb_pruned),
                C.byref(h)), "samd_ldpc5g_create")
        return h

    for k, n, bg, m in CODES + [(1024, 2048, "bg1", None), (2816, 8448, "bg1", 6)]:
        enc = LDPC5GEncoder(k, n, num_bits_per_symbol=m, bg=bg)
        lay = LDPC5GDecoder(enc, cn_update="minsum", cn_schedule="layered")
        h = handle(enc, lay._nb_pruned_nodes)
        assert [lib.samd_ldpc5g_decode_layered_rt_supported(h, cn) for cn in range(5)] == [0, 0, 1, 1, 0], (k, n)
        assert lib.samd_ldpc5g_decode_layered_rt_slots(h) >= 1
        assert lib.samd_ldpc5g_decode_layered_rt_workspace_bytes(h, 4096) == 0
        lib.samd_ldpc5g_destroy(h)
    enc = LDPC5GEncoder(500, 1000, num_bits_per_symbol=4)
    flo = LDPC5GDecoder(enc, cn_update="minsum")                     # flooding prunes to the node, not to the base row
    assert flo._nb_pruned_nodes % enc.z != 0
    h = handle(enc, flo._nb_pruned_nodes)
    assert lib.samd_ldpc5g_decode_layered_rt_supported(h, 2) == 0 and lib.samd_ldpc5g_decode_layered_rt_slots(h) == 0
    lib.samd_ldpc5g_destroy(h)
    with _ffi.option("SAMD_NO_ONCHIP_LAYERED", "1"):                   # the switch of the layered engines covers this one too
        h = handle(LDPC5GEncoder(200, 600, num_bits_per_symbol=2), LDPC5GDecoder(LDPC5GEncoder(200, 600, num_bits_per_symbol=2),
                                                                                  cn_update="minsum", cn_schedule="layered")._nb_pruned_nodes)
    assert lib.samd_ldpc5g_decode_layered_rt_supported(h, 2) == 0 and lib.samd_ldpc5g_decode_layered_rt_slots(h) == 0
    lib.samd_ldpc5g_destroy(h)
    assert lib.samd_ldpc5g_decode_layered_rt_supported(None, 2) == 0
