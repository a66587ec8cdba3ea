"""CPU validation of the QC kernel algorithms (tests/kernel_models.py) against the oracle."""
import numpy as np
import pytest

from oracle.ldpc5g import LDPC5GCode
from oracle import ldpc_bp as obp
from sionna_amd.phy.fec.ldpc import LDPC5GEncoder, LDPC5GDecoder
from tests.kernel_models import encode_qc_model, decode_onchip_model

CODES = [(64, 128, None, None), (200, 600, None, 2), (1024, 2048, "bg1", None), (500, 1000, None, 4),
         (2816, 8448, "bg1", 6), (1347, 1554, None, None), (8448, 25344, None, None), (3840, 4800, "bg2", None)]


@pytest.mark.parametrize("k,n,bg,m", CODES)
def test_encoder_model_matches_oracle(k, n, bg, m):
    enc = LDPC5GEncoder(k, n, num_bits_per_symbol=m, bg=bg)
    code = LDPC5GCode(k, n, num_bits_per_symbol=m, bg=bg)
    u = np.random.default_rng(k + n).integers(0, 2, (6, k)).astype(np.float32)
    assert np.array_equal(encode_qc_model(enc, u), code.encode(u))


@pytest.mark.parametrize("k,n,bg,m,offset", [(64, 128, None, None, 0.0), (200, 600, None, 2, 0.5),
                                             (100, 200, "bg1", None, 0.0), (400, 480, None, 4, 0.5)])
def test_onchip_decoder_model_bit_exact(k, n, bg, m, offset):
    enc = LDPC5GEncoder(k, n, num_bits_per_symbol=m, bg=bg)
    cn = "offset-minsum" if offset else "minsum"
    dec = LDPC5GDecoder(enc, cn_update=cn, hard_out=False, return_infobits=False)
    code = LDPC5GCode(k, n, num_bits_per_symbol=m, bg=bg)
    odec = obp.LDPC5GDecoder(code, cn_update=cn, hard_out=False, return_infobits=False)
    rng = np.random.default_rng(11)
    u = rng.integers(0, 2, (3, k)).astype(np.float32)
    c = code.encode(u)
    llr = ((2 * c - 1) * 2 + rng.normal(scale=2.0, size=c.shape)).astype(np.float32)
    llr[0, :5] = 0.0                                    # exact zeros / ties
    llr[1] = np.round(llr[1])                           # many duplicate magnitudes
    for it in (0, 1, 3):
        x_model = decode_onchip_model(dec, llr, it, offset)
        ref = obp.LDPCBPDecoder(odec.pcm, cn_update=cn, hard_out=False, num_iter=it)
        x_ref = -ref.decode(odec.rate_recover(llr))     # internal LLR sign
        assert np.array_equal(x_model, x_ref), f"iter {it}"


# ---------------------------------------------------------------------------------------------------------------------
# cir_to_ofdm_channel: the dispatcher and the pass kernel's row ownership in integers, the summation orders in float32
# (tests/kernel_models.py), the latter held to the derived bound of tests/channel_f32.py from both sides.
# ---------------------------------------------------------------------------------------------------------------------
from tests import channel_cases as chc, channel_f32 as chf
from tests import kernel_models as km

C2O_SWEEP_F = (1, 2, 12, 36, 63, 64, 65, 76, 100, 128, 255, 256, 257, 300, 511, 512)


@pytest.mark.parametrize("shape,family,props", chc.TABLE, ids=[chc.sid(s) for s in chc.SHAPES])
def test_c2o_dispatch_reaches_the_table_families(shape, family, props):
    d = km.c2o_dispatch(*shape)
    assert d["family"] == family, d
    for k, v in props.items():
        assert d[k] == v, (k, d)


def test_c2o_dispatch_switches():
    """SAMD_C2O_PASS = 0 is none of the pass widths (8, 4, 2): the register-staged kernel runs; SAMD_C2O_TWO_PASS: the first."""
    for shape, family, _ in chc.TABLE:
        if family == "pass":
            assert km.c2o_dispatch(*shape, pass_width=0)["family"] == "reg"
            for pw in (2, 8):
                assert km.c2o_dispatch(*shape, pass_width=pw) == km.c2o_dispatch(*shape)
        assert km.c2o_dispatch(*shape, two_pass=True)["family"] == "two_pass"
    assert km.c2o_dispatch(4, 2, 23, 14, 76)["fused"] and not km.c2o_dispatch(2, 3, 8, 3, 12)["fused"]
    assert not km.c2o_dispatch(4, 2, 23, 14, 76, num_tx=2)["fused"]


def test_c2o_magic_division_is_exact_over_the_guarded_range():
    """umulhi(n, magic(d)) = n // d for every n the host guard admits (source indices below 8192; units and groups far below)
    and every divisor d <= n_max - and for d up to 8191 at the top of the range."""
    n = np.arange(8192, dtype=np.uint64)
    for d in range(1, 8192):
        assert np.array_equal(km.c2o_divu(n, d, km.c2o_magic(d)), n // np.uint64(d)), d
    assert km.c2o_magic(1) == 0 and km.c2o_magic(2) == 0x80000000 and km.c2o_magic(3) == 0x55555556


@pytest.mark.parametrize("RA", range(1, 9))
def test_c2o_pass_kernel_row_ownership(RA):
    """Every shape the dispatcher sends to the pass kernel, RA, TA in 1 ... 8, T in 1 ... 16, F over the block-size edges and
    every path class: staging is injective into the padded tap table, RowWalk reports for register r of group g the
    (ra, ta, t) whose taps staging put in row g + r G, every real row is stored exactly once and no padded row is, and in
    grouped mode the TA rows of a unit are consecutive registers of one thread (the fused kernel sums over them in place)."""
    seen = dict(pass_=0, grouped=0, ungrouped=0, fused=0)
    for TA in range(1, 9):
        for T in range(1, 17):
            for nf in C2O_SWEEP_F:
                for P in (1, 8, 9, 16, 17, 24, 25, 32):
                    d = km.c2o_dispatch(RA, TA, P, T, nf)
                    if d["family"] != "pass":
                        assert not d["fused"]                        # fused and separate entries run the same chain, or fused refuses
                        continue
                    G, RPT, grouped = d["G"], d["RPT"], d["grouped"]
                    assert RA * TA * P * T < 8192 and d["nt"] == G * nf + d["spare"] and G >= 1
                    lk, t, row = km.c2o_stage_rows(RA, TA, P, T, G, RPT, P - 1)
                    lk0, t0, row0 = km.c2o_stage_rows(RA, TA, P, T, G, RPT, 0)
                    rows = RA * TA * T
                    assert np.array_equal(lk, np.repeat(np.arange(RA * TA), T)) and np.array_equal(t, np.tile(np.arange(T), RA * TA))
                    assert np.array_equal(row, row0) and np.array_equal(lk, lk0) and np.array_equal(t, t0)
                    assert row.min() >= 0 and row.max() < RPT * G and np.unique(row).size == rows, (RA, TA, P, T, nf)
                    if P not in (8, 32):
                        continue                                     # the walk does not depend on the path count
                    w_ra, w_ta, w_t = km.c2o_row_walk(RA, TA, T, G, RPT, grouped)
                    g, r = row % G, row // G
                    key = (lk // TA, lk % TA, t)
                    got = (w_ra[g, r], w_ta[g, r], w_t[g, r])
                    assert all(np.array_equal(x, y) for x, y in zip(got, key)), (RA, TA, P, T, nf)
                    stored = w_ra < RA
                    assert int(stored.sum()) == rows                 # with the line above: each real row once, no padded row
                    if grouped:
                        first = row[(lk % TA) == 0]
                        for k in range(1, TA):
                            nxt = row[(lk % TA) == k]
                            assert np.array_equal(nxt % G, first % G) and np.array_equal(nxt // G, first // G + k)
                        assert np.all((first // G) % TA == 0)        # a unit starts where the fused kernel resets its sum
                    if d["fused"]:
                        assert grouped
                        seen["fused"] += 1
                    seen["pass_"] += 1
                    seen["grouped" if grouped else "ungrouped"] += 1
    assert seen["grouped"] and seen["ungrouped"] and seen["fused"], seen


@pytest.fixture(scope="module")
def c2o_case():
    cache = {}

    def get(shape, normalize):
        if (shape, normalize) not in cache:
            fr, a, tau = chc.make(shape)
            cache[(shape, normalize)] = (fr, a, tau, chf.anchor(fr, a, tau, normalize), chf.bound(fr, a, tau, normalize))
        return cache[(shape, normalize)]
    return get


def _c2o_chains(d):
    return ("one", "uv", "pass") if d["family"] == "pass" else ("one", "uv")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", chc.SHAPES, ids=chc.sid)
def test_c2o_restatements_lie_inside_the_bound(c2o_case, shape, normalize):
    """the bound is not too tight: every summation order, with host sin / cos, stays inside it on every output"""
    fr, a, tau, ref, bd = c2o_case(shape, normalize)
    d = km.c2o_dispatch(*shape)
    outs = {}
    for chain in _c2o_chains(d):
        h = km.c2o_model_f32(fr, a, tau, normalize, d, chain=chain)
        outs[chain] = h
        err = np.abs(h.astype(np.complex128) - ref)
        assert np.all(err <= bd), (chain, float(np.max(err / np.maximum(bd, 1e-300))))
    if "pass" in outs and not normalize:
        assert np.array_equal(outs["pass"], outs["one"])             # padded passes add exact zeros: the same chain


@pytest.mark.parametrize("mutation", km.C2O_MUTATIONS)
@pytest.mark.parametrize("shape", chc.SHAPES, ids=chc.sid)
def test_c2o_seeded_faults_leave_the_bound(c2o_case, shape, mutation):
    """the bound is not too loose: each seeded fault of the restatement exceeds it on at least one output"""
    normalize = mutation == "inv_neighbour"
    fr, a, tau, ref, bd = c2o_case(shape, normalize)
    d = km.c2o_dispatch(*shape)
    h = km.c2o_model_f32(fr, a, tau, normalize, d, mutation=mutation)
    assert np.any(np.abs(h.astype(np.complex128) - ref) > bd), (shape, mutation)


def test_c2o_bound_edges():
    """a link without energy: anchor and bound are exactly 0 under normalisation, the other links are untouched; tau = 0
    leaves only the accumulation term (and the exact cos 0 = 1 within the sin / cos allowance)"""
    shape = (2, 3, 8, 3, 12)
    fr, a, tau = chc.make(shape)
    a0 = a.copy()
    a0[1, 0, :, 1] = 0
    r0, b0 = chf.anchor(fr, a0, tau, True), chf.bound(fr, a0, tau, True)
    assert np.all(r0[1, 0, :, 1] == 0) and np.all(b0[1, 0, :, 1] == 0) and np.all(np.isfinite(r0)) and np.all(np.isfinite(b0))
    keep = np.ones(r0.shape, bool)
    keep[1, 0, :, 1] = False
    assert np.array_equal(r0[keep], chf.anchor(fr, a, tau, True)[keep])
    d = km.c2o_dispatch(*shape)
    h0 = km.c2o_model_f32(fr, a0, tau, True, d)
    assert np.all(h0[1, 0, :, 1] == 0) and np.all(np.abs(h0 - r0) <= b0)
    bz = chf.bound(fr, a, np.zeros_like(tau), False)
    amp = np.abs(a.astype(np.complex128)).sum(axis=5)[..., None]
    assert np.allclose(bz, (2 * chf.C_SC * chf.U + np.sqrt(2) * chf._gamma(18) * (1 + 8 * chf.U)) * amp + 2.0 ** -50 * 8 * amp, rtol=1e-12)
