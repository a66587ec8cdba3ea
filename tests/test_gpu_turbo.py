"""The turbo-code kernels of csrc/turbo.hip on the GPU (TurboEncoder, TurboDecoder) against
  - the composition of the existing public blocks in the reference's order (ConvEncoder; BCJRDecoder(hard_out=False) with
    llr_a, the interleaver block, torch subtraction and clamp): the same device code in the same order, array_equal;
  - the specification tests/turbo_f32.py: encoder and maxlog array_equal; map / log soft outputs against the float64
    specification within conv_cases.anchored_bar per codeword, hard decisions where |spec64 LLR| exceeds that bar (at most
    1 % of the bits of a case may be skipped; tests/test_turbo_host.py checks that condition on the CPU).
Shapes: tests/turbo_cases.py."""
import numpy as np
import pytest
import torch

import turbo_cases as tc
import turbo_f32 as spec
from sionna_amd.phy.fec.conv import BCJRDecoder, ConvEncoder
from sionna_amd.phy.fec.turbo import TurboDecoder, TurboEncoder

pytestmark = pytest.mark.gpu
ALGS = ("map", "log", "maxlog")


def _blocks(case, alg="map", hard_out=False, precision=None, interleaver="3GPP"):
    _, code, rate, term, _, _, it, _ = case
    kw = dict(constraint_length=code) if isinstance(code, int) else dict(gen_poly=code)
    enc = TurboEncoder(rate=rate, terminate=term, interleaver_type=interleaver, precision=precision, **kw)
    dec = TurboDecoder(enc, num_iter=it, hard_out=hard_out, algorithm=alg, precision=precision)
    return enc, dec


def _np(t):
    return t.cpu().numpy()


def compose_encode(enc, u):
    """encoding.py:390-417 on the public blocks: ConvEncoder twice, the interleaver block; the re-ordering and puncturing
    are index plumbing on the host"""
    gp, term, k = enc.gen_poly, enc.terminate, u.shape[-1]
    conv = ConvEncoder(gen_poly=gp, rsc=True, terminate=term, precision=enc.precision)
    cw1 = _np(conv(u))
    cw2 = _np(conv(enc.internal_interleaver(u)))
    B, mu = cw1.shape[0], len(gp[0]) - 1
    cw = np.concatenate([cw1[:, :2 * k].reshape(B, k, 2), cw2[:, 1:2 * k:2].reshape(B, k, 1)], axis=-1)
    if term:
        t = np.concatenate([cw1[:, 2 * k:], cw2[:, 2 * k:]], axis=-1)
        S = spec.num_term_syms(mu)
        t = np.concatenate([t, np.zeros((B, 3 * S - t.shape[1]), t.dtype)], axis=-1)
        cw = np.concatenate([cw, t.reshape(B, S, 3)], axis=-2)
    cw = cw.reshape(B, -1)
    return cw[:, spec.punct_mask(cw.shape[1] // 3, enc._coderate_desired)]


def compose_decode(dec, llr, perm):
    """decoding.py:383-432 on the public blocks: BCJRDecoder(hard_out=False) with llr_a, the interleaver block, torch
    subtraction and clamp, in the reference's order.  y1_cw / y2_cw are copies of the input's values (turbo_f32.split)."""
    dt = torch.float64 if dec.precision == "double" else torch.float32
    k, y1, y2 = spec.split(np.asarray(llr), dec.gen_poly, perm, dec.coderate, dec._terminate)
    dev = "cuda"
    y1, y2 = torch.as_tensor(y1, device=dev).to(dt), torch.as_tensor(y2, device=dev).to(dt)
    bcjr = BCJRDecoder(gen_poly=dec.gen_poly, rsc=True, hard_out=False, terminate=dec._terminate, algorithm=dec._algorithm,
                       precision=dec.precision)
    if dt == torch.float32:
        ilv = lambda x, inverse=False: dec.internal_interleaver(x.contiguous(), inverse=inverse)
    else:                                   # the encoder's interleaver is a single-precision block: gather the float64 values by index
        p = torch.as_tensor(np.asarray(perm), device=dev).long()
        ip = torch.argsort(p)
        ilv = lambda x, inverse=False: x[:, ip if inverse else p]
    B, T = y1.shape[0], y1.shape[1] // 2
    ch1, ch2 = y1[:, 0:2 * k:2], y2[:, 0:2 * k:2]
    llr_1e = torch.zeros((B, T), dtype=dt, device=dev)
    terminfo = torch.zeros((B, T - k), dtype=dt, device=dev)
    llr_2i = torch.zeros((B, k), dtype=dt, device=dev)
    for _ in range(dec.num_iter):
        llr_1i = bcjr(y1, llr_a=llr_1e)[:, :k]
        llr_extr = llr_1i - ch1 - llr_1e[:, :k]
        llr_2e = torch.clamp(torch.cat([ilv(llr_extr), terminfo], dim=-1), -20., 20.)
        llr_2i = bcjr(y2, llr_a=llr_2e)[:, :k]
        llr_extr = llr_2i - llr_2e[:, :k] - ch2
        llr_1e = torch.cat([torch.clamp(ilv(llr_extr, inverse=True), -20., 20.), terminfo], dim=-1)
    out = ilv(llr_2i, inverse=True)
    if dec._hard_out:
        out = (0.0 < out).to(dt)
    return _np(out)


# ---------------------------------------------------------------- encoder
@pytest.mark.parametrize("cid", [c for c in tc.SOFT_IDS])
def test_encoder_equals_specification_and_composition(cid):
    case = tc.BY_ID[cid]
    gp, perm, u, c, _ = tc.inputs(cid)
    enc, _ = _blocks(case)
    got = _np(enc(u))
    assert got.dtype == np.float32 and np.array_equal(got, c)
    assert np.array_equal(got, compose_encode(enc, torch.as_tensor(u)))
    assert enc.k == u.shape[1] and got.shape[1] == c.shape[1]
    enc64, _ = _blocks(case, precision="double")
    got64 = _np(enc64(u))
    assert got64.dtype == np.float64 and np.array_equal(got64, c)


# ---------------------------------------------------------------- decoder against the composition of the public blocks
@pytest.mark.parametrize("precision", ["single", "double"])
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("cid", tc.SOFT_IDS)
def test_decoder_equals_composition(cid, alg, precision):
    case = tc.BY_ID[cid]
    _, perm, _, _, llr = tc.inputs(cid)
    for hard in (False, True):
        _, dec = _blocks(case, alg, hard, precision)
        got = _np(dec(llr))
        assert got.dtype == (np.float64 if precision == "double" else np.float32)
        want = compose_decode(dec, llr, perm)
        assert np.array_equal(got, want, equal_nan=True), (cid, alg, precision, hard, np.nanmax(np.abs(got - want)))
        assert dec.k == perm.shape[0] and dec.n == llr.shape[1]


# ---------------------------------------------------------------- decoder against the specification
@pytest.mark.parametrize("cid", tc.SOFT_IDS)
def test_maxlog_equals_specification(cid):
    case = tc.BY_ID[cid]
    gp, perm, u, _, llr = tc.inputs(cid)
    _, _, rate, term, _, _, it, _ = case
    want = spec.decode(llr, gp, perm, rate, term, it, False, "maxlog")
    _, dec = _blocks(case, "maxlog")
    assert np.array_equal(_np(dec(llr)), want)
    _, dec = _blocks(case, "maxlog", hard_out=True)
    assert np.array_equal(_np(dec(llr)), (want > 0).astype(np.float32))
    if cid != "k6144":
        want64 = spec.decode(llr, gp, perm, rate, term, it, False, "maxlog", dtype=np.float64)
        _, dec = _blocks(case, "maxlog", precision="double")
        assert np.array_equal(_np(dec(llr)), want64)


@pytest.mark.parametrize("cid,alg", tc.SOFT_PAIRS)
def test_soft_outputs_within_the_anchored_bar(cid, alg):
    case = tc.BY_ID[cid]
    _, _, _, _, llr = tc.inputs(cid)
    _, r64 = tc.refs(cid, alg)
    bar, sure = tc.bar_and_mask(cid, alg)
    _, dec = _blocks(case, alg)
    got = _np(dec(llr)).astype(np.float64)
    d = np.max(np.abs(got - r64), axis=-1)
    print(f"{cid} {alg}: max |got - spec64| {d.max():.3e}, bar {bar.min():.3e} .. {bar.max():.3e}, share {np.max(d / bar):.2f}, "
          f"bits skipped {1 - sure.mean():.4f}")
    assert np.all(d <= bar), (cid, alg, d, bar)
    assert 1 - sure.mean() <= tc.MAX_SKIPPED
    _, dec = _blocks(case, alg, hard_out=True)
    hard = _np(dec(llr))
    assert set(np.unique(hard)) <= {0.0, 1.0} and np.array_equal(hard[sure], (r64 > 0).astype(np.float32)[sure])


# ---------------------------------------------------------------- batch, input forms, interleaver, construction, LLR edges
def test_batch_zero_and_one():
    case = tc.BY_ID["K4"]
    gp, perm, u, c, llr = tc.inputs("K4")
    enc, dec = _blocks(case, "maxlog", hard_out=False)
    assert tuple(enc(u[:0]).shape) == (0, c.shape[1]) and tuple(dec(llr[:0]).shape) == (0, 40)
    _, _, rate, term, _, _, it, _ = case
    assert np.array_equal(_np(enc(u[:1])), c[:1])
    assert np.array_equal(_np(dec(llr[:1])), spec.decode(llr[:1], gp, perm, rate, term, it, False, "maxlog"))


def test_batch_of_many_waves():
    gp, perm, u, c, llr = tc.inputs("grid")
    _, _, rate, term, _, B, it, _ = tc.BIG_BATCH
    enc, dec = _blocks(tc.BIG_BATCH, "maxlog")
    assert np.array_equal(_np(enc(u)), c)
    got = _np(dec(llr))
    assert got.shape == (B, 40) and np.array_equal(got, spec.decode(llr, gp, perm, rate, term, it, False, "maxlog"))


def test_leading_dimensions_views_and_a_change_of_n():
    case = tc.BY_ID["K3"]                                           # 17 codewords
    gp, perm, u, c, llr = tc.inputs("K3")
    _, _, rate, term, _, _, it, _ = case
    enc, dec = _blocks(case, "maxlog")
    want = spec.decode(llr, gp, perm, rate, term, it, False, "maxlog")
    n = llr.shape[1]
    got = _np(dec(llr[:6].reshape(2, 3, n)))
    assert got.shape == (2, 3, 40) and np.array_equal(got.reshape(6, 40), want[:6])
    assert np.array_equal(_np(enc(u[:6].reshape(2, 3, 40))).reshape(6, n), c[:6])
    wide = torch.zeros((17, 2 * n), device="cuda")
    wide[:, ::2] = torch.as_tensor(llr, device="cuda")
    view = wide[:, ::2]
    assert not view.is_contiguous() and np.array_equal(_np(dec(view)), want)
    # a change of n (and k) between two calls of the same blocks
    gp2, perm2, u2, c2, llr2 = tc.inputs("k33")
    c33 = spec.encode(u2, gp, perm2, rate, term)
    assert np.array_equal(_np(enc(u2)), c33) and enc.k == 33
    llr33 = (3.0 * (2 * c33.astype(np.float32) - 1)).astype(np.float32)
    assert np.array_equal(_np(dec(llr33)), spec.decode(llr33, gp, perm2, rate, term, it, False, "maxlog")) and dec.k == 33
    assert np.array_equal(_np(dec(llr)), want) and dec.k == 40


@pytest.mark.parametrize("rate", [1/3, 1/2])
def test_random_interleaver(rate):
    case = ("rand", 4, rate, True, 45, 9, 4, 4.0)
    enc, dec = _blocks(case, "maxlog", interleaver="random")
    k = 45
    perm = _np(enc.internal_interleaver(torch.arange(k, dtype=torch.float32)[None, :]))[0].astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(k))
    rng = np.random.default_rng(11)
    u = rng.integers(0, 2, (9, k)).astype(np.float32)
    c = spec.encode(u, enc.gen_poly, perm, rate, True)
    assert np.array_equal(_np(enc(u)), c)
    llr = (4.0 * (2 * c.astype(np.float32) - 1) + rng.normal(size=c.shape) * np.sqrt(8.0)).astype(np.float32)
    assert np.array_equal(_np(dec(llr)), spec.decode(llr, enc.gen_poly, perm, rate, True, 4, False, "maxlog"))
    for alg in ("map", "log"):
        d2 = TurboDecoder(enc, num_iter=4, hard_out=False, algorithm=alg)
        assert np.array_equal(_np(d2(llr)), compose_decode(d2, llr, perm), equal_nan=True)


def test_decoder_built_without_an_encoder():
    case = tc.BY_ID["r2T"]
    gp, perm, u, _, llr = tc.inputs("r2T")
    _, _, rate, term, _, _, it, _ = case
    dec = TurboDecoder(gen_poly=gp, rate=rate, terminate=term, interleaver="3GPP", num_iter=it, hard_out=True, algorithm="maxlog")
    got = _np(dec(llr))
    assert np.array_equal(got, spec.decode(llr, gp, perm, rate, term, it, True, "maxlog"))


@pytest.mark.parametrize("alg", ALGS)
def test_llrs_all_zero_and_very_large(alg):
    case = tc.BY_ID["K4"]
    gp, perm, u, c, llr = tc.inputs("K4")
    _, dec = _blocks(case, alg)
    zero = np.zeros_like(llr)
    assert np.array_equal(_np(dec(zero)), compose_decode(dec, zero, perm), equal_nan=True)
    big = (1e4 * (2 * c - 1)).astype(np.float32)
    got = _np(dec(big))
    assert np.array_equal(got, compose_decode(dec, big, perm), equal_nan=True)
    if alg != "map":                                                # map overflows exp(5e3) like the reference does
        assert np.array_equal((got > 0).astype(np.float32), u)
    _, hard = _blocks(case, alg, hard_out=True)
    assert np.array_equal(_np(hard(big)), (got > 0).astype(np.float32))
