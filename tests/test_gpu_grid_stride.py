"""Streaming kernels past one trip of their grid-stride loop, and launch-path branches no other test takes.

Every element-wise kernel of the hot path runs ``for (i = global thread; i < n; i += gridDim.x * blockDim.x)`` under a
capped grid, so up to ``cap * work items per workgroup`` work items every thread runs the loop body exactly once: the
software-pipelined prefetches of ``qam_map_kernel`` / ``demap_square_qam_kernel``, the ``s * M`` address arithmetic of a later
trip and the accumulation across trips of ``count_errors_kernel`` / ``crc_kernel`` never execute.  The tests below hold each
kernel to its oracle at

    N1 = threshold + 1                   work items   (exactly one work item takes a second trip)
    N2 = 2 * threshold + 256 * 37 + 19   work items   (a partly filled third trip, a tail that is no multiple of 64)

with the bar of the kernel's existing small-size test against the same oracle (named at each test; no new tolerance).  Where a
hard-decision output has no such bar (SymbolDemapper with a prior, LLRs2SymbolLogits, SymbolLogits2LLRs) the criterion is derived
from the soft bar of the same case and says so.

Position-independent operations get a periodic input: one random block of P = 10007 (prime) items is tiled to the full
length, the float64 oracle runs once on the block and the comparison happens on the device against ``got`` viewed as
(reps, P, ...) plus the tail.  The stride is a power of two, so ``stride mod P != 0`` and a read from the wrong trip lands
on a different value.  Kernels on Philox counters (BinarySource, AWGN, the float64 TDL taps) are position dependent and are
compared over their whole length on the host.

Largest tensors of one case (device): Mapper m = 8 at N2, bits 4.2 M x 8 float32 = 134 MB; Demapper m = 8 at N2, LLRs 134 MB
(+ a float64 comparison chunk of <= 128 MB); SymbolDemapper m = 4 at N1, logits and prior 2.1 M x 16 float32 = 134 MB each;
LLRs2SymbolLogits at N2, 1.66 M x 16 float32 = 106 MB; float64 ApplyTimeChannel at N1, h 268 MB.  Every case stays below 1 GB.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mapping as omap, utils as outil, ofdm as o, f64_ofdm as o64, polar as op

# ---------------------------------------------------------------------------------------------------------------------
# Launch geometry, read from the launch code.  ``unit``: elements of the entry point's size argument that ONE work item
# (a thread, or a wave for the two reductions, or a workgroup tile for llrs2logits) handles; ``per_wg``: work items per
# workgroup; ``cap``: the most workgroups the launch asks for.  threshold = cap * per_wg work items fill exactly one trip.
#   name                 unit  per_wg  cap        launch line
GEOMETRY = {
    "qam_map":          (1,    256,    256 * 32,  "mapping.hip:240 (grid_for, mapping.hip:230-233)"),
    "square_qam_demap": (1,    256,    256 * 32,  "mapping.hip:261"),
    "qam_demap":        (1,    256,    256 * 32,  "mapping.hip:279"),
    "qam_demap_prior":  (1,    256,    256 * 32,  "mapping.hip:295"),
    "symbol_demap":     (1,    256,    256 * 32,  "mapping.hip:522"),
    "logits2llrs":      (1,    256,    256 * 32,  "mapping.hip:382"),
    "llrs2logits":      (64,   1,      256 * 32,  "mapping.hip:485: grid_for((rows + 63) / 64 * 256, 256), a workgroup per 64 rows"),
    "logits2moments":   (1,    256,    256 * 32,  "mapping.hip:496"),
    "pam2qam":          (1,    256,    256 * 32,  "mapping.hip:507: grid_for(rows << m, 256), a thread per OUTPUT element"),
    "binary_source":    (4,    256,    256 * 32,  "channel.hip:80: grid_for((n + 3) / 4, 256), a thread per 4 bits"),
    "awgn":             (2,    256,    256 * 32,  "channel.hip:90: grid_for((n + 1) / 2, 256), a thread per 2 samples"),
    "rg_map":           (1,    256,    256 * 32,  "ofdm.hip:755 (grid_for, ofdm.hip:744-747), a thread per grid element"),
    "gather3":          (1,    256,    256 * 32,  "ofdm.hip:772, a thread per output element"),
    "apply_ofdm":       (1,    256,    256 * 32,  "ofdm.hip:933, a thread per output element"),
    "lin_interp":       (1,    256,    256 * 32,  "ofdm.hip:998, a thread per output element"),
    "ls_gather_scale":  (1,    256,    256 * 32,  "ofdm.hip:1023, a thread per output element"),
    "count_errors":     (1,    4,      256 * 16,  "metrics.hip:52-53, a wave per block, 4 waves per workgroup"),
    "crc":              (1,    4,      256 * 8,   "polar.hip:463-464, a wave per word, 4 waves per workgroup"),
    # float64 twins
    "qam_demap_f64":        (1, 256, 256 * 32, "f64.hip:723"),
    "symbol_demap_f64":     (1, 256, 256 * 32, "f64_mapping.hip:159 (grid_for64, f64_mapping.hip:15-18)"),
    "logits2llrs_f64":      (1, 256, 256 * 32, "f64_mapping.hip:171"),
    "llrs2logits_f64":      (1, 256, 256 * 32, "f64_mapping.hip:181, a thread per row (unlike the float32 kernel)"),
    "logits2moments_f64":   (1, 256, 256 * 32, "f64_mapping.hip:191"),
    "pam2qam_f64":          (1, 256, 256 * 32, "f64_mapping.hip:202, a thread per output element"),
    "awgn_f64":             (2, 256, 256 * 32, "f64_ofdm.hip:210 (grid_for, f64_ofdm.hip:195-198), a thread per 2 samples"),
    "rg_map_f64":           (1, 256, 256 * 32, "f64_ofdm.hip:220"),
    "apply_ofdm_f64":       (1, 256, 256 * 32, "f64_ofdm.hip:257"),
    "ls_gather_scale_f64":  (1, 256, 256 * 32, "f64_ofdm.hip:267"),
    "lin_interp_f64":       (1, 256, 256 * 32, "ofdm.hip:1012"),
    "tdl_cir_f64":          (1, 256, 256 * 32, "f64_ofdm.hip:231, a thread per tap sample a[b, ra, ta, p, t]"),
    "cir_to_ofdm_f64":      (1, 256, 256 * 32, "f64_ofdm.hip:244, a thread per output element"),
    "cir_to_time_f64":      (1, 256, 256 * 32, "f64_time.hip:106 (grid_for_t, f64_time.hip:90-93), a thread per output element"),
    "apply_time_f64":       (1, 256, 256 * 32, "f64_time.hip:120, a thread per output sample"),
}
P = 10007                                  # period of the tiled inputs (prime)
SIZES = ["N1", "N2"]


def threshold(name):
    """Work items that fill exactly one trip of the kernel's grid-stride loop."""
    _, per_wg, cap, _ = GEOMETRY[name]
    return cap * per_wg


def work_items(name, size):
    t = threshold(name)
    return t + 1 if size == "N1" else 2 * t + 256 * 37 + 19


def elements(name, size, rest=1):
    """Size argument that makes ``work_items(name, size)`` work items, the last one holding ``rest`` (< unit) elements."""
    unit = GEOMETRY[name][0]
    n = unit * (work_items(name, size) - 1) + min(rest, unit)
    assert -(-n // unit) > threshold(name), (name, size, n)            # a test at or below the threshold tests nothing new
    return n


def stride_items(name):
    return threshold(name) * GEOMETRY[name][0]


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else x


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tile(block, n):
    """[p, ...] host block -> [n, ...] device tensor, the block repeated."""
    t = _dev(block)
    reps = -(-n // t.shape[0])
    return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()


def _bad_items(got, ref, pred):
    """got [n, ...] on the device against the periodic reference ref [p, ...]: bool [n], True where ``pred(got, ref)`` (element
    wise "is wrong") holds for any entry of the item.  Chunked so that a float64 temporary stays below 128 MB."""
    got = _t(got)
    n, p = got.shape[0], ref.shape[0]
    assert got.shape[1:] == ref.shape[1:], (got.shape, ref.shape)
    per = max(1, int(np.prod(got.shape[1:])))
    step = max(1, (1 << 24) // (p * per)) * p
    out = torch.empty(n, dtype=torch.bool, device=got.device)
    for start in range(0, n, step):
        g = got[start:min(n, start + step)]
        full = g.shape[0] // p
        parts = []
        if full:
            parts.append(pred(g[:full * p].reshape((full, p) + tuple(g.shape[1:])), ref[None]).reshape((full * p,) + tuple(g.shape[1:])))
        if g.shape[0] % p:
            parts.append(pred(g[full * p:], ref[:g.shape[0] - full * p]))
        b = torch.cat(parts)
        out[start:start + g.shape[0]] = b.reshape(b.shape[0], -1).any(1)
    return out


def _report(bad, stride, what):
    """Fail with the index pattern of the wrong items: how many per trip of the loop, the first one and its lane."""
    nbad = int(bad.sum())
    if nbad == 0:
        return
    idx = torch.nonzero(bad).reshape(-1)
    trips = torch.bincount(idx // stride).tolist()
    first = int(idx[0])
    raise AssertionError(f"{what}: {nbad} of {bad.numel()} items wrong; per trip {trips}; first item {first} "
                         f"(trip {first // stride}, workgroup {(first % stride) // 256}, lane {first % 64})")


def _close_pred(rtol, atol):
    """np.allclose's rule, |got - ref| <= atol + rtol |ref|, in the reference's (double) precision."""
    def pred(g, r):
        return ~((g.to(r.dtype) - r).abs() <= atol + rtol * r.abs())
    return pred


def _exact_pred(g, r):
    return g != r.to(g.dtype)


def _check_periodic(got, ref_block, pred, name, what):
    got = _t(got)
    ref = _dev(np.ascontiguousarray(ref_block))
    stride = stride_items(name)
    assert got.shape[0] > stride and stride % ref.shape[0] != 0
    _report(_bad_items(got, ref, pred), stride, what)


# ===================================================================================================== mapping.hip
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("m", [2, 4, 6, 8, 3])
def test_mapper_past_one_trip(phy, m, size):
    """qam_map_kernel<2|4|6|8> and the run-time-m instantiation (m = 3, a custom constellation): bit-exact like
    test_gpu_parity.py::test_mapper_bit_exact.  The second trip reads the bits the prefetch (nxt[] <- bits[s2 * m + i]) fetched."""
    n = elements("qam_map", size)
    rng = np.random.default_rng(m)
    bits = rng.integers(0, 2, (P, m)).astype(np.float32)
    k = stride_items("qam_map") % P              # the one second-trip symbol of N1 is symbol k of the period: a prefetch that
    if np.array_equal(bits[0], bits[k]):         # re-reads the first trip's symbol 0 must see other bits there
        bits[0, 0] = 1 - bits[0, 0]
    if m % 2 == 0:
        pts, mapper = omap.qam(m), phy.mapping.Mapper("qam", m)
    else:
        const = phy.mapping.Constellation("custom", m, points=(rng.normal(size=1 << m) + 1j * rng.normal(size=1 << m)).astype(np.complex64))
        pts, mapper = np.asarray(const()).astype(np.complex64), phy.mapping.Mapper(constellation=const)
    ref = omap.mapper(bits.reshape(-1), pts)                                    # [P]
    got = mapper(_tile(bits, n).reshape(-1))
    assert got.shape == (n,)
    _check_periodic(torch.view_as_real(_t(got)), np.stack([ref.real, ref.imag], -1), _exact_pred, "qam_map", f"Mapper m={m} {size}")


@functools.lru_cache(maxsize=None)
def _demap_case(m, method, per_symbol_no):
    """Inputs drawn like test_gpu_parity.py::test_demapper_vs_oracle (points + 0.3 noise; no = 0.2 or U(0.01, 100) per symbol)
    for one period, and the float64 oracle on them."""
    rng = np.random.default_rng(10 + m)
    pts = omap.qam(m)
    y = (pts[rng.integers(0, 2 ** m, P)] + (rng.normal(size=P) + 1j * rng.normal(size=P)) * 0.3).astype(np.complex64)
    no = rng.uniform(0.01, 100, size=P).astype(np.float32) if per_symbol_no else np.float32(0.2)
    k = stride_items("square_qam_demap") % P     # the one second-trip symbol of N1 is symbol k of the period
    y[0] = -y[k]                                 # ... and symbol 0, which a stale prefetch would hand it, decides every bit's axis the other way
    ref64 = omap.demapper(y.astype(np.complex128), np.asarray(no, np.float64), pts.astype(np.complex128), method).reshape(P, m)
    differ = (ref64[0] > 0) != (ref64[k] > 0)
    assert (differ & (np.abs(ref64[0]) > 1e-3) & (np.abs(ref64[k]) > 1e-3)).any()      # so hard decisions tell the two apart at N1 too
    return y, no, ref64


def _demapper_past_one_trip(phy, kernel, m, method, per_symbol_no, separable, size, hard=False):
    n = elements(kernel, size)
    y, no, ref64 = _demap_case(m, method, per_symbol_no)
    yd = _tile(y, n)
    nod = _tile(no, n) if per_symbol_no else no
    got = phy.mapping.Demapper(method, "qam", m, separable=separable, hard_out=hard)(yd, nod)
    assert got.shape == (n * m,)
    what = f"Demapper m={m} {method} {'per-symbol' if per_symbol_no else 'scalar'} no separable={separable} hard={hard} {size}"
    if hard:
        # test_demapper_vs_oracle: decisions compared where |ref| > 1e-3
        pred = lambda g, r: (g != (r > 0).to(g.dtype)) & (r.abs() > 1e-3)
    else:
        # test_demapper_vs_oracle: rtol 1e-5, atol 1e-4 * max(1, 1e-2 * max |ref64|)
        pred = _close_pred(1e-5, 1e-4 * max(1.0, float(np.max(np.abs(ref64))) * 1e-2))
    _check_periodic(_t(got).reshape(n, m), ref64, pred, kernel, what)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("per_symbol_no", [False, True])
@pytest.mark.parametrize("method", ["app", "maxlog"])
@pytest.mark.parametrize("m", [2, 4, 6, 8])
def test_demapper_separable_past_one_trip(phy, m, method, per_symbol_no, size):
    """demap_square_qam_kernel: the second trip works on ynext / nnext, fetched from y[s + stride] / no[s + stride]."""
    _demapper_past_one_trip(phy, "square_qam_demap", m, method, per_symbol_no, True, size)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("per_symbol_no", [False, True])
@pytest.mark.parametrize("method", ["app", "maxlog"])
@pytest.mark.parametrize("m", [4, 6])
def test_demapper_generic_past_one_trip(phy, m, method, per_symbol_no, size):
    """demap_kernel<M, MAXLOG> (separable=False)."""
    _demapper_past_one_trip(phy, "qam_demap", m, method, per_symbol_no, False, size)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("separable", [True, False])
def test_demapper_hard_out_past_one_trip(phy, separable, size):
    """hard_out of both demapper kernels.  _demap_case makes symbol 0 and the one second-trip symbol of N1 decide differently, so a
    wrong-trip read shows in hard decisions at N1 as well."""
    _demapper_past_one_trip(phy, "square_qam_demap" if separable else "qam_demap", 4, "app", True, separable, size, hard=True)


@functools.lru_cache(maxsize=None)
def _prior_case(method, per_symbol):
    """Drawn like test_gpu_parity.py::test_demapper_with_prior: y ~ CN(0, 2), no ~ U(0.05, 1), prior 2 N(0,1) [m] or 3 N(0,1)
    [n, m]; the oracle called the same way (complex64 in).  The [m] case carries the scalar no."""
    m = 4
    rng = np.random.default_rng(m)
    y = (rng.normal(size=P) + 1j * rng.normal(size=P)).astype(np.complex64)
    no = rng.uniform(0.05, 1.0, P).astype(np.float32) if per_symbol else np.float32(0.2)
    prior = (rng.normal(size=(P, m)) * 3 if per_symbol else rng.normal(size=m) * 2).astype(np.float32)
    ref = omap.demapper(y, no, omap.qam(m), method, prior=prior)
    return y, no, prior, ref.reshape(P, m)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("per_symbol", [False, True])
@pytest.mark.parametrize("method", ["app", "maxlog"])
def test_demapper_prior_past_one_trip(phy, method, per_symbol, size):
    """demap_kernel with the a-priori term, prior [m] (+ scalar no) and [n, m] (+ per-symbol no): prior[s * M + i] on a later
    trip.  Bar of test_demapper_with_prior: rtol 1e-4, atol 2e-4; hard decisions where |ref| > 1e-3 (test_demapper_vs_oracle)."""
    m = 4
    n = elements("qam_demap_prior", size)
    y, no, prior, ref = _prior_case(method, per_symbol)
    args = (_tile(y, n), _tile(no, n) if per_symbol else no, _tile(prior, n) if per_symbol else prior)
    got = phy.mapping.Demapper(method, "qam", m)(*args)
    _check_periodic(_t(got).reshape(n, m), ref, _close_pred(1e-4, 2e-4), "qam_demap_prior", f"Demapper prior {method} per_symbol={per_symbol} {size}")
    if method == "app":
        hard = phy.mapping.Demapper(method, "qam", m, hard_out=True)(*args)
        _check_periodic(_t(hard).reshape(n, m), ref, lambda g, r: (g != (r > 0).to(g.dtype)) & (r.abs() > 1e-3), "qam_demap_prior",
                        f"Demapper prior hard per_symbol={per_symbol} {size}")


@functools.lru_cache(maxsize=None)
def _symbol_demap_case(m, per_symbol):
    """Drawn like test_gpu_ofdm.py::test_symbol_demapper_vs_oracle: points + 0.2 noise, no = 0.3 or U(0.05, 2) per symbol, prior
    N(0,1) on the points ([2^m] there; [n, 2^m] for the per-symbol case)."""
    rng = np.random.default_rng(m)
    pts = omap.qam(m)
    y = (pts[rng.integers(0, 2 ** m, P)] + 0.2 * (rng.normal(size=P) + 1j * rng.normal(size=P))).astype(np.complex64)
    no = rng.uniform(0.05, 2.0, P).astype(np.float32) if per_symbol else np.float32(0.3)
    prior = rng.normal(size=(P, 1 << m) if per_symbol else (1 << m,)).astype(np.float32)
    e = omap.symbol_demapper(y, no, pts, prior)
    return y, no, prior, e


def _symbol_demap_check(phy, m, per_symbol, n):
    y, no, prior, ref = _symbol_demap_case(m, per_symbol)
    args = (_tile(y, n), _tile(no, n) if per_symbol else no, _tile(prior, n) if per_symbol else prior)
    got = phy.mapping.SymbolDemapper("qam", m)(*args)
    assert got.shape == (n, 1 << m)
    # bar of test_symbol_demapper_vs_oracle's prior case: rtol 1e-5, atol 2e-3.  The per-symbol prior runs the same arithmetic
    # (e + pr[c]); only the address of pr differs (prior + s * P), which is what these sizes are about.
    bad = _bad_items(got, _dev(ref), _close_pred(1e-5, 2e-3))
    # hard decisions - a DERIVED bar, not one of an existing test (test_symbol_demapper_vs_oracle compares hard decisions only
    # without a prior, exactly): the soft bar bounds every exponent's error by 2e-3 (+ 1e-5 relative), so the most likely point
    # must be the oracle's wherever its float64 lead over the runner-up exceeds twice that (ref holds log-probabilities, the
    # lead is the difference of the two largest); more than 99 % of the symbols are that clear
    hard = phy.mapping.SymbolDemapper("qam", m, hard_out=True)(*args)
    assert hard.dtype == torch.int32 and hard.shape == (n,)
    top2 = np.sort(ref, axis=-1)[:, -2:]
    sure = _dev((top2[:, 1] - top2[:, 0]) > 2 * (2e-3 + 1e-5 * np.abs(top2).max(-1)))
    arg = _dev(np.argmax(ref, axis=-1).astype(np.int32))
    reps = -(-n // P)
    arg_n, sure_n = arg.repeat(reps)[:n], sure.repeat(reps)[:n]
    assert float(sure.float().mean()) > 0.99
    return bad, (_t(hard) != arg_n) & sure_n


def test_symbol_demapper_per_symbol_prior_one_period(phy):
    """The small-size test the big ones borrow from: SymbolDemapper with a per-symbol prior [n, 2^m] has no float32 oracle
    test elsewhere (test_symbol_demapper_vs_oracle gives the prior per point only); same draw, same bar, one period."""
    for m in (2, 4):
        bad, bad_hard = _symbol_demap_check(phy, m, True, P)
        assert not bool(bad.any()) and not bool(bad_hard.any()), (m, int(bad.sum()), int(bad_hard.sum()))


@pytest.mark.parametrize("m,size,per_symbol", [(2, "N1", True), (2, "N2", True), (4, "N1", True), (2, "N1", False)])
def test_symbol_demapper_past_one_trip(phy, m, size, per_symbol):
    """symbol_demap_kernel, soft and hard, per-symbol no and prior (prior + s * P) and one scalar-no / [2^m]-prior case.
    N2 only for m = 2 (logits 4.2 M x 4 float32 = 67 MB)."""
    n = elements("symbol_demap", size)
    bad, bad_hard = _symbol_demap_check(phy, m, per_symbol, n)
    _report(bad, stride_items("symbol_demap"), f"SymbolDemapper m={m} {size} soft")
    _report(bad_hard, stride_items("symbol_demap"), f"SymbolDemapper m={m} {size} hard")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("method,per_row_prior", [("app", True), ("maxlog", True), ("app", False)])
def test_symbol_logits2llrs_past_one_trip(phy, method, per_row_prior, size):
    """logits2llrs_kernel<4>: rows of 16 logits (3 N(0,1)) with priors 2 N(0,1) per row or [m], drawn like the fixture of
    test_gpu_parity.py::test_symbol_logits2llrs_block; its bar against the float64 oracle: max |err| <= 2e-5 max(1, max |ref|)."""
    m = 4
    n = elements("logits2llrs", size)
    rng = np.random.default_rng(41)
    z = (3.0 * rng.normal(size=(P, 1 << m))).astype(np.float32)
    prior = (2.0 * rng.normal(size=(P, m) if per_row_prior else (m,))).astype(np.float32)
    ref = omap.symbol_logits2llrs(z, m, method, prior)
    got = phy.mapping.SymbolLogits2LLRs(method, m)(_tile(z, n), _tile(prior, n) if per_row_prior else prior)
    assert got.shape == (n, m)
    bar = 2e-5 * max(1.0, float(np.abs(ref).max()))
    _check_periodic(got, ref, _close_pred(0.0, bar), "logits2llrs", f"SymbolLogits2LLRs {method} per_row_prior={per_row_prior} {size}")
    if method == "app" and per_row_prior:
        # hard_out (exact against the executed reference in the small test): derived from the soft bar - the decision is the
        # oracle's wherever |ref| exceeds it
        hard = phy.mapping.SymbolLogits2LLRs(method, m, hard_out=True)(_tile(z, n), _tile(prior, n))
        _check_periodic(hard, ref, lambda g, r: (g != (r > 0).to(g.dtype)) & (r.abs() > bar), "logits2llrs",
                        f"SymbolLogits2LLRs hard {size}")


@pytest.mark.parametrize("size", SIZES)
def test_llrs2symbol_logits_past_one_trip(phy, size):
    """llrs2logits_kernel: a workgroup per tile of 64 rows, so one trip is 8192 tiles = 524288 rows; the last tile holds 19 rows.
    LLRs 5 N(0,1) and the bar of test_gpu_symbol.py::test_llrs2symbol_logits_and_inds2bits (``close``): max |err| <= 4e-5 max(1,
    max |ref|) against the float64 oracle.  hard_out: that test asks for agreement on > 99.9 % of the rows; the criterion here is
    DERIVED from the soft bar instead, so that it can name the rows: the index must be the oracle's on every row whose float64 lead
    over the runner-up exceeds twice the soft bar (more than 99 % of the rows).  The 19 rows of the last tile at N1 are the whole second
    trip, so the hard case has its power at N2."""
    m = 4
    rows = elements("llrs2logits", size, rest=19)
    assert rows > threshold("llrs2logits") * 64
    llrs = (np.random.default_rng(m).normal(size=(P, m)) * 5).astype(np.float32)
    ref = omap.llrs2symbol_logits(llrs, m)
    x = _tile(llrs, rows)
    got = phy.mapping.LLRs2SymbolLogits(m)(x)
    assert got.shape == (rows, 1 << m)
    bar = 4e-5 * max(1.0, float(np.abs(ref).max()))
    _check_periodic(got, ref, _close_pred(0.0, bar), "llrs2logits", f"LLRs2SymbolLogits {size}")
    hard = _t(phy.mapping.LLRs2SymbolLogits(m, hard_out=True)(x))
    top2 = np.sort(ref, -1)[:, -2:]
    sure = _dev(top2[:, 1] - top2[:, 0] > 2 * bar)
    reps = -(-rows // P)
    wrong = (hard != _dev(np.argmax(ref, -1).astype(np.int32)).repeat(reps)[:rows]) & sure.repeat(reps)[:rows]
    assert float(sure.float().mean()) > 0.99
    _report(wrong, stride_items("llrs2logits"), f"LLRs2SymbolLogits hard {size}")


@functools.lru_cache(maxsize=None)
def _moments_case():
    m = 4
    logits = (np.random.default_rng(17).normal(size=(P, 1 << m)) * 3).astype(np.float32)     # 3 N(0,1) like the fixture of test_moments_and_pam_qam
    mean, var = omap.symbol_logits2moments(logits, omap.qam(m))
    return logits, mean, var


# SymbolLogits2Moments has no small float32 test against oracle.mapping: test_gpu_symbol.py::test_moments_and_pam_qam holds it
# to the executed reference with ``close``, max |err| <= 4e-5 max(1, max |ref|).  _moments_f32 below states the oracle in float32
# (every intermediate rounded, the 16 points summed in order like the kernel); against the float64 oracle on this period it is
# off by at most 3.5e-7 in the mean (max |mean| 1.34) and 4.1e-7 in the variance (max 1.69), measured on the CPU and asserted in
# test_moments_bar_covers_float32_rounding.  That is two orders below the bar, which therefore applies unchanged here.
MOMENTS_BAR = 4e-5


def _moments_f32(logits, points):
    z = np.asarray(logits, np.float32)
    p = np.exp(z - z.max(-1, keepdims=True), dtype=np.float32)
    p = (p / p.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    pts = np.asarray(points, np.complex64)
    mean = np.zeros(z.shape[:-1], np.complex64)
    for c in range(len(pts)):
        mean = (mean + p[..., c] * pts[c]).astype(np.complex64)
    d2 = (np.abs(pts - mean[..., None]) ** 2).astype(np.float32)
    var = np.zeros(z.shape[:-1], np.float32)
    for c in range(len(pts)):
        var = (var + p[..., c] * d2[..., c]).astype(np.float32)
    return mean, var


def test_moments_bar_covers_float32_rounding():
    """Host arithmetic only: the float32 statement of the oracle stays within 1e-6 of its float64 form (measured 3.5e-7 / 4.1e-7)."""
    logits, mean, var = _moments_case()
    m32, v32 = _moments_f32(logits, omap.qam(4))
    assert np.abs(m32 - mean).max() <= 1e-6 and np.abs(v32 - var).max() <= 1e-6


def _moments_check(phy, n):
    logits, mean, var = _moments_case()
    gm, gv = phy.mapping.SymbolLogits2Moments("qam", 4)(_tile(logits, n))
    assert gm.shape == (n,) and gv.shape == (n,)
    bm = _bad_items(torch.view_as_real(_t(gm)), _dev(np.stack([mean.real, mean.imag], -1)),
                    _close_pred(0.0, MOMENTS_BAR * max(1.0, float(np.abs(mean).max()))))
    bv = _bad_items(_t(gv)[:, None], _dev(var[:, None]), _close_pred(0.0, MOMENTS_BAR * max(1.0, float(np.abs(var).max()))))
    return bm | bv


def test_symbol_logits2moments_one_period(phy):
    assert not bool(_moments_check(phy, P).any())


@pytest.mark.parametrize("size", SIZES)
def test_symbol_logits2moments_past_one_trip(phy, size):
    n = elements("logits2moments", size)
    _report(_moments_check(phy, n), stride_items("logits2moments"), f"SymbolLogits2Moments {size}")


@pytest.mark.parametrize("size", SIZES)
def test_pam2qam_logits_past_one_trip(phy, size):
    """pam2qam_logits_kernel: a thread per output element, 16 per row at m = 4, so rows = work items / 16 rounded up (the
    second trip of N1 holds the 16 elements of one row, not one).  One float32 add per entry: bit for bit against the oracle
    like test_gpu_symbol.py::test_moments_and_pam_qam."""
    m, q = 4, 16
    rows = -(-work_items("pam2qam", size) // q)
    assert rows * q > threshold("pam2qam")
    rng = np.random.default_rng(m)
    a = (rng.normal(size=(P, 4)) * 2).astype(np.float32)
    b = (rng.normal(size=(P, 4)) * 2).astype(np.float32)
    ref = omap.pam2qam(a, b, m, hard_in_out=False)
    assert ref.dtype == np.float32
    got = _t(phy.mapping.PAM2QAM(m, hard_in_out=False)(_tile(a, rows), _tile(b, rows)))
    assert got.shape == (rows, q)
    assert (threshold("pam2qam") // q) % P != 0
    _report(_bad_items(got, _dev(ref), _exact_pred), threshold("pam2qam") // q, f"PAM2QAM logits {size}")


# ===================================================================================================== channel.hip
@pytest.mark.parametrize("size", SIZES)
def test_binary_source_past_one_trip(phy, size):
    """binary_source_kernel against oracle.utils.random_bits over the whole length, bit-exact like
    test_gpu_parity.py::test_binary_source_bit_exact; n is no multiple of 4 (element-wise stores of the last block)."""
    n = elements("binary_source", size, rest=3)
    assert (n + 3) // 4 > threshold("binary_source") and n % 4
    phy.config.seed = 2024
    got = _np(phy.mapping.BinarySource()([n]))
    ref = outil.random_bits(2024, 0, n)
    bad = torch.from_numpy(got != ref)
    _report(bad, stride_items("binary_source"), f"BinarySource {size}")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("per_element_no", [False, True])
def test_awgn_past_one_trip(phy, per_element_no, size):
    """awgn_kernel against oracle.utils.awgn over the whole (odd) length; signal, noise variances and bar (rtol 1e-5, atol 2e-6) of
    test_gpu_parity.py::test_awgn_matches_stream_spec."""
    n = elements("awgn", size)
    assert (n + 1) // 2 > threshold("awgn") and n % 2
    phy.config.seed = 77
    i = np.arange(n)
    x = (i % 7 - 3 + 1j * (i % 5 - 2)).astype(np.complex64)
    no = np.linspace(0.01, 2, n).astype(np.float32) if per_element_no else 0.37
    got = _np(phy.channel.AWGN()(x, no))
    ref = outil.awgn(x, no, 77, 0)
    bad = torch.from_numpy(~np.isclose(got, ref, rtol=1e-5, atol=2e-6))
    _report(bad, stride_items("awgn"), f"AWGN per_element_no={per_element_no} {size}")


def test_binary_source_misaligned_output(phy):
    """The element-wise store path of binary_source_kernel: ``out`` 4 bytes past a 16-byte boundary (torch allocations never
    are), n no multiple of 4.  The window holds the oracle's stream; its neighbours in the buffer stay untouched."""
    from sionna_amd import _ffi
    n = 4 * 1000 + 3
    buf = torch.full((n + 8,), -7.0, dtype=torch.float32, device=_ffi.device())
    out = buf[1:]
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    _ffi.check(_ffi.lib().samd_binary_source_f32(99, 3, n, ctypes.c_void_p(out.data_ptr()), _ffi.stream()), "BinarySource")
    torch.cuda.synchronize()
    got = _np(buf)
    assert np.array_equal(got[1:1 + n], outil.random_bits(99, 3, n))
    assert got[0] == -7.0 and np.all(got[1 + n:] == -7.0)


# ===================================================================================================== ofdm.hip
def _rg_pair(phy, precision=None):
    kw = dict(num_tx=2, num_streams_per_tx=1, cyclic_prefix_length=6, num_guard_carriers=[5, 6], dc_null=True,
              pilot_pattern="kronecker", pilot_ofdm_symbol_indices=[2, 11])
    if precision == "double":
        rg = phy.ofdm.ResourceGrid(14, 76, 15e3, precision="double", **kw)
        org = o.ResourceGrid(14, 76, 15e3, **kw)
        opp = org.pilot_pattern

        class _Pilots64:                               # the oracle sees the block's own float64 pilots (test_gpu_double.py::_grids64)
            mask, num_pilot_symbols, num_data_symbols = opp.mask, opp.num_pilot_symbols, opp.num_data_symbols
            pilots = np.asarray(rg.pilot_pattern.pilots)
        org.pilot_pattern = _Pilots64
        return rg, org
    return phy.ofdm.ResourceGrid(14, 76, 15e3, **kw), o.ResourceGrid(14, 76, 15e3, **kw)


PB = 13                                    # distinct batch items of the batch-periodic OFDM inputs (prime)


def _batch_for(name, size, per_batch):
    """Smallest batch whose work items reach work_items(name, size): a batch item is ``per_batch`` work items."""
    b = -(-work_items(name, size) // per_batch)
    assert b * per_batch > threshold(name)
    assert (threshold(name) % (PB * per_batch)) != 0                  # a read from the wrong trip lands on another value
    return b


def _cplx(rng, shape, dtype=np.complex64):
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)


def _check_batch_periodic(got, ref, pred, name, per_batch, what):
    got = _t(got)
    if got.is_complex():
        got, ref = torch.view_as_real(got), np.stack([ref.real, ref.imag], -1)
    bad = _bad_items(got, _dev(ref), pred)                             # per batch item
    _report(bad, max(1, threshold(name) // per_batch), what + " (items = batch entries)")


@pytest.mark.parametrize("size", SIZES)
def test_resource_grid_mapper_demapper_past_one_trip(phy, size):
    """rg_map_kernel and gather3_kernel<2> (ResourceGridDemapper): bit-exact like test_gpu_ofdm.py::test_rg_mapper_demapper_roundtrip
    (the mapper against oracle.ofdm.rg_map, the demapper returning the data symbols)."""
    rg, org = _rg_pair(phy)
    sm = phy.mimo.StreamManagement([[1, 0], [0, 1]], 1)
    rng = np.random.default_rng(0)
    x = _cplx(rng, (PB, 2, 1, rg.num_data_symbols))
    ref = o.rg_map(org, x)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("rg_map", size, per_batch)
    xd = _tile(x, b)
    grid = phy.ofdm.ResourceGridMapper(rg)(xd)
    assert tuple(grid.shape) == (b,) + ref.shape[1:]
    _check_batch_periodic(grid, ref, _exact_pred, "rg_map", per_batch, f"ResourceGridMapper {size}")
    # the demapper gathers num_data_symbols elements per stream: its own batch size
    per_batch_d = int(np.prod(x.shape[1:]))
    bd = _batch_for("gather3", size, per_batch_d)
    gridd = phy.ofdm.ResourceGridMapper(rg)(_tile(x, bd))
    back = phy.ofdm.ResourceGridDemapper(rg, sm)(gridd)
    assert tuple(back.shape) == (bd,) + x.shape[1:]
    _check_batch_periodic(back, x, _exact_pred, "gather3", per_batch_d, f"ResourceGridDemapper {size}")


@pytest.mark.parametrize("size", SIZES)
def test_apply_ofdm_channel_past_one_trip(phy, size):
    """apply_ofdm_channel_kernel: bar of test_gpu_ofdm.py::test_cir_to_ofdm_and_apply_channel (rtol 1e-4, atol 1e-5); unit-variance
    x and h like there (h_freq normalised to unit energy)."""
    rng = np.random.default_rng(1)
    x = _cplx(rng, (PB, 1, 2, 14, 76))
    h = (_cplx(rng, (PB, 1, 4, 1, 2, 14, 76)) / np.sqrt(2)).astype(np.complex64)
    ref = o.apply_ofdm_channel(x, h)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("apply_ofdm", size, per_batch)
    y = phy.channel.ApplyOFDMChannel()(_tile(x, b), _tile(h, b))
    assert tuple(y.shape) == (b,) + ref.shape[1:]
    _check_batch_periodic(y, ref, _close_pred(1e-4, 1e-5), "apply_ofdm", per_batch, f"ApplyOFDMChannel {size}")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("interp", ["nn", None])
def test_ls_estimator_past_one_trip(phy, interp, size):
    """ls_gather_scale_kernel (LS estimate at the pilots, and with the nearest-neighbour spreading over the grid): bar of
    test_gpu_ofdm.py::test_ls_estimator_matches_oracle, rtol 1e-5, atol 1e-6."""
    rg, org = _rg_pair(phy)
    rng = np.random.default_rng(2)
    y = _cplx(rng, (PB, 1, 4, 14, 76))
    ref, _ = o.ls_estimate(org, y, 0.07, interp)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("ls_gather_scale", size, per_batch)
    h_hat, _ = phy.ofdm.LSChannelEstimator(rg, interpolation_type=interp, defer=False)(_tile(y, b), 0.07)
    assert tuple(h_hat.shape) == (b,) + ref.shape[1:]
    _check_batch_periodic(h_hat, ref, _close_pred(1e-5, 1e-6), "ls_gather_scale", per_batch, f"LSChannelEstimator {interp} {size}")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("time_avg", [False, True])
def test_linear_interpolator_past_one_trip(phy, time_avg, size):
    """lin_interp_kernel<float2> through LSChannelEstimator("lin" / "lin_time_avg"): bar of
    test_gpu_ofdm.py::test_ls_estimator_linear_vs_oracle, rtol 1e-4, atol 1e-5."""
    rg, org = _rg_pair(phy)
    rng = np.random.default_rng(7)
    y = _cplx(rng, (PB, 1, 4, 14, 76))
    ref, _ = o.ls_estimate_lin(org, y, 0.05, time_avg=time_avg)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("lin_interp", size, per_batch)
    h, _ = phy.ofdm.LSChannelEstimator(rg, interpolation_type="lin_time_avg" if time_avg else "lin")(_tile(y, b), 0.05)
    assert tuple(h.shape) == (b,) + ref.shape[1:]
    _check_batch_periodic(h, ref, _close_pred(1e-4, 1e-5), "lin_interp", per_batch, f"LinearInterpolator time_avg={time_avg} {size}")


# ===================================================================================================== float64 twins (N1)
def _close9():
    return _close_pred(1e-9, 1e-9)                                     # test_gpu_double.py::_close9


def test_demapper_double_past_one_trip(phy):
    """demap64_kernel (f64.hip:723): draw and bars of test_gpu_double.py::test_demapper_double_vs_oracle - rtol 1e-11, atol 1e-10
    without prior (per-symbol no), rtol 1e-10, atol 1e-9 with a per-symbol prior."""
    m = 4
    n = elements("qam_demap_f64", "N1")
    rng = np.random.default_rng(m)
    pts = omap.qam(m, dtype=np.complex128)
    y = pts[rng.integers(0, 2 ** m, P)] + (rng.normal(size=P) + 1j * rng.normal(size=P)) * 0.3
    no = rng.uniform(0.01, 100, size=P)
    prior = rng.normal(size=(P, m)) * 2
    dm = phy.mapping.Demapper("app", "qam", m, precision="double")
    ref = omap.demapper(y, no, pts, "app").reshape(P, m)
    got = dm(_tile(y, n), _tile(no, n))
    assert got.dtype == torch.float64
    _check_periodic(_t(got).reshape(n, m), ref, _close_pred(1e-11, 1e-10), "qam_demap_f64", "Demapper double")
    ref = omap.demapper(y, np.float64(0.3), pts, "app", prior=prior).reshape(P, m)
    got = dm(_tile(y, n), 0.3, _tile(prior, n))
    _check_periodic(_t(got).reshape(n, m), ref, _close_pred(1e-10, 1e-9), "qam_demap_f64", "Demapper double with prior")


def test_symbol_blocks_double_past_one_trip(phy):
    """f64_mapping.hip, one case per kernel, draws and bar (_close9; PAM2QAM and hard decisions exact) of
    test_gpu_double.py::test_symbol_blocks_double."""
    m = 2
    rng = np.random.default_rng(m)
    pts = omap.qam(m, dtype=np.complex128)
    n = elements("symbol_demap_f64", "N1")
    y = (rng.normal(size=P) + 1j * rng.normal(size=P)) * 0.7
    no, prior = rng.uniform(0.1, 1.0, size=P), rng.normal(size=(P, 1 << m))
    got = phy.mapping.SymbolDemapper("qam", m, precision="double")(_tile(y, n), _tile(no, n), _tile(prior, n))
    assert got.dtype == torch.float64
    _check_periodic(got, omap.symbol_demapper(y, no, pts, prior), _close9(), "symbol_demap_f64", "SymbolDemapper double")
    m = 4
    pts = omap.qam(m, dtype=np.complex128)
    logits = rng.normal(size=(P, 1 << m)) * 3
    pr = rng.normal(size=(P, m))
    n = elements("logits2llrs_f64", "N1")
    zd = _tile(logits, n)
    got = phy.mapping.SymbolLogits2LLRs("app", m, precision="double")(zd, _tile(pr, n))
    _check_periodic(got, omap.symbol_logits2llrs(logits, m, "app", pr), _close9(), "logits2llrs_f64", "SymbolLogits2LLRs double")
    n = elements("logits2moments_f64", "N1")
    mean, var = phy.mapping.SymbolLogits2Moments("qam", m, precision="double")(zd[:n])
    rm, rv = omap.symbol_logits2moments(logits, pts)
    _check_periodic(torch.view_as_real(_t(mean)), np.stack([rm.real, rm.imag], -1), _close9(), "logits2moments_f64", "Moments double mean")
    _check_periodic(_t(var)[:, None], rv[:, None], _close9(), "logits2moments_f64", "Moments double var")
    del zd, got, mean, var
    llrs = rng.normal(size=(P, m)) * 4
    n = elements("llrs2logits_f64", "N1")
    got = phy.mapping.LLRs2SymbolLogits(m, precision="double")(_tile(llrs, n))
    _check_periodic(got, omap.llrs2symbol_logits(llrs, m), _close9(), "llrs2logits_f64", "LLRs2SymbolLogits double")
    del got
    q = 16
    rows = -(-work_items("pam2qam_f64", "N1") // q)
    assert rows * q > threshold("pam2qam_f64") and (threshold("pam2qam_f64") // q) % P != 0
    p1, p2 = rng.normal(size=(P, 4)), rng.normal(size=(P, 4))
    got = _t(phy.mapping.PAM2QAM(m, hard_in_out=False, precision="double")(_tile(p1, rows), _tile(p2, rows)))
    assert got.dtype == torch.float64
    _report(_bad_items(got, _dev(omap.pam2qam(p1, p2, m, hard_in_out=False)), _exact_pred), threshold("pam2qam_f64") // q, "PAM2QAM double")


def test_awgn_double_past_one_trip(phy):
    """awgn128_kernel against oracle.f64_ofdm.awgn over the whole length, per-element no: _close9 like
    test_gpu_double.py::test_complex_normal_awgn_double."""
    n = elements("awgn_f64", "N1")
    rng = np.random.default_rng(0)
    x = _cplx(rng, (n,), np.complex128)
    no = rng.uniform(0.1, 2.0, size=n)
    phy.config.seed = 9
    y = _np(phy.channel.AWGN(precision="double")(x, no))
    ref = o64.awgn(x, no, 9, 0)
    assert y.dtype == np.complex128
    _report(torch.from_numpy(~np.isclose(y, ref, rtol=1e-9, atol=1e-9)), stride_items("awgn_f64"), "AWGN double")


def test_ofdm_blocks_double_past_one_trip(phy):
    """rg_map128_kernel (exact, test_gpu_double.py::test_resource_grid_blocks_double), apply_ofdm_channel128_kernel
    (test_tdl_ofdm_channel_double), ls_gather_scale128_kernel and lin_interp_kernel<double2> (test_ls_estimator_double): _close9."""
    rg, org = _rg_pair(phy, "double")
    rng = np.random.default_rng(1)
    x = _cplx(rng, (PB, 2, 1, rg.num_data_symbols), np.complex128)
    ref = o64.rg_map(org, x)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("rg_map_f64", "N1", per_batch)
    grid = phy.ofdm.ResourceGridMapper(rg, precision="double")(_tile(x, b))
    assert grid.dtype == torch.complex128
    _check_batch_periodic(grid, ref, _exact_pred, "rg_map_f64", per_batch, "ResourceGridMapper double")
    del grid
    xs = _cplx(rng, (PB, 1, 2, 14, 76), np.complex128)
    h = _cplx(rng, (PB, 1, 4, 1, 2, 14, 76), np.complex128)
    ref = o64.apply_ofdm_channel(xs, h)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("apply_ofdm_f64", "N1", per_batch)
    y = phy.channel.ApplyOFDMChannel(precision="double")(_tile(xs, b), _tile(h, b))
    _check_batch_periodic(y, ref, _close9(), "apply_ofdm_f64", per_batch, "ApplyOFDMChannel double")
    del y
    yy = _cplx(rng, (PB, 1, 4, 14, 76), np.complex128)
    ref, _ = o64.ls_estimate(org, yy, 0.1)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("ls_gather_scale_f64", "N1", per_batch)
    h_hat, _ = phy.ofdm.LSChannelEstimator(rg, interpolation_type="nn", precision="double")(_tile(yy, b), 0.1)
    assert h_hat.dtype == torch.complex128
    _check_batch_periodic(h_hat, ref, _close9(), "ls_gather_scale_f64", per_batch, "LSChannelEstimator double")
    del h_hat
    ref, _ = o64.ls_estimate_lin(org, yy, 0.1, False)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("lin_interp_f64", "N1", per_batch)
    h_lin, _ = phy.ofdm.LSChannelEstimator(rg, interpolation_type="lin", precision="double")(_tile(yy, b), 0.1)
    _check_batch_periodic(h_lin, ref, _close9(), "lin_interp_f64", per_batch, "LinearInterpolator double")


def test_tdl_cir_double_past_one_trip(phy):
    """tdl_cir128_kernel draws from Philox counters indexed by (b, p, n) / (b, ra, ta, p, n): position dependent, so the whole
    batch against oracle.f64_ofdm.tdl_cir; model (LOS "D", so the p == 0 branch runs too), speeds, antennas, sampling frequency and bar
    (_close9) of test_gpu_double.py::test_tdl_ofdm_channel_double.  Largest host temporary of the oracle: 2.1 M x 20 complex128 = 0.7 GB."""
    ra, ta, T = 4, 2, 14
    tdl = phy.channel.tr38901.TDL("D", 300e-9, 2.6e9, min_speed=3., max_speed=30., num_rx_ant=ra, num_tx_ant=ta, precision="double")
    per_batch = ra * ta * tdl.num_clusters * T
    b = -(-work_items("tdl_cir_f64", "N1") // per_batch)
    assert b * per_batch > threshold("tdl_cir_f64")
    fs = 1 / 71.4e-6
    phy.config.seed = 11
    a, tau = tdl(b, T, fs)
    assert a.dtype == torch.complex128 and tuple(a.shape) == (b, 1, ra, 1, ta, tdl.num_clusters, T)
    ref_a, ref_tau = o64.tdl_cir(11, 0, b, T, fs, tdl.delays, tdl._mean_powers, tdl._min_doppler, tdl._max_doppler, ra, ta, 20,
                                 los_power=tdl._los_power if tdl.los else None)
    got = _np(a)
    bad = ~np.isclose(got, ref_a, rtol=1e-9, atol=1e-9).reshape(-1)
    _report(torch.from_numpy(bad), stride_items("tdl_cir_f64"), "TDL double")
    assert np.allclose(_np(tau), ref_tau, rtol=1e-9, atol=1e-9)


def test_cir_to_ofdm_double_past_one_trip(phy):
    """cir_to_ofdm128_kernel (and c2o_normalize128_kernel behind it, one workgroup per (b, rx, tx)) on batch-periodic TDL taps:
    draws and bar (_close9) of test_gpu_double.py::test_tdl_ofdm_channel_double."""
    tdl = phy.channel.tr38901.TDL("A", 300e-9, 2.6e9, min_speed=3., max_speed=30., num_rx_ant=4, num_tx_ant=2, precision="double")
    a, tau = o64.tdl_cir(11, 0, PB, 14, 1 / 71.4e-6, tdl.delays, tdl._mean_powers, tdl._min_doppler, tdl._max_doppler, 4, 2, 20)
    fr = phy.channel.subcarrier_frequencies(76, 15e3, precision="double")
    for norm in (False, True):
        ref = o64.cir_to_ofdm_channel(fr, a, tau, normalize=norm)
        per_batch = int(np.prod(ref.shape[1:]))
        b = _batch_for("cir_to_ofdm_f64", "N1", per_batch)
        h = phy.channel.cir_to_ofdm_channel(fr, _tile(a, b), _tile(tau, b), normalize=norm)
        assert h.dtype == torch.complex128 and tuple(h.shape) == (b,) + ref.shape[1:]
        _check_batch_periodic(h, ref, _close9(), "cir_to_ofdm_f64", per_batch, f"cir_to_ofdm_channel double normalize={norm}")


def test_time_channel_double_past_one_trip(phy):
    """cir_to_time128_kernel (with and without time_normalize128_kernel) and apply_time128_kernel on batch-periodic inputs: draws and
    bar (_close9) of test_gpu_double.py::test_time_channel_double.  apply_time writes only rx_ant x (tn + L - 1) samples per batch
    item, so its case keeps one transmitter with two antennas, four taps and 250 samples: h is 4145 x 2 x 2 x 253 x 4 complex128 =
    268 MB, the largest tensor of the float64 cases."""
    rng = np.random.default_rng(12)
    rx, ra, tx, ta, npath, tn, l_min, l_max = 1, 2, 2, 2, 5, 40, -3, 7
    L = l_max - l_min + 1
    a = _cplx(rng, (PB, rx, ra, tx, ta, npath, tn + L - 1), np.complex128) * 0.5
    tau = rng.uniform(0, 3e-7, size=(PB, rx, tx, npath))
    W = 15.36e6
    for norm in (False, True):
        ref = o64.cir_to_time_channel(W, a, tau, l_min, l_max, norm)
        per_batch = int(np.prod(ref.shape[1:]))
        b = _batch_for("cir_to_time_f64", "N1", per_batch)
        h = phy.channel.cir_to_time_channel(W, _tile(a, b), _tile(tau, b), l_min, l_max, normalize=norm)
        assert h.dtype == torch.complex128 and tuple(h.shape) == (b,) + ref.shape[1:]
        _check_batch_periodic(h, ref, _close9(), "cir_to_time_f64", per_batch, f"cir_to_time_channel double normalize={norm}")
    del h
    tx, tn, l_min, l_max = 1, 250, -1, 2
    L = l_max - l_min + 1
    a = _cplx(rng, (PB, rx, ra, tx, ta, npath, tn + L - 1), np.complex128) * 0.5
    tau = rng.uniform(0, 3e-7, size=(PB, rx, tx, npath))
    h = o64.cir_to_time_channel(W, a, tau, l_min, l_max, True)
    x = _cplx(rng, (PB, tx, ta, tn), np.complex128)
    ref = o64.apply_time_channel(x, h)
    per_batch = int(np.prod(ref.shape[1:]))
    b = _batch_for("apply_time_f64", "N1", per_batch)
    y = phy.channel.ApplyTimeChannel(tn, L, precision="double")(_tile(x, b), _tile(h, b))
    assert y.dtype == torch.complex128 and tuple(y.shape) == (b,) + ref.shape[1:]
    _check_batch_periodic(y, ref, _close9(), "apply_time_f64", per_batch, "ApplyTimeChannel double")


# ===================================================================================================== metrics.hip
@pytest.mark.parametrize("soft", [False, True])
def test_count_errors_across_trips(phy, soft):
    """count_errors_kernel accumulates over the blocks a wave visits: 2 * 16384 + 5 blocks of 67 bits are three trips.  Flips
    are placed so that every trip has clean and erroneous blocks; both counters equal NumPy's, exactly
    (test_gpu_parity.py::test_count_errors).  soft: b_hat are LLRs, decided by > 0 inside the kernel."""
    nb, bl = 2 * 16384 + 5, 67
    t = threshold("count_errors")
    assert nb > 2 * t
    rng = np.random.default_rng(0)
    b = rng.integers(0, 2, (nb, bl)).astype(np.float32)
    flip = rng.random(b.shape) < 0.004                     # ~ 24 % of the blocks carry an error
    flip[::3] = False                                      # a third of the blocks of every trip is clean for sure
    flip[t + 1, 5] = flip[2 * t + 4, 66] = True            # a block at the start of trip 2 and the last block of trip 3
    bh = np.where(flip, 1 - b, b)
    for trip in range(3):
        rows = flip[trip * t:(trip + 1) * t].any(1)
        assert rows.any() and not rows.all()
    if soft:
        bh = ((2 * bh - 1) * rng.uniform(0.1, 9, b.shape)).astype(np.float32)
        bh[7, :5] = 0.0                                    # an LLR of zero decides 0 (strict > 0)
        hard = (bh > 0).astype(np.float32)
    else:
        hard = bh
    from sionna_amd import _ffi
    bd, bhd = _dev(b), _dev(bh.astype(np.float32))
    if soft:
        counters = torch.zeros(2, dtype=torch.int64, device=bd.device)
        _ffi.check(_ffi.lib().samd_count_errors_f32(_ffi.ptr(bd), _ffi.ptr(bhd), nb, bl, 1, _ffi.ptr(counters), _ffi.stream()), "count_errors")
        bits, blocks = (int(v) for v in _np(counters))
    else:
        bits, blocks = int(phy.utils.count_errors(bd, bhd)), int(phy.utils.count_block_errors(bd, bhd))
    assert bits == outil.count_errors(b, hard) and blocks == outil.count_block_errors(b, hard), (bits, blocks)


# ===================================================================================================== CRC (polar.hip)
def test_crc_across_trips(phy):
    """crc_kernel: 2 * 8192 + 3 words of k = 100 are three trips of its wave-per-word loop; encode against
    oracle.polar.crc_encode bit for bit (test_gpu_polar.py::test_crc_golden_and_oracle), check mode with a known subset of
    corrupted words in every trip."""
    nw, k = 2 * 8192 + 3, 100
    t = threshold("crc")
    assert nw > 2 * t
    bits = np.random.default_rng(1).integers(0, 2, (nw, k)).astype(np.float32)
    enc = phy.fec.crc.CRCEncoder("CRC24A")
    dec = phy.fec.crc.CRCDecoder(enc)
    x = _np(enc(bits))
    ref = op.crc_encode(bits, "CRC24A")
    bad = torch.from_numpy((x != ref).any(1))
    _report(bad, t, "CRCEncoder")
    corrupt = np.zeros(nw, bool)
    corrupt[[0, 5, t - 1, t, t + 1, t + 77, 2 * t - 1, 2 * t, 2 * t + 2]] = True
    corrupt[::11] = True
    xb = ref.copy()
    xb[corrupt, 17] = 1 - xb[corrupt, 17]
    info, valid = dec(xb)
    assert np.array_equal(_np(info), xb[:, :k])
    _report(torch.from_numpy(_np(valid)[:, 0] != ~corrupt), t, "CRCDecoder")
    assert np.array_equal(_np(valid), op.crc_check(xb, "CRC24A")[1])


@pytest.mark.parametrize("k", [20011, 32768 - 24, 32768, 32769 - 24, 32769])
def test_crc_table_sizes_and_kernel_switch(phy, k):
    """samd_crc_f32 (polar.hip:461-469) keeps its table of k words in LDS up to 128 KB and walks longer words serially:
      * k = 20011: an 80 KB table (above the 64 KB a kernel gets without the raised limit), in encode and in check mode
        (k + 24 bits = 80.1 KB);
      * check mode at 32768 bits (info 32744), the last length on crc_kernel, and at 32769 bits (info 32745), the first on
        crc_serial_kernel;
      * encode at k = 32768 (crc_kernel; its check at 32792 bits runs crc_serial_kernel) and at k = 32769 (crc_serial_kernel).
    Each of a handful of words against oracle.polar.crc_encode / crc_check, bit for bit."""
    bits = np.random.default_rng(k).integers(0, 2, (5, k)).astype(np.float32)
    enc = phy.fec.crc.CRCEncoder("CRC24A")
    dec = phy.fec.crc.CRCDecoder(enc)
    ref = op.crc_encode(bits, "CRC24A")
    assert np.array_equal(_np(enc(bits)), ref)
    xb = ref.copy()
    xb[1, 0] = 1 - xb[1, 0]
    xb[3, k + 23] = 1 - xb[3, k + 23]
    xb[4, k // 2] = 1 - xb[4, k // 2]
    info, valid = dec(xb)
    assert np.array_equal(_np(info), xb[:, :k])
    assert np.array_equal(_np(valid)[:, 0], [True, False, True, False, False])
    assert np.array_equal(_np(valid), op.crc_check(xb, "CRC24A")[1])
