"""The generated min-sum kernel with its peeled, lean last iteration on the GPU (CPU twin: tests/test_jit_emu_rotations.py).

C2's code at the smallest batch the generated kernel takes by default (256) and at 300 (a batch tail within one grid trip), one
iteration (the peeled trip alone) and twenty, both output forms, soft outputs and hard decisions: array_equal to the generic
on-chip kernel (SAMD_LDPC_JIT=0) on every row and to oracle/ldpc_bp.c on 64 of them; the generated kernel is the one that ran.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.ldpc5g import LDPC5GCode
from oracle import ldpc_bp as obp, cbind

K, N, BG, M = 2816, 8448, "bg1", 6
ORACLE_ROWS = 64


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _opt(key, value="1"):
    from sionna_amd import _ffi
    return _ffi.option(key, value)


def _launches(enc, dec):
    from sionna_amd import _ffi
    return int(_ffi.lib().samd_ldpc5g_jit_launches(enc._handle(dec._nb_pruned_nodes)))


@pytest.fixture(scope="module")
def llr300():
    """300 noisy codewords with zeros, exact ties and values beyond the clip; rows 0 .. 255 are the batch of 256"""
    code = LDPC5GCode(K, N, M, BG)
    rng = np.random.default_rng(K + N)
    u = rng.integers(0, 2, (300, K)).astype(np.float32)
    c = code.encode(u)
    sigma = 0.8
    y = (2 * c - 1) + sigma * rng.normal(size=c.shape)
    llr = (2 * y / sigma ** 2).astype(np.float32)
    llr[0, :7] = 0
    llr[1] = np.round(llr[1])
    llr[2, ::5] *= 40
    return code, llr


@pytest.fixture(scope="module")
def oracle_soft(llr300):
    """soft outputs of the C oracle on the first 64 rows, per (iterations, output form): computed once"""
    code, llr = llr300
    out = {}
    for it in (1, 20):
        odec = obp.LDPC5GDecoder(code, cn_update="minsum", hard_out=False, return_infobits=True, num_iter=it)
        xr = cbind.bp_decode(odec, odec.rate_recover(llr[:ORACLE_ROWS]), num_iter=it, hard_out=0)
        out[it, True] = xr[:, :code.k]
        x_nf = np.concatenate([xr[:, :code.k], xr[:, code.k_ldpc:]], axis=1)      # decoding.py:1506-1531
        out[it, False] = x_nf[:, 2 * code.z:2 * code.z + code.n][:, code.out_int]
    return out


@pytest.mark.parametrize("batch", [256, 300])
@pytest.mark.parametrize("it", [1, 20])
def test_lean_last_iteration_bit_exact(phy, llr300, oracle_soft, batch, it):
    _, llr_all = llr300
    llr = torch.from_numpy(llr_all[:batch]).cuda()
    enc = phy.fec.ldpc.LDPC5GEncoder(K, N, num_bits_per_symbol=M, bg=BG)
    for infobits in (True, False):
        for hard in (False, True):
            dec = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", hard_out=hard, return_infobits=infobits, num_iter=it)
            before = _launches(enc, dec)
            got = _np(dec(llr))
            assert _launches(enc, dec) == before + 1, "the generated kernel did not run"
            with _opt("SAMD_LDPC_JIT", "0"):
                enc0 = phy.fec.ldpc.LDPC5GEncoder(K, N, num_bits_per_symbol=M, bg=BG)
                dec0 = phy.fec.ldpc.LDPC5GDecoder(enc0, cn_update="minsum", hard_out=hard, return_infobits=infobits, num_iter=it)
                generic = _np(dec0(llr))
                assert _launches(enc0, dec0) == 0
            assert np.array_equal(got, generic), (infobits, hard, float(np.mean(got != generic)))
            ref = oracle_soft[it, infobits]
            ref = (ref >= 0).astype(np.float32) if hard else ref
            assert np.array_equal(got[:ORACLE_ROWS], ref), (infobits, hard, float(np.mean(got[:ORACLE_ROWS] != ref)))


def test_return_state_two_calls_of_three_equal_one_of_six(phy, llr300):
    """the state variant keeps the whole last iteration: its image is those v2c"""
    _, llr_all = llr300
    llr = torch.from_numpy(llr_all[:256]).cuda()
    T = lambda x: x.as_subclass(torch.Tensor)
    enc = phy.fec.ldpc.LDPC5GEncoder(K, N, num_bits_per_symbol=M, bg=BG)
    mk = lambda n_it, st: phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", hard_out=False, num_iter=n_it, return_state=st)
    d3 = mk(3, True)
    _, s1 = d3(llr)
    assert d3._state_lay[1] is not None, "the generated kernel with state did not run"
    x2, s2 = d3(llr, msg_v2c=s1)
    x6, s6 = mk(6, True)(llr)
    assert torch.equal(T(x2), T(x6)) and torch.equal(T(s2), T(s6))
    d6 = mk(6, False)
    before = _launches(enc, d6)
    assert torch.equal(T(d6(llr)), T(x6))                     # the lean kernel: same outputs
    assert _launches(enc, d6) == before + 1
