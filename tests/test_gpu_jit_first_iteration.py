"""The generated min-sum kernel with its peeled, lean first iteration on the GPU (CPU twin: tests/test_jit_emu_first_iteration.py).

C2's code at the smallest batch the generated kernel takes by default (256) and at 300 (a batch tail within one grid trip); two
iterations (the lean first trip and the lean last one), three (one loop trip between them) and twenty; min-sum and
offset-min-sum, both output forms, soft outputs and hard decisions: array_equal to the generic on-chip kernel (SAMD_LDPC_JIT=0)
on every row and to oracle/ldpc_bp.c on 64 of them; the generated kernel is the one that ran.  (One iteration - the path
without a first trip - is tests/test_gpu_jit_rotations.py.)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.ldpc5g import LDPC5GCode
from oracle import ldpc_bp as obp, cbind

K, N, BG, M = 2816, 8448, "bg1", 6
ORACLE_ROWS = 64
OFFSET = 0.5
ITERS = (2, 3, 20)
RULES = ("minsum", "offset-minsum")


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
    """300 noisy codewords; row 0: first 7 values 0, row 1: rounded (exact ties), row 2: every fifth value x 40 (the clip), row 3:
    all zero (every message +-0), row 4: -0.0 inputs and magnitudes below the offset; rows 0 .. 255 are the batch of 256"""
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
    llr[3] = 0
    llr[4, ::3] = np.sign(llr[4, ::3]) * np.float32(0.25)
    llr[4, 1::7] = np.float32(-0.0)
    return code, llr


@pytest.fixture(scope="module")
def oracle_soft(llr300):
    """soft outputs of the C oracle on the first 64 rows, per (rule, iterations, output form): computed once"""
    code, llr = llr300
    out = {}
    for rule in RULES:
        for it in ITERS:
            odec = obp.LDPC5GDecoder(code, cn_update=rule, hard_out=False, return_infobits=True, num_iter=it)
            xr = cbind.bp_decode(odec, odec.rate_recover(llr[:ORACLE_ROWS]), num_iter=it, hard_out=0, offset=OFFSET)
            out[rule, it, True] = xr[:, :code.k]
            x_nf = np.concatenate([xr[:, :code.k], xr[:, code.k_ldpc:]], axis=1)      # decoding.py:1506-1531
            out[rule, it, False] = x_nf[:, 2 * code.z:2 * code.z + code.n][:, code.out_int]
    return out


@pytest.mark.parametrize("batch", [256, 300])
@pytest.mark.parametrize("it", ITERS)
@pytest.mark.parametrize("rule", RULES)
def test_lean_first_iteration_bit_exact(phy, llr300, oracle_soft, rule, it, batch):
    _, llr_all = llr300
    llr = torch.from_numpy(llr_all[:batch]).cuda()
    enc = phy.fec.ldpc.LDPC5GEncoder(K, N, num_bits_per_symbol=M, bg=BG)
    with _opt("SAMD_LDPC_JIT", "0"):
        enc0 = phy.fec.ldpc.LDPC5GEncoder(K, N, num_bits_per_symbol=M, bg=BG)
    for infobits in (True, False):
        for hard in (False, True):
            dec = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update=rule, hard_out=hard, return_infobits=infobits, num_iter=it)
            before = _launches(enc, dec)
            got = _np(dec(llr))
            assert _launches(enc, dec) == before + 1, "the generated kernel did not run"
            with _opt("SAMD_LDPC_JIT", "0"):
                dec0 = phy.fec.ldpc.LDPC5GDecoder(enc0, cn_update=rule, hard_out=hard, return_infobits=infobits, num_iter=it)
                generic = _np(dec0(llr))
                assert _launches(enc0, dec0) == 0
            assert np.array_equal(got, generic), (infobits, hard, float(np.mean(got != generic)))
            ref = oracle_soft[rule, it, infobits]
            ref = (ref >= 0).astype(np.float32) if hard else ref
            assert np.array_equal(got[:ORACLE_ROWS], ref), (infobits, hard, float(np.mean(got[:ORACLE_ROWS] != ref)))
