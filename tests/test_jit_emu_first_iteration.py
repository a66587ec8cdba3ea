"""The generated min-sum programs with the FIRST iteration peeled and lean, held to the oracle without a GPU.

The channel value of a punctured column is +0 on every lane, so the first check-node update of a row that touches such a column
sends +-0 on every edge but the one to that column, and a variable node that adds +-0 returns its channel value - what init()
stored.  The generator (csrc/ldpc5g_jit_gen.cpp, Class1Emitter::lean_first) therefore emits, for the min-sum / offset-min-sum
programs of the Z = 128 k class without state and at least two iterations, a first trip of one message per row with exactly one
punctured column (jit_cn_first) and the update of the punctured columns over those messages (jit_vnb_first / jit_vn_first);
init() stores nothing for the punctured columns, whose slots then still hold the previous codeword's messages.

Same emulation as tests/test_jit_emu_rotations.py: the generated text compiled with g++ against the 64-wide stand-ins of
tests/jit_emu (its trap on a -0 where none may be stays active), soft outputs and hard decisions array_equal to
oracle/ldpc_bp.c.  (`-m gpu` twin: tests/test_gpu_jit_first_iteration.py.)
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ldpc5g import LDPC5GCode          # noqa: E402
from oracle import ldpc_bp as obp, cbind      # noqa: E402
from tools import jit_dump                    # noqa: E402

EMU = os.path.join(ROOT, "tests", "jit_emu")
LLR_MAX = 20.0
OFFSET = 0.5
C2 = (2816, 8448, "bg1", 6)


def _build_emu(tmp_path, h, infobits, tag, cn="minsum"):
    src = jit_dump.jit_source(h, infobits, 0, cn)
    inc = tmp_path / f"emu_src_{tag}.h"
    inc.write_text(src)
    so = tmp_path / f"emu_{tag}.so"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-pthread", f"-DJIT_EMU_SRC=\"{inc}\"", "-I", EMU, "-o", str(so),
                           os.path.join(EMU, "jit_emu_main.cpp")])
    lib = C.CDLL(str(so))
    lib.jit_emu_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
    return lib, src


def edge_llr(code, batch, seed, sigma=0.8):
    """noisy codewords; row 0: first 7 values 0, row 1: rounded (exact ties), row 2: every fifth value x 40 (the clip),
    row 3: all zero (every message +-0: the signed-zero case), row 4: -0.0 inputs and magnitudes below the offset"""
    assert batch >= 5
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (batch, code.k)).astype(np.float32)
    c = code.encode(u)
    y = (2 * c - 1) + sigma * rng.normal(size=c.shape)
    llr = (2 * y / sigma ** 2).astype(np.float32)
    llr[0, :7] = 0
    llr[1] = np.round(llr[1])
    llr[2, ::5] *= 40
    llr[3] = 0
    llr[4, ::3] = np.sign(llr[4, ::3]) * np.float32(0.25)        # |v| - 0.5 < 0: clips to 0
    llr[4, 1::7] = np.float32(-0.0)
    assert np.signbit(llr[4, 1]) and llr[4, 1] == 0
    return llr


def _reference(code, llr, cn, it, infobits, m, hard):
    odec = obp.LDPC5GDecoder(code, cn_update=cn, hard_out=False, return_infobits=infobits, num_iter=it)
    xr = cbind.bp_decode(odec, odec.rate_recover(llr), num_iter=it, hard_out=0, offset=OFFSET)
    if infobits:
        ref = xr[:, :code.k]
    else:                                                        # decoding.py:1506-1531
        x_nf = np.concatenate([xr[:, :code.k], xr[:, code.k_ldpc:]], axis=1)
        ref = x_nf[:, 2 * code.z:2 * code.z + code.n]
        if m is not None:
            ref = ref[:, code.out_int]
    return (ref >= 0).astype(np.float32) if hard else ref        # hard: 0 >= x_hat (internal sign) = returned logit >= 0


def _check(lib, code, llr, m, rule, infobits, iters, grid=2):
    batch = llr.shape[0]
    x = np.ascontiguousarray(llr)
    for it in iters:
        soft = None if it == 0 else _reference(code, llr, rule, it, bool(infobits), m, 0)
        for hard in (0, 1):
            out = np.full((batch, code.k if infobits else code.n), np.nan, np.float32)
            lib.jit_emu_decode(x.ctypes.data, out.ctypes.data, batch, it, LLR_MAX, OFFSET if rule == "offset-minsum" else 0.0, hard, grid)
            if it == 0:                                          # no iteration: no output written
                assert np.isnan(out).all()
                continue
            ref = (soft >= 0).astype(np.float32) if hard else soft
            assert np.array_equal(out, ref), f"{rule} it={it} infobits={infobits} hard={hard}: {np.mean(out != ref):.3e} differ, " \
                                             f"nan {np.isnan(out).sum()}"


@pytest.mark.parametrize("infobits", [1, 0])
@pytest.mark.parametrize("rule", ["minsum", "offset-minsum"])
def test_c2_lean_first_iteration_matches_oracle(tmp_path, rule, infobits):
    """no iteration (nothing written), one (the old path: full init, last trip), two (FIRST + LAST), three and five (one and three
    loop trips between them); 5 codewords on a grid of 2: workgroup 0 decodes three in sequence, so the punctured columns' slots
    the first trip must not read hold another codeword's messages"""
    from sionna_amd import _ffi
    k, n, bg, m = C2
    code = LDPC5GCode(k, n, m, bg)
    h = jit_dump.host_only_handle(k, n, m, bg)
    llr = edge_llr(code, 5, k + n)
    lib, src = _build_emu(tmp_path, h, infobits, f"c2_{rule}_{infobits}", rule)
    assert "jit_cn_first<" in src and "jit_vnb_first<" in src and f"#define JIT_OFFSET0 {1 if rule == 'minsum' else 0}" in src
    _check(lib, code, llr, m, rule, infobits, (0, 1, 2, 3, 5))
    _ffi.lib().samd_ldpc5g_destroy(h)


# BG2 at Z = 128, with and without the output interleaver (any-lifting-size programs: no lean first trip, the same outputs);
# BG1 at Z = 256: the chunk-planar layout of the class (jit_vn_first, one and two chunks per item)
OTHER = [(1280, 3840, "bg2", None), (1280, 2560, "bg2", 2), (5632, 8448, "bg1", None)]


@pytest.mark.parametrize("k,n,bg,m", OTHER)
def test_other_codes_of_the_class_match_oracle(tmp_path, k, n, bg, m):
    from sionna_amd import _ffi
    h, enc, _ = jit_dump.host_only_handle(k, n, m, bg, return_obj=True)
    code = LDPC5GCode(k, n, m, enc._bg)
    llr = edge_llr(code, 5, k + n)
    for infobits in (1, 0):
        lib, src = _build_emu(tmp_path, h, infobits, f"o{k}_{n}_{infobits}")
        # (the BG2 codes get the any-lifting-size programs, which keep their whole first trip: same check, other text)
        general = "#define JIT_GENERAL 1" in src
        assert general == (bg == "bg2") and ("jit_cn_first<" in src) == (not general)
        assert ("jit_vn_first<" in src) == (not general and enc._z > 128)
        _check(lib, code, llr, m, "minsum", infobits, (2, 5))
    _ffi.lib().samd_ldpc5g_destroy(h)


def _first_trip(wave):
    """(init for every trip count, init of the punctured columns below two iterations, first check-node phase, first variable-node
    phase) of one wave's text"""
    head, rest = wave.split("    jit_barrier();\n    if (num_iter >= 2) {\n")
    head = head.split("    const float* row = ")[1]               # the codeword loop's body
    small = ""
    if "    if (num_iter < 2) {\n" in head:
        head, small = head.split("    if (num_iter < 2) {\n")
    parts = rest.split("    const int jit_rest = ")[0].split("jit_barrier();\n")
    assert len(parts) == 3 and parts[2].strip() == "}"           # CN | VN | (end): two barriers
    return head, small, parts[0], parts[1]


def test_static_counts_of_the_first_iteration():
    """C2's program, information bits out: 34 first check-node items - the rows with exactly one punctured column, each with its
    degree, the edge index of that column and its fused flag - 2 first variable-node items with 18 + 16 HAVE bits, no first item
    for any other row or column, init stores for 24 columns (the two punctured ones only below two iterations); boxplus-phi, the state variant and the
    any-lifting-size programs have no first trip"""
    from sionna_amd import _ffi
    k, n, bg, m = C2
    h, enc, _ = jit_dump.host_only_handle(k, n, m, bg, return_obj=True)
    rows, cols = np.asarray(enc._bg_rows), np.asarray(enc._bg_cols)
    deg = np.bincount(cols)
    expect = []                                                  # (degree, edge index of the punctured column, fused)
    two_zero = 0
    for r in range(rows.max() + 1):
        cs = np.sort(cols[rows == r])
        zero = [i for i, c in enumerate(cs) if c < 2]
        assert zero, "a row without a punctured column"
        if len(zero) == 1:
            expect.append((len(cs), zero[0], bool(deg[cs[-1]] == 1)))
        else:
            two_zero += 1
    assert len(expect) == 34 and two_zero == 12
    for rule in ("minsum", "offset-minsum"):
        src = jit_dump.jit_source(h, 1, 0, rule)
        found, have, n_lean_init, n_full_init = [], [], 0, 0
        for w in src.split("JIT_DEV void jit_wave_")[1:]:
            assert w.count("    if (num_iter >= 2) {\n") == 1 and w.count("    if (num_iter < 2) {\n") <= 1
            init, small, cnp, vnp = _first_trip(w)
            for mm in re.finditer(r"jit_cn_first<(\d+), 2, (true|false), (\d+)>", cnp):
                found.append((int(mm.group(1)), int(mm.group(3)), mm.group(2) == "true"))
            assert cnp.count("jit_cn_first<") == len(re.findall(r"jit_cn_first<\d+, 2, (?:true|false), \d+>", cnp))
            assert "jit_cn_update" not in cnp and "_first<" not in init + small and "jit_cn_first" not in vnp
            for mm in re.finditer(r"jit_vnb_first<(\d+), 0x([0-9a-f]+)u>", vnp):
                have.append((int(mm.group(1)), bin(int(mm.group(2), 16)).count("1")))
            assert vnp.count("_first<") == vnp.count("jit_vnb_first<") and "jit_vnb_update" not in vnp and "lds_ld" not in vnp
            n_lean_init += init.count("jit_vnb_init<")
            n_full_init += small.count("jit_vnb_init<")
            assert "jit_cn_init_fused<" not in small and (small == "") == (vnp.count("_first<") == 0)
        assert sorted(found) == sorted(expect)
        assert sorted(have) == [(28, 16), (30, 18)]
        assert n_lean_init == 24 and n_lean_init + n_full_init == 26 == int(np.sum(deg > 1))
    _ffi.set_option("SAMD_JIT_STATE", "1")
    try:
        state = jit_dump.jit_source(h, 1, 0, "minsum")
    finally:
        _ffi.set_option("SAMD_JIT_STATE", None)
    for text in (state, jit_dump.jit_source(h, 1, 0, "boxplus-phi")):
        assert "_first<" not in text and "num_iter >= 2" not in text
    _ffi.lib().samd_ldpc5g_destroy(h)
    hg = jit_dump.host_only_handle(2816, 8436, 6, "bg1")         # a pruned last row: the any-lifting-size programs
    text = jit_dump.jit_source(hg, 1, 0, "minsum")
    assert "JIT_GENERAL 1" in text and "_first<" not in text and "num_iter >= 2" not in text
    _ffi.lib().samd_ldpc5g_destroy(hg)
