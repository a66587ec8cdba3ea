"""The generated min-sum programs with the LAST iteration peeled and lean, held to the oracle without a GPU.

After the last check-node phase nobody reads a v2c again, so the generator (csrc/ldpc5g_jit_gen.cpp) emits the last iteration of the
min-sum / offset-min-sum programs of the Z = 128 k class from `last` forms of the item bodies: the variable-node items of the
output columns form their totals (jit_vnb_total / jit_vn_total) and store nothing, the other columns have no item, and the
check-node items form and store c2v only for the edges those items read (the KEEP mask of jit_cn_update).  The state variant,
whose image IS the v2c of the last iteration, boxplus-phi and the any-lifting-size programs keep the whole last iteration.

Same emulation as tests/test_jit_emu.py: the generated text compiled with g++ against the 64-wide stand-ins of tests/jit_emu,
soft outputs and hard decisions array_equal to oracle/ldpc_bp.c.  (`-m gpu` twin: tests/test_gpu_jit_rotations.py.)

The lane rotations of the same issue (compile-time lane selections in the variable-node phase) are not built: there is no
solver and no constant mask to check here.
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


def _noisy_llr(code, batch, seed, sigma=0.8):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (batch, code.k)).astype(np.float32)
    c = code.encode(u)
    y = (2 * c - 1) + sigma * rng.normal(size=c.shape)
    llr = (2 * y / sigma ** 2).astype(np.float32)
    llr[0, :7] = 0
    llr[1] = np.round(llr[1])                                    # exact ties
    llr[2, ::5] *= 40                                            # clipping
    return llr


def _reference(code, llr, cn, it, infobits, m, hard, offset=0.5):
    odec = obp.LDPC5GDecoder(code, cn_update=cn, hard_out=False, return_infobits=infobits, num_iter=it)
    xr = cbind.bp_decode(odec, odec.rate_recover(llr), num_iter=it, hard_out=0, offset=offset)
    if infobits:
        ref = xr[:, :code.k]
    else:                                                        # decoding.py:1506-1531
        x_nf = np.concatenate([xr[:, :code.k], xr[:, code.k_ldpc:]], axis=1)
        ref = x_nf[:, 2 * code.z:2 * code.z + code.n]
        if m is not None:
            ref = ref[:, code.out_int]
    return (ref >= 0).astype(np.float32) if hard else ref        # hard: 0 >= x_hat (internal sign) = returned logit >= 0


def _check(lib, code, llr, m, rule, infobits, cases, grid=2):
    batch = llr.shape[0]
    for it, hard in cases:
        out = np.full((batch, code.k if infobits else code.n), np.nan, np.float32)
        x = np.ascontiguousarray(llr)
        lib.jit_emu_decode(x.ctypes.data, out.ctypes.data, batch, it, LLR_MAX, 0.5 if rule == "offset-minsum" else 0.0, hard, grid)
        ref = _reference(code, llr, rule, it, bool(infobits), m, hard)
        assert np.array_equal(out, ref), f"{rule} it={it} infobits={infobits} hard={hard}: {np.mean(out != ref):.3e} differ, " \
                                         f"nan {np.isnan(out).sum()}"


C2 = (2816, 8448, "bg1", 6)


@pytest.mark.parametrize("infobits", [1, 0])
def test_c2_minsum_lean_last_iteration_matches_oracle(tmp_path, infobits):
    """C2's code: one, two and five iterations (the peeled trip alone, one and four trips of the loop in front of it), soft
    outputs and hard decisions, both output forms; no iteration = no output written, as before"""
    from sionna_amd import _ffi
    k, n, bg, m = C2
    code = LDPC5GCode(k, n, m, bg)
    h = jit_dump.host_only_handle(k, n, m, bg)
    llr = _noisy_llr(code, 5, k + n)                             # workgroup 0 decodes 3 codewords in sequence, workgroup 1 two
    lib, src = _build_emu(tmp_path, h, infobits, f"c2_{infobits}")
    assert "#define JIT_LAYOUT_B 1" in src and "JIT_GENERAL" not in src.split("// specialised")[0]
    _check(lib, code, llr, m, "minsum", infobits, [(it, hard) for it in (1, 2, 5) for hard in (0, 1)])
    out = np.full((5, k if infobits else n), np.nan, np.float32)
    lib.jit_emu_decode(np.ascontiguousarray(llr).ctypes.data, out.ctypes.data, 5, 0, LLR_MAX, 0.0, 0, 2)
    assert np.isnan(out).all()
    _ffi.lib().samd_ldpc5g_destroy(h)


def test_c2_offset_minsum_lean_last_iteration_matches_oracle(tmp_path):
    """the second rule on the same bodies"""
    from sionna_amd import _ffi
    k, n, bg, m = C2
    code = LDPC5GCode(k, n, m, bg)
    h = jit_dump.host_only_handle(k, n, m, bg)
    llr = _noisy_llr(code, 5, k + n + 3)
    for infobits in (1, 0):
        lib, src = _build_emu(tmp_path, h, infobits, f"c2oms_{infobits}", "offset-minsum")
        assert "#define JIT_OFFSET0 0" in src and "jit_vnb_total<" in src
        _check(lib, code, llr, m, "offset-minsum", infobits, [(3, 0), (3, 1)])
    _ffi.lib().samd_ldpc5g_destroy(h)


# BG1 at Z = 128 with a pruned, partly filled last base row (any-lifting-size programs: PRUNE masks); BG2 at Z = 128 (other
# fused columns, other output columns); BG1 at Z = 256 (chunk-planar layout of the class: jit_vn_total, one and two chunks per item)
OTHER = [(2816, 8436, "bg1", 6), (1280, 3840, "bg2", None), (1280, 2560, "bg2", 2), (5632, 8448, "bg1", None)]


@pytest.mark.parametrize("k,n,bg,m", OTHER)
def test_other_codes_match_oracle(tmp_path, k, n, bg, m):
    from sionna_amd import _ffi
    h, enc, _ = jit_dump.host_only_handle(k, n, m, bg, return_obj=True)
    code = LDPC5GCode(k, n, m, enc._bg)
    assert _ffi.lib().samd_ldpc5g_jit_supported(h) == 1
    for infobits in (1, 0):
        lib, src = _build_emu(tmp_path, h, infobits, f"o{k}_{n}_{infobits}")
        group = int(src.split("// JIT_GROUP ")[1].split()[0]) if "// JIT_GROUP " in src else 1
        llr = _noisy_llr(code, 2 * group + 3, k + n)
        _check(lib, code, llr, m, "minsum", infobits, [(1, 0), (2, 1), (5, 0)])
    _ffi.lib().samd_ldpc5g_destroy(h)


def test_state_variant_keeps_the_whole_last_iteration(tmp_path):
    """2 + 3 iterations through the image = 5 in one call, and the mapped image = the oracle's msg_v2c: the image is the v2c of the
    last iteration, so the state variant has no lean last iteration"""
    from sionna_amd import _ffi
    lib0 = _ffi.lib()
    k, n, bg, m = C2
    h, enc, _ = jit_dump.host_only_handle(k, n, m, bg, return_obj=True)
    code = LDPC5GCode(k, n, m, enc._bg)
    mode = _ffi.CN_MODES["minsum"]
    img, cwpp = C.c_int(), C.c_int()
    assert lib0.samd_ldpc5g_state_layout(h, mode, C.byref(img), C.byref(cwpp)) == 0, lib0.samd_last_error().decode()
    img, cwpp = img.value, cwpp.value
    cw, cn, vn = (np.empty(img, np.int32) for _ in range(3))
    assert lib0.samd_ldpc5g_state_map(h, mode, cw.ctypes.data_as(C.c_void_p), cn.ctypes.data_as(C.c_void_p),
                                      vn.ctypes.data_as(C.c_void_p)) == 0
    _ffi.set_option("SAMD_JIT_STATE", "1")
    try:
        lib, src = _build_emu(tmp_path, h, 1, "c2_state")
    finally:
        _ffi.set_option("SAMD_JIT_STATE", None)
    assert "jit_copy_l2g" in src and "jit_vnb_total<" not in src and "if (num_iter > 0)" not in src
    lib.jit_emu_decode_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]
    batch, grid = 3, 2
    passes = -(-batch // cwpp)
    llr = _noisy_llr(code, batch, k + n + 1)

    def run(it, st_in, want):
        out = np.full((batch, k), np.nan, np.float32)
        st_out = np.full((passes, img), np.nan, np.float32) if want else None
        lib.jit_emu_decode_state(llr.ctypes.data, out.ctypes.data, batch, it, LLR_MAX, 0.0, 0, grid,
                                 None if st_in is None else st_in.ctypes.data, None if st_out is None else st_out.ctypes.data)
        return out, st_out

    out5, im5 = run(5, None, True)
    _, im2 = run(2, None, True)
    out23, im23 = run(3, im2, True)
    assert np.array_equal(out5, out23) and np.array_equal(im5, im23)
    assert np.array_equal(out5, _reference(code, llr, "minsum", 5, True, m, 0))
    # the lean programs give the same outputs as the state variant run without an image
    lean, _ = _build_emu(tmp_path, h, 1, "c2_lean")
    _check(lean, code, llr, m, "minsum", 1, [(5, 0)])
    # the oracle's state (VN-major edge order, logit sign) against the mapped image
    odec = obp.LDPC5GDecoder(code, cn_update="minsum", hard_out=False, return_infobits=True, num_iter=2, return_state=True)
    key = odec.vn_idx.astype(np.int64) * odec.num_cns + odec.cn_idx
    live = cw >= 0
    e = np.searchsorted(key, vn[live].astype(np.int64) * odec.num_cns + cn[live])
    assert np.array_equal(key[e], vn[live].astype(np.int64) * odec.num_cns + cn[live])
    _, st = odec.decode(odec.rate_recover(llr), num_iter=2)          # [E, B]
    got = np.full_like(st, np.nan)
    q = np.nonzero(live)[0]
    for p_ in range(passes):
        b = p_ * cwpp + cw[q]
        ok = b < batch
        got[e[ok], b[ok]] = -im2[p_, q[ok]]
    assert np.array_equal(got, st)
    lib0.samd_ldpc5g_destroy(h)


def test_static_counts_of_the_last_iteration():
    """what the issue lets one read off the generated source before any run: in C2's program (information bits out) the loop body
    carries no output code, the last variable-node phase has one total-only item per information column (22 of the 26 columns
    with items) and no store, and the last check-node phase stores exactly the edges of those columns"""
    from sionna_amd import _ffi
    k, n, bg, m = C2
    h, enc, _ = jit_dump.host_only_handle(k, n, m, bg, return_obj=True)
    z = enc._z
    rows, cols = np.asarray(enc._bg_rows), np.asarray(enc._bg_cols)
    deg = np.bincount(cols)
    n_rows = rows.max() + 1
    info_cols = k // z
    keep_edges = int(np.sum(cols < info_cols))
    for infobits, rule in ((1, "minsum"), (1, "offset-minsum")):
        src = jit_dump.jit_source(h, infobits, 0, rule)
        assert "if (last)" not in src.split("JIT_DEV void jit_wave_0(")[1]
        waves = src.split("JIT_DEV void jit_wave_")[1:]
        n_tot = n_upd = kept = n_cn_last = 0
        for w in waves:
            loop, last = w.split("    if (num_iter > 0) {\n")
            loop = loop.split("for (int it = 1; it < num_iter; ++it) {\n")[1]
            assert "g_st(" not in loop and "jit_vnb_total" not in loop
            assert "jit_vnb_update" not in last and "jit_vn_update" not in last
            assert loop.count("jit_barrier();") == 2 and last.count("jit_barrier();") == 1
            n_upd += loop.count("jit_vnb_update<")
            n_tot += last.count("jit_vnb_total<")
            for mm in re.finditer(r"jit_cn_update<(\d+), 2, (true|false), false, false, 0x([0-9a-f]+)u>", last):
                n_cn_last += 1
                kept += bin(int(mm.group(3), 16)).count("1")
                assert mm.group(2) == "false"                    # information bits out: no fused (parity) column is stored
            assert last.count("jit_cn_update<") == loop.count("jit_cn_update<")
        assert n_upd == int(np.sum(deg > 1)) == 26 and n_tot == info_cols == 22
        assert n_cn_last == n_rows == 46 and kept == keep_edges
    # the codeword out: every transmitted column keeps its item, the two punctured columns do not; fused totals are stored
    src = jit_dump.jit_source(h, 0, 0, "minsum")
    last = "".join(w.split("    if (num_iter > 0) {\n")[1] for w in src.split("JIT_DEV void jit_wave_")[1:])
    assert last.count("jit_vnb_total<") == 24
    assert len(re.findall(r"jit_cn_update<\d+, 2, true, false, false, 0x", last)) == 42
    # boxplus-phi keeps the loop as it was
    src = jit_dump.jit_source(h, 1, 0, "boxplus-phi")
    assert "if (num_iter > 0)" not in src and "const bool last = it == num_iter - 1;" in src
    _ffi.lib().samd_ldpc5g_destroy(h)
