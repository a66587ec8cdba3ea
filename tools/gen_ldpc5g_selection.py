"""Engine selection of the 5G LDPC handle over a grid of codes -> tests/golden/ldpc5g_selection.json.

RULE: the fixture is a record of what the library did BEFORE a change of the handle or of the selection code.  Generate it
against the PARENT commit's library, never against the branch under test:

    SAMD_LIB=<parent build>/libsionna_amd.so python tools/gen_ldpc5g_selection.py

tests/test_ldpc5g_selection.py runs `measure` of this file against the library of the tree and compares.

`--tables` records what the handle's table builders PRODUCE instead (-> tests/golden/ldpc5g_tables.json, same rule, same
grid): per code the digest samd_debug_table_digest returns after samd_ldpc5g_create - every device table of every engine
(element size, count, bytes) and the engines' scalars.  A refactoring of a builder must reproduce it exactly.

Runs WITHOUT a GPU: handles are built under SAMD_HOST_ONLY (tables and schedules only).  Such a handle owns no device
table, so its answers are those of a device handle whose explicit-message lists are absent: min-sum never reports the
explicit-message engine there.  `--device` records DEVICE_CODES with real handles on a GPU instead
(-> tests/golden/ldpc5g_selection_gpu.json, same rule: the parent's library), which pins that choice.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "ldpc5g_selection.json")
DEVICE_FIXTURE = os.path.join(ROOT, "tests", "golden", "ldpc5g_selection_gpu.json")
TABLES_FIXTURE = os.path.join(ROOT, "tests", "golden", "ldpc5g_tables.json")
# codes whose messages fit LDS (the explicit-message engine; 2816 / 8448 with the channel LLRs in the workspace), and one
# that does not
DEVICE_CODES = (("bg1", 352, 1056, 6), ("bg2", 960, 1920, None), ("bg1", 2112, 3168, 6), ("bg1", 2816, 8448, 6),
                ("bg1", 2816, 3168, None), ("bg1", 8448, 16896, 6))
LIFTING = (2, 3, 7, 16, 52, 96, 128, 176, 208, 256, 288, 384)      # one or more of every lifting set
RATES = ((1, 3), (1, 2), (2, 3), (8, 9))
SWITCHES = ("SAMD_ONCHIP_COMPRESSED", "SAMD_FORCE_SPILL", "SAMD_NO_SPILL", "SAMD_NO_ONCHIP_LAYERED", "SAMD_BP_ENGINE")
BATCHES = (1, 255, 256, 4096)
CN_MODES = (0, 1, 2, 3, 4)


def _bg2_k(z):
    for kb, above in ((10, 640), (9, 560), (8, 192), (6, 0)):        # k_b of BG2 depends on k (38.212 5.2.2)
        if kb * z > above:
            return kb * z


def codes():
    """(bg, k, n, m): k fills the base graph at the lifting size (k_b Z), n from the rate, m = 6 (output interleaver) / None.
    Each code once (at Z = 2 two rates round to the same n).  The grid holds the two codes of tools/sweep_ldpc.py that sit
    either side of the spill threshold, (8448, 25344) and (8448, 16896)."""
    out = []
    for bg in ("bg1", "bg2"):
        for z in LIFTING:
            k = 22 * z if bg == "bg1" else _bg2_k(z)
            for num, den in RATES:
                n = -(-k * den // (num * 6)) * 6
                out += [c for c in ((bg, k, n, 6), (bg, k, n, None)) if c not in out]
    return out


def _row(lib, h):
    """34 ints: per cn_mode (engine, workspace bytes at the four batches, layered supported), then the layered workspace"""
    row = []
    for mode in CN_MODES:
        row.append(int(lib.samd_ldpc5g_decode_engine(h, mode)))
        row += [int(lib.samd_ldpc5g_decode_workspace_bytes(h, b, mode)) for b in BATCHES]
        row.append(int(lib.samd_ldpc5g_decode_layered_supported(h, mode)))
    return row + [int(lib.samd_ldpc5g_decode_layered_workspace_bytes(h, b)) for b in BATCHES]


def _layers(code):
    """(encoder, decoder) of the Python layer for one code, or None when they refuse the parameters"""
    import sionna_amd.phy as phy
    bg, k, n, m = code
    try:
        enc = phy.fec.ldpc.LDPC5GEncoder(k, n, num_bits_per_symbol=m, bg=bg)
        return enc, phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum")
    except (ValueError, AssertionError):
        return None


def _create(lib, enc, dec, m):
    from sionna_amd import _ffi
    h = C.c_void_p()
    _ffi.check(lib.samd_ldpc5g_create(
        1 if enc._bg == "bg1" else 2, enc._z, enc._bg_rows.ctypes.data_as(C.c_void_p),
        enc._bg_cols.ctypes.data_as(C.c_void_p), enc._bg_shifts.ctypes.data_as(C.c_void_p), len(enc._bg_rows),
        enc._k, enc._n, 0 if m is None else int(m), int(dec._nb_pruned_nodes), C.byref(h)), "samd_ldpc5g_create")
    return h


def measure(code, host_only=True):
    """{switch or "none": [lifting size] + _row} for one code; None when the encoder / decoder refuse the parameters"""
    from sionna_amd import _ffi
    lib = _ffi.lib()
    layers = _layers(code)
    if layers is None:
        return None
    enc, dec = layers
    out = {}
    for sw in ("none",) + SWITCHES:
        _ffi.set_option("SAMD_HOST_ONLY", "1" if host_only else None)
        if sw != "none":
            _ffi.set_option(sw, "1")
        try:
            h = _create(lib, enc, dec, code[3])
        finally:
            _ffi.set_option("SAMD_HOST_ONLY", None)
            if sw != "none":
                _ffi.set_option(sw, None)
        out[sw] = [enc._z] + _row(lib, h)
        lib.samd_ldpc5g_destroy(h)
    return out


def table_digest(code):
    """[lifting size, digest as 16 hex digits] of a host-only handle's tables for one code; None when the layers refuse it"""
    from sionna_amd import _ffi
    lib = _ffi.lib()
    layers = _layers(code)
    if layers is None:
        return None
    enc, dec = layers
    _ffi.set_option("SAMD_HOST_ONLY", "1")
    try:
        lib.samd_debug_table_digest()                          # reset: the Python layers above built handles of their own
        h = _create(lib, enc, dec, code[3])
        digest = int(lib.samd_debug_table_digest())
    finally:
        _ffi.set_option("SAMD_HOST_ONLY", None)
    lib.samd_ldpc5g_destroy(h)
    return [enc._z, f"{digest:016x}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="DEVICE_CODES with handles on a GPU instead of the host-only grid")
    ap.add_argument("--tables", action="store_true", help="table digests of the host-only grid instead of the selection")
    ap.add_argument("--out", help="file to write (default: the fixture under tests/golden)")
    a = ap.parse_args()
    path = a.out or (TABLES_FIXTURE if a.tables else DEVICE_FIXTURE if a.device else FIXTURE)
    rows = []
    if a.tables:
        for code in codes():
            got = table_digest(code)
            if got is None:
                print("refused:", code)
                continue
            rows.append({"code": list(code), "z": got[0], "digest": got[1]})
    for code in (() if a.tables else DEVICE_CODES if a.device else codes()):
        got = measure(code, host_only=not a.device)
        if got is None:
            print("refused:", code)
            continue
        # a switch that changes nothing for a code is left out: its row is the "none" row
        rows.append({"code": list(code), **{sw: r for sw, r in got.items() if sw == "none" or r != got["none"]}})
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(f"{len(rows)} codes -> {path}")


if __name__ == "__main__":
    main()
