"""Digests of every source text the generator of the specialised 5G LDPC decoder (csrc/ldpc5g_jit_gen.cpp) produces for a set
of codes that hits each of its paths, and of the state layout it reports.  Runs WITHOUT a GPU (handles built under
SAMD_HOST_ONLY).  A change that must leave the generated kernels alone is checked by running this on the library before and
after it and comparing the two outputs:

    python tools/jit_source_digests.py > after.txt        (SAMD_LIB=<other libsionna_amd.so> for the library before)

One `sha256  length  key` line per code x rule x return_infobits x with_ops x state variant (`none`: no such variant), then
one `layout` line per code x rule: image floats, codewords per pass and the digest of the three samd_ldpc5g_state_map arrays.
profiles/jit_source_digests.txt is the record of one such comparison, not a fixture: a generator change regenerates it.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jit_dump import host_only_handle, jit_source  # noqa: E402

CODES = [(2816, 8448, "bg1", 6), (2816, 8448, "bg1", None), (2816, 5632, "bg1", 2), (5632, 8448, "bg1", None),
         (768, 1536, None, 2), (1024, 2048, "bg1", None), (1234, 2468, None, 4), (100, 200, None, None),
         (2816, 8436, "bg1", 6), (6144, 9216, "bg1", None), (30, 90, None, None)]
RULES = ["minsum", "offset-minsum", "boxplus-phi"]


def main():
    from sionna_amd import _ffi
    lib = _ffi.lib()
    for k, n, bg, m in CODES:
        h = host_only_handle(k, n, m, bg)
        for rule in RULES:
            for state in (None, "1"):
                _ffi.set_option("SAMD_JIT_STATE", state)
                for rib in (0, 1):
                    for ops in (0, 1):
                        key = f"k={k} n={n} bg={bg} m={m} {rule} rib={rib} ops={ops} state={state or 0}"
                        try:
                            src = jit_source(h, rib, ops, rule).encode()
                            print(f"{hashlib.sha256(src).hexdigest()}  {len(src)}  {key}")
                        except NotImplementedError:
                            print(f"none  {key}")
            _ffi.set_option("SAMD_JIT_STATE", None)
            img, cwpp = C.c_int(0), C.c_int(0)
            key = f"layout k={k} n={n} bg={bg} m={m} {rule}"
            if lib.samd_ldpc5g_state_layout(h, _ffi.CN_MODES[rule], C.byref(img), C.byref(cwpp)) != 0:
                print(f"none  {key}")
                continue
            maps = np.empty((3, img.value), np.int32)
            rc = lib.samd_ldpc5g_state_map(h, _ffi.CN_MODES[rule], *(maps[i].ctypes.data_as(C.c_void_p) for i in range(3)))
            print(f"{hashlib.sha256(maps.tobytes()).hexdigest()}  img={img.value} cwpp={cwpp.value} rc={rc}  {key}")


if __name__ == "__main__":
    main()
