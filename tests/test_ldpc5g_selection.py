"""Engine selection of the 5G LDPC handle is a recorded contract (CPU, handles built under SAMD_HOST_ONLY).

tests/golden/ldpc5g_selection.json holds, for a grid of codes (both base graphs, lifting sizes of every set, rates 1/3 ...
8/9, with and without the output interleaver, the two spill-threshold codes of tools/sweep_ldpc.py), for every cn_mode and
under each selection switch: samd_ldpc5g_decode_engine, samd_ldpc5g_decode_workspace_bytes at batch 1 / 255 / 256 / 4096,
samd_ldpc5g_decode_layered_supported and samd_ldpc5g_decode_layered_workspace_bytes.  tools/gen_ldpc5g_selection.py wrote
it from the library of the commit BEFORE the handle's tables and its engine choice were reorganised; a change that is
meant to leave the choice alone must reproduce it exactly.  INTEGRATION.md and tools/sweep_ldpc.py read these values.

A host-only handle owns no device table, so min-sum never reports the explicit-message engine in that record.
tests/golden/ldpc5g_selection_gpu.json is the same record for a few codes with handles on a device (written by the same
tool with --device, from the same earlier library): codes whose messages fit LDS - min-sum engine 2, one of them with the
channel LLRs in the workspace - and one that spills; test_device_selection_matches_the_record (gpu) holds it.

tests/golden/ldpc5g_tables.json (the same tool with --tables, the same grid) records what the table builders PRODUCE: per
code the 64-bit digest samd_debug_table_digest returns after samd_ldpc5g_create of a host-only handle - every device table
of every engine (element size, count, bytes, in build order) and the engines' scalars.  It was written from the library of
the commit before the tuning options of the hand-written engines were retired (that commit plus the digest entry alone), so
test_tables_match_the_record holds every schedule and table of those builders to what they were."""
import json

import pytest

from tools import gen_ldpc5g_selection as gen

with open(gen.FIXTURE) as _f:
    ROWS = json.load(_f)
with open(gen.DEVICE_FIXTURE) as _f:
    DEVICE_ROWS = json.load(_f)
with open(gen.TABLES_FIXTURE) as _f:
    TABLE_ROWS = json.load(_f)
GROUPS = sorted({(r["code"][0], r["none"][0]) for r in ROWS})          # (base graph, lifting size)


def test_fixture_covers_the_grid():
    assert [tuple(r["code"]) for r in ROWS] == gen.codes()
    assert {z for _, z in GROUPS} == set(gen.LIFTING) and {bg for bg, _ in GROUPS} == {"bg1", "bg2"}
    assert all(len(r["none"]) == 1 + 6 * len(gen.CN_MODES) + len(gen.BATCHES) for r in ROWS)
    # the grid reaches every answer: engines 0 ... 3 and a workspace need
    engines = {row[1 + 6 * m] for r in ROWS for sw, row in r.items() if sw != "code" for m in gen.CN_MODES}
    assert engines == {0, 1, 2, 3}
    assert any(r["none"][2] > 0 for r in ROWS)


@pytest.mark.parametrize("bg,z", GROUPS, ids=[f"{bg}-z{z}" for bg, z in GROUPS])
def test_selection_matches_the_record(bg, z):
    for r in ROWS:
        if (r["code"][0], r["none"][0]) != (bg, z):
            continue
        got = gen.measure(tuple(r["code"]))
        assert got is not None, r["code"]
        for sw in ("none",) + gen.SWITCHES:
            assert got[sw] == r.get(sw, r["none"]), (r["code"], sw)


def test_tables_fixture_covers_the_grid():
    assert [tuple(r["code"]) for r in TABLE_ROWS] == gen.codes()
    assert sorted({(r["code"][0], r["z"]) for r in TABLE_ROWS}) == GROUPS
    assert all(len(r["digest"]) == 16 and int(r["digest"], 16) >= 0 for r in TABLE_ROWS)
    # the digest separates the codes: every (base graph, k, n) has tables of its own, and the output interleaver shows
    # where the handle has a table for it (the bit-packed encoder's, lifting sizes that are multiples of 32)
    plain = {tuple(r["code"][:3]): r["digest"] for r in TABLE_ROWS if r["code"][3] is None}
    assert len(set(plain.values())) == len(plain) == len(TABLE_ROWS) // 2
    assert any(r["code"][3] == 6 and r["digest"] != plain[tuple(r["code"][:3])] for r in TABLE_ROWS)


@pytest.mark.parametrize("bg,z", GROUPS, ids=[f"{bg}-z{z}" for bg, z in GROUPS])
def test_tables_match_the_record(bg, z):
    for r in TABLE_ROWS:
        if (r["code"][0], r["z"]) == (bg, z):
            assert gen.table_digest(tuple(r["code"])) == [r["z"], r["digest"]], r["code"]


MINSUM, OFFSET = 2, 3                                                   # cn_mode values (include/sionna_amd.h)


def test_device_fixture_pins_the_explicit_message_choice():
    assert [tuple(r["code"]) for r in DEVICE_ROWS] == list(gen.DEVICE_CODES)
    fit = [r for r in DEVICE_ROWS if r["none"][1 + 6 * MINSUM] == 2]
    assert len(fit) >= 4 and {r["none"][0] for r in fit} >= {16, 96, 128}
    for r in fit:                                                       # SAMD_ONCHIP_COMPRESSED moves min-sum off that engine
        assert [r["SAMD_ONCHIP_COMPRESSED"][1 + 6 * m] for m in (MINSUM, OFFSET)] == [1, 1]
    assert any(r["none"][2 + 6 * MINSUM] > 0 for r in fit)              # ... one with the channel LLRs in the workspace
    assert any(r["none"][1] == 3 for r in DEVICE_ROWS)                  # ... and a code beyond LDS (boxplus: the spill engine)


@pytest.mark.gpu
@pytest.mark.parametrize("row", DEVICE_ROWS, ids=["-".join(str(x) for x in r["code"]) for r in DEVICE_ROWS])
def test_device_selection_matches_the_record(row):
    got = gen.measure(tuple(row["code"]), host_only=False)
    assert got is not None
    for sw in ("none",) + gen.SWITCHES:
        assert got[sw] == row.get(sw, row["none"]), (row["code"], sw)
