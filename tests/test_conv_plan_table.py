"""CPU: the host-side conv planners of libfvc (make_cfg in csrc/fvc_conv.hip, x3_cfg in
csrc/fvc_conv_x3.hip, the all-classes deconv's config in csrc/fvc_deconv_x3.hip, all on the tap
geometry of csrc/fvc_taps.h) must keep answering every geometry query as recorded in
tests/golden/conv_plan_table.json: pack sizes, which kernel family takes a layer, the pack layout id
and the fused-epilogue forms. A pack written under one answer and launched under another is
garbage, and the answers decide which layers the product runs on which kernel.

The table is recorded with the planning switches unset, and again with FVC_DX=0 and with
FVC_X3_PT=0 (the library reads them on every call); for the two switches the file keeps only the
rows that differ from the unset table. It is regenerated with
    FVC_LIB_PATH=<libfvc.so of a trusted build> python tests/test_conv_plan_table.py > tests/golden/conv_plan_table.json
from a build of a commit whose plans are known good (the parent of the change under test), never
from the code under test."""
import itertools
import json
import os
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from fastvideocodec_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")

# ks 4 and stride 3 are refused by every planner: the refusals are part of the record
AXES = {"cin": [2, 3, 4, 8, 16, 32, 48, 64, 96, 128], "cout": [1, 2, 3, 4, 16, 32, 64, 96, 128, 160],
        "ks": [1, 3, 4, 5, 7], "stride": [1, 2, 3], "transposed": [0, 1]}
GRID = list(itertools.product(*AXES.values()))
COLUMNS = ["wpack_floats", "x3_supported", "x3_layout_id", "x3_wpack_bytes", "deconv_all_classes", "x3_tap_pcp20",
           "x3_tap_pcp28", "x3_tap_pcp32", "x3_pool"]
SETTINGS = {"unset": {}, "FVC_DX=0": {"FVC_DX": "0"}, "FVC_X3_PT=0": {"FVC_X3_PT": "0"}}
_PLAN_ENV = ("FVC_DX", "FVC_X3_")  # prefixes of the switches the planners read


def _row(lib, cin, cout, ks, stride, transposed):
    geo = (cin, cout, ks, stride, transposed)
    return [lib.fvc_conv_wpack_floats(*geo), lib.fvc_conv_x3_supported(*geo), lib.fvc_conv_x3_layout_id(*geo),
            lib.fvc_conv_x3_wpack_bytes(*geo), lib.fvc_deconv_x3_all_classes(cin, cout, ks, stride),
            lib.fvc_conv_x3_tap_supported(*geo, 20), lib.fvc_conv_x3_tap_supported(*geo, 28),
            lib.fvc_conv_x3_tap_supported(*geo, 32), lib.fvc_conv_x3_pool_supported(cin, cout, ks)]


def _table(setting):
    """every row of the grid under one setting; the process environment is put back afterwards"""
    saved = dict(os.environ)
    try:
        for k in [k for k in os.environ if k.startswith(_PLAN_ENV)]:
            del os.environ[k]
        os.environ.update(SETTINGS[setting])
        lib = _lib.load()
        return [_row(lib, *geo) for geo in GRID]
    finally:
        for k in [k for k in os.environ if k not in saved]:
            del os.environ[k]
        os.environ.update(saved)


def _expected(golden, setting):
    rows = [list(r) for r in golden["unset"]]
    if setting != "unset":
        for i, r in golden[setting].items():
            rows[int(i)] = r
    return rows


if __name__ != "__main__":
    with open(GOLDEN) as f:
        _GOLDEN = json.load(f)


def test_golden_describes_this_grid():
    assert _GOLDEN["axes"] == AXES and _GOLDEN["columns"] == COLUMNS
    assert len(_GOLDEN["unset"]) == len(GRID) == 3000
    assert sorted(k for k in _GOLDEN if k not in ("axes", "columns")) == sorted(SETTINGS)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_plans_match_recorded_table(setting):
    got, want = _table(setting), _expected(_GOLDEN, setting)
    bad = [(GRID[i], got[i], want[i]) for i in range(len(GRID)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} geometries differ (geometry, got, recorded), first: {bad[:5]}"


def test_grid_holds_every_kind_of_layer():
    """a table of zeros would match a library that refuses everything: the recorded unset table
    must hold each kind of plan, and each switch must change some rows"""
    col = {c: i for i, c in enumerate(COLUMNS)}
    rows = list(zip(GRID, _GOLDEN["unset"]))
    x3 = [(g, r) for g, r in rows if r[col["x3_supported"]]]
    pt_rows = {int(i) for i in _GOLDEN["FVC_X3_PT=0"]}
    kinds = {
        "all-classes deconv": [g for g, r in x3 if g[4] == 1 and r[col["deconv_all_classes"]]],
        "pair-tap": [GRID[i] for i in pt_rows if _GOLDEN["unset"][i][col["x3_supported"]]],
        "small-N refused by x3": [g for g, r in rows if g[1] <= 4 and r[col["wpack_floats"]] and g[0] % 8 == 0
                                  and not r[col["x3_supported"]]],
        "small-N taken by x3": [g for g, r in x3 if g[1] <= 4],
        "cin padded to 4": [g for g, r in x3 if g[0] <= 4],
        "tap epilogue": [g for g, r in x3 if r[col["x3_tap_pcp28"]]],
        "pool epilogue": [g for g, r in x3 if r[col["x3_pool"]]],
        "refused by every planner": [g for g, r in rows if not any(r)],
    }
    assert all(kinds.values()), {k: len(v) for k, v in kinds.items()}
    assert _GOLDEN["FVC_DX=0"] and _GOLDEN["FVC_X3_PT=0"]
    # FVC_DX=0 moves exactly the all-classes layers (they stay on x3, with another layout)
    assert sorted(GRID[int(i)] for i in _GOLDEN["FVC_DX=0"] if GRID[int(i)][4] == 1) == sorted(kinds["all-classes deconv"])


if __name__ == "__main__":
    base = _table("unset")
    out = {"axes": AXES, "columns": COLUMNS, "unset": base}
    for setting in SETTINGS:
        if setting != "unset":
            out[setting] = {str(i): r for i, r in enumerate(_table(setting)) if r != base[i]}
    # one row of integers per geometry
    sys.stdout.write('{"axes": %s,\n "columns": %s' % (json.dumps(AXES), json.dumps(COLUMNS)))
    sys.stdout.write(',\n "unset": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in base) + "]")
    for setting in SETTINGS:
        if setting != "unset":
            sys.stdout.write(',\n "%s": {\n' % setting + ",\n".join(
                '"%s":%s' % (i, json.dumps(r, separators=(",", ":"))) for i, r in out[setting].items()) + "}")
    sys.stdout.write("}\n")
