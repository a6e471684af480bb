"""The host API's size and offset queries against tests/golden/api_layout.json, exactly (no GPU: host arithmetic).  Python reads
the error words at smm_error_word_offset and callers size their buffers by the other queries, so a byte that moves here is a
kernel reading the wrong place."""
import importlib.util
import json
import os

from action_segmentation_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_api_layout", os.path.join(GOLDEN, "make_golden_api_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_queries_answer_as_the_golden_table():
    gen = _generator()
    lib = gen.open_lib(_lib.LIB_PATH)
    with open(os.path.join(GOLDEN, "api_layout.json")) as f:
        table = json.load(f)
    assert len(table) >= 100
    assert [{k: v for k, v in r.items() if k != "out"} for r in table] == gen.rows()     # the table is the generator's grid
    for row in table:
        assert gen.measure(lib, row) == row["out"], row
        for name in row["zero"]:
            assert row["out"][name] == 0, (row, name)


def test_error_word_offset_lies_inside_the_workspace_metadata():
    gen = _generator()
    with open(os.path.join(GOLDEN, "api_layout.json")) as f:
        table = json.load(f)
    n = 0
    for row in table:
        out = row["out"]
        if row["kind"] != "smm" or out["workspace"] == 0:
            continue
        assert out["error_word_offset"] % 256 == 0 and 0 < out["error_word_offset"] + 512 <= out["workspace"]
        for name in ("kbest", "align"):
            assert out[name] == 0 or out[name] > out["workspace"]
        assert out["mbr"] in (0, out["workspace"])
        n += 1
    assert n >= 72
