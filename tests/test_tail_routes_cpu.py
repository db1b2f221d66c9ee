"""The route table of SegPipeline's tails, pinned on the CPU: which ops calls ``segment_scene`` / ``segment_scenes`` make, with which
deciding arguments, in which order, and which ``pixel_bytes`` the planner is given -- for the full cross product of label_head x
prob_head x resize_head x PAMR x area_thd x Q in {8, 65} x wanted in {labels, probs, top-k 3} x ori_shapes x entry x flush_bytes
(tools/record_tail_routes.py: AXES).  No GPU and no library load: the ops are recorders that return zero tensors.

tail_routes_cpu.json was written by that tool run on the commit before the tails were collapsed into one route decision
(``python tools/record_tail_routes.py --repo <that checkout> --out tests/tail_routes_cpu.json``), so every case here is "the same calls
as before".  A route that is changed on purpose is re-recorded the same way, on the commit that changes it."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tail_routes_cpu.json")


def _tool():
    spec = importlib.util.spec_from_file_location("record_tail_routes", os.path.join(ROOT, "tools", "record_tail_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spell(table):
    return [[table["calls"][i] for i in table["sequences"][s]] for s in table["cases"]]


@pytest.fixture(scope="module")
def routes():
    tool = _tool()
    with open(TABLE) as f:
        want = json.load(f)
    got = tool.record()
    assert got["axes"] == want["axes"], "the recorded table was made for other axes: record it again"
    return tool.case_keys(), _spell(got), _spell(want)


def test_the_table_holds_the_full_cross_product(routes):
    keys, got, want = routes
    assert len(keys) == len(got) == len(want) == 3 * 3 * 2 * 2 * 2 * 2 * 3 * 3 * 2 * 2


@pytest.mark.parametrize("ori_shapes", ["none", "equal", "one_differs"])
@pytest.mark.parametrize("wanted", ["labels", "probs", "topk3"])
@pytest.mark.parametrize("entry", ["segment_scene", "segment_scenes"])
def test_every_case_makes_the_recorded_calls(routes, entry, wanted, ori_shapes):
    keys, got, want = routes
    n = 0
    for key, g, w in zip(keys, got, want):
        if (key["entry"], key["wanted"], key["ori_shapes"]) != (entry, wanted, ori_shapes):
            continue
        n += 1
        assert g == w, f"{key}:\n  now      {g}\n  recorded {w}"
    assert n == 3 * 3 * 2 * 2 * 2 * 2 * 2
