"""The top-N score tables' host side, without a GPU: gs_debug_scores_string against the reference's own vector, the
selection of gs_top_select.h (the logic top_scores_kernel runs) against numpy, the structs, and that the truth the GPU
tests compare against (tests/top_scores_util.py) is a demanding one."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from koordinator_amd import abi, build
from tests import fit_diag_util as fd
from tests import top_scores_util as tu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debug_scores.json")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return abi.load()


# ---- gs_debug_scores_string ----
def test_debug_scores_golden(lib):
    """debug_test.go TestDebugScores: 10 plugins, 4 nodes, the rendered table byte for byte."""
    g = json.load(open(GOLDEN))
    names = list(g["plugins"])
    assert len(names) == 10 and len(g["nodes"]) == 4
    got = abi.debug_scores_string(g["topn"], g["pod"], g["nodes"], names, [g["plugins"][n] for n in names])
    assert got == g["expected"]
    # the plugin columns are sorted by name whatever order they arrive in
    rev = names[::-1]
    assert abi.debug_scores_string(g["topn"], g["pod"], g["nodes"], rev, [g["plugins"][n] for n in rev]) == g["expected"]


HEAD = "| # | Pod | Node | Score | A | B |\n| --- | --- | --- | ---:| ---:| ---:|"


def test_debug_scores_topn_and_ties(lib):
    nodes, sc = ["n0", "n1", "n2", "n3"], [[5, 7, 5, 1], [2, 0, 2, 6]]   # totals 7, 7, 7, 7
    line = lambda i, n: f"\n| {i} | ns/p | {nodes[n]} | 7 | {sc[0][n]} | {sc[1][n]} |"
    full = HEAD + "".join(line(i, i) for i in range(4))   # ties keep the input order
    for topn, rows in ((2, 2), (4, 4), (9, 4), (0, 0)):   # below, at and above the node count; none
        assert abi.debug_scores_string(topn, "ns/p", nodes, ["B", "A"][::-1], sc) == "\n".join(full.split("\n")[:2 + rows])
    sc2 = [[1, 9, 1, 9], [0, 0, 0, 0]]
    want = HEAD + "\n| 0 | ns/p | n1 | 9 | 9 | 0 |\n| 1 | ns/p | n3 | 9 | 9 | 0 |\n| 2 | ns/p | n0 | 1 | 1 | 0 |"
    assert abi.debug_scores_string(3, "ns/p", nodes, ["A", "B"], sc2) == want
    assert abi.debug_scores_string(8, "ns/p", [], ["A", "B"], np.zeros((2, 0))) == HEAD   # zero nodes
    assert abi.debug_scores_string(8, "ns/p", ["x"], [], np.zeros((0, 1))) == (
        "| # | Pod | Node | Score |\n| --- | --- | --- | ---:|\n| 0 | ns/p | x | 0 |")


def test_debug_scores_truncation(lib):
    g = json.load(open(GOLDEN))
    names = list(g["plugins"])
    nn = (C.c_char_p * 4)(*[n.encode() for n in g["nodes"]])
    pn = (C.c_char_p * 10)(*[n.encode() for n in names])
    sc = np.array([g["plugins"][n] for n in names], np.int64)
    args = (g["topn"], g["pod"].encode(), nn, 4, pn, 10, abi.ptr(sc))
    full = g["expected"].encode()
    assert lib.gs_debug_scores_string(*args, None, 0) == len(full)
    for cap in (1, 2, 100, len(full), len(full) + 1, len(full) + 50):
        buf = C.create_string_buffer(b"\xAA" * (cap + 8), cap + 8)
        assert lib.gs_debug_scores_string(*args, buf, cap) == len(full)
        assert buf.raw[:cap] == (full[:cap - 1] + b"\0" + b"\xAA" * cap)[:cap] and buf.raw[cap:] == b"\xAA" * 8
    assert lib.gs_debug_scores_string(-1, *args[1:], None, 0) == abi.GS_EINVAL
    assert lib.gs_debug_scores_string(4, None, *args[2:], None, 0) == abi.GS_EINVAL


def test_debug_scores_table_columns():
    """The table builder: a column per enabled score plugin, plugin x weight."""
    rows = np.zeros(2, abi.TOP_SCORE_DTYPE)
    rows["node"] = [3, 1]
    rows["plugin"] = [[10, 20, 30], [9, 8, 7]]
    cfg = fd.make_cfg(dataclasses.make_dataclass("C", ["num_nodes"])(4), True, weights=(7, 13, 2))
    names = [f"node-{i}" for i in range(4)]
    got = abi.debug_scores_table(rows, cfg, "d/p", names)
    assert got == ("| # | Pod | Node | Score | LoadAwareScheduling | NodeNUMAResource | NodeResourcesFit |\n"
                   "| --- | --- | --- | ---:| ---:| ---:| ---:|\n"
                   "| 0 | d/p | node-3 | 390 | 260 | 60 | 70 |\n| 1 | d/p | node-1 | 181 | 104 | 14 | 63 |")
    cfg.enabled = abi.GS_ENABLE_FIT_FILTER | abi.GS_ENABLE_LA_SCORE
    assert abi.debug_scores_table(rows, cfg, "d/p", names).split("\n")[2] == "| 0 | d/p | node-3 | 260 | 260 |"


# ---- the selection header against numpy ----
LENS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 2049)


def select(lib, row, excl, topn):
    row = np.ascontiguousarray(row, np.int16)
    excl = np.ascontiguousarray(excl, np.uint32)
    nodes, totals = np.full(topn, 0xFFFFFFFF, np.uint32), np.full(topn, -7, np.int16)
    lib.gsx_top_select.restype = C.c_int
    lib.gsx_top_select.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    n = lib.gsx_top_select(abi.ptr(row), len(row), abi.ptr(excl) if len(excl) else None, len(excl), topn,
                           abi.ptr(nodes), abi.ptr(totals))
    assert 0 <= n <= topn, n
    assert (nodes[n:] == 0xFFFFFFFF).all() and (totals[n:] == -7).all()   # nothing past the count is written
    return nodes[:n], totals[:n]


def select_numpy(row, excl, topn):
    ok = row >= 0
    ok[np.asarray(excl, np.int64)] = False
    cand = np.nonzero(ok)[0]
    order = cand[np.lexsort((cand, -row[cand].astype(np.int32)))][:topn]
    return order.astype(np.uint32), row[order]


def rows_of(n: int, s: np.random.RandomState):
    yield "all equal", np.full(n, 37, np.int16)
    yield "two levels", np.where(s.randint(0, 2, n) == 1, 100, 99).astype(np.int16)
    yield "0 and 2047", np.where(s.randint(0, 3, n) == 0, 2047, 0).astype(np.int16)
    r = s.randint(0, 40, n).astype(np.int16)
    r[s.randint(0, 3, n) == 0] = -1
    yield "holes", r
    yield "all holes", np.full(n, -1, np.int16)
    yield "random", s.randint(0, 2048, n).astype(np.int16)


def exclusions(n: int, s: np.random.RandomState):
    yield []
    yield [0]
    yield [n - 1]
    # 128 entries with index 0 and the last index (fewer distinct on a short row: duplicates, as repeated landings are)
    yield [0, n - 1] + s.randint(0, n, 126).tolist()


@pytest.mark.parametrize("n", LENS)
def test_select_header(lib, n):
    s = np.random.RandomState(n)
    for what, row in rows_of(n, s):
        for excl in exclusions(n, s):
            for topn in (1, 8, 63, 64):
                nodes, totals = select(lib, row, excl, topn)
                wn, wt = select_numpy(row, excl, topn)
                assert np.array_equal(nodes, wn) and np.array_equal(totals, wt), (what, n, len(excl), topn, nodes, wn)


# ---- structs ----
def test_structs_and_abi(lib):
    text = open(os.path.join(os.path.dirname(abi.PKG_DIR), "include", "gpuscore.h")).read()
    assert "#define GS_ABI_VERSION 6u" in text and abi.GS_ABI_VERSION == 6
    assert "#define GS_MAX_TOP_SCORES 64" in text and abi.GS_MAX_TOP_SCORES == 64
    assert abi.STRUCT_SIZES["gs_top_score"] == 12 and abi.STRUCT_SIZES["gs_top_scores"] == 24
    assert [abi.TOP_SCORE_DTYPE.fields[f][1] for f in ("node", "total", "plugin")] == [0, 4, 6]
    names = list(abi.STRUCT_SIZES)
    assert names[-2:] == ["gs_top_score", "gs_top_scores"]   # appended: the earlier indices keep their meaning
    arr = (C.c_uint64 * len(names))()
    lib.gs_abi_sizes(arr, len(names))
    assert [int(x) for x in arr] == [abi.STRUCT_SIZES[n] for n in names]
    for sym in ("gs_schedule_top_scores", "gs_schedule_submit_top_scores", "gs_debug_scores_string"):
        assert sym in abi.header_symbols() and sym in abi.SIGNATURES


# ---- the GPU cases' input conditions, on the oracle alone ----
def conditions(t: tu.Truth, topn: int):
    return (int((t.count(topn) > 0).sum()), int(t.moved(topn).sum()), int(t.cut_tie(topn).sum()),
            int(t.short(topn).sum()))


def test_conditions_tight():
    _, t = tu.case(700, 512, 0, False)
    assert (t.placements["node"] < 0).sum() >= 100                      # (the oracle alone: 121)
    tables, moved, cut, short = conditions(t, 8)                       # (391, 366, 218, 4)
    assert tables >= 350 and moved >= tables // 2 and cut >= 20 and short >= 1
    tables, moved, cut, short = conditions(t, 1)                       # (391, 321, ., 0)
    assert moved >= tables // 2 and short == 0
    tables, moved, cut, short = conditions(t, 64)                      # (391, 379, ., 78)
    assert moved >= tables // 2 and short >= 20


def test_conditions_numa():
    c, t = tu.case(700, 256, 3, True)
    tables, moved, cut, short = conditions(t, 8)                       # (181, 173, ., 0)
    assert tables >= 150 and moved >= tables // 2
    tables, moved, cut, short = conditions(t, 64)                      # (181, 177, ., 17)
    assert moved >= tables // 2 and short >= 5
    policy = c.numa["node_numa"]["numa_topology_policy"] != 0
    on_policy = sum(int(policy[t.table(i, 8)["node"]].sum()) for i in range(len(c.pods)))
    assert on_policy >= 100                                            # rows on nodes with a NUMA topology policy
    numa_scores = sum(int((t.table(i, 8)["plugin"][:, abi.GS_PLUGIN_NUMA] > 0).sum()) for i in range(len(c.pods)))
    assert numa_scores >= 100


def test_conditions_padding_tail():
    _, t = tu.case(1500, 640, 0, False)
    tables, moved, cut, short = conditions(t, 8)                       # (486, 450, ., .)
    assert tables >= 400 and moved >= tables // 2 and cut >= 20


def test_one_feasible_node_has_no_table():
    """A pod that fits one node only is placed, and [upstream] schedulePod never scores it: no table."""
    c, t = tu.one_feasible_case()
    k = tu.ONE_FEASIBLE_POD
    assert t.placements["feasible"][k] == 1 and t.placements["node"][k] >= 0
    assert t.count(8)[k] == 0 and len(t.kept[k]) == 1
    assert t.count(8)[k - 1] > 0 and t.count(8)[k + 1] > 0
