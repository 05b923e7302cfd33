"""The status map's host side, without a GPU: the struct and the helpers of include/gpuscore.h, and that the truth the
GPU tests compare against (tests/fit_status_util.py) is a demanding one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from koordinator_amd import abi, build
from tests import fit_diag_util as fd
from tests import fit_status_util as fs

S = abi.GS_FAIL_NUMA_SHIFT


@pytest.fixture(scope="module")
def lib():
    build.build()
    return abi.load()


def test_struct_layout_matches_header(lib):
    """gs_status_map: the header's fields in order, the C layout of a 64-bit ABI, and the library's sizeof."""
    text = open(os.path.join(os.path.dirname(abi.PKG_DIR), "include", "gpuscore.h")).read()
    body = re.search(r"typedef struct gs_status_map \{(.*?)\} gs_status_map;", text, re.S).group(1)
    decl = re.findall(r"^\s*(uint16_t\*|uint32_t|int32_t\*)\s+(\w+);", body, re.M)
    ctype = {"uint16_t*": C.c_void_p, "int32_t*": C.c_void_p, "uint32_t": C.c_uint32}
    assert [(n, ctype[t]) for t, n in decl] == list(abi.GsStatusMap._fields_)
    assert [getattr(abi.GsStatusMap, n).offset for _, n in decl] == [0, 8, 16, 24, 28]
    assert C.sizeof(abi.GsStatusMap) == 32
    sizes = (C.c_uint64 * 20)()
    lib.gs_abi_sizes(sizes, 20)
    assert sizes[19] == abi.STRUCT_SIZES["gs_status_map"] == 32
    assert "#define GS_ABI_VERSION 6u" in text


def test_macros():
    text = open(os.path.join(os.path.dirname(abi.PKG_DIR), "include", "gpuscore.h")).read()
    assert "#define GS_STATUS_CODE(w)        ((uint32_t)(w) & 0x0FFFu)" in text
    assert "#define GS_STATUS_SCALAR_MASK(w) ((((uint32_t)(w) >> 12) & 0xFu) << 3)" in text
    for w in (0, 0x0002, 0x1010, 0xF01F, 0x0C20, 0x02C0, 0xFFFF):
        assert abi.status_code(w) == w & 0xFFF
        assert abi.status_scalar_mask(w) == ((w >> 12) & 0xF) << 3


def test_framework_code_of_numa_reasons(lib):
    """All 11 NodeNUMAResource reasons: the code gs_reason_string returns."""
    unresolvable = 0
    for r in range(1, 12):
        code, _ = abi.reason_string(r << S)
        assert code in (1, 2)
        assert abi.status_framework_code(r << S) == code, r
        assert (code == 2) == (r in fd.UNRESOLVABLE_NUMA), r
        unresolvable += code == 2
    assert unresolvable == 7
    assert abi.status_framework_code(0) == 0
    assert abi.status_framework_code(12 << S) < 0      # no such reason: malformed, as gs_reason_string says
    assert abi.status_framework_code(abi.GS_FAIL_LA_MEMORY) < 0


@pytest.mark.parametrize("cid,numa", [(0, False), (3, True)])
def test_framework_code_of_truth_words(lib, cid, numa):
    _, _, st = fs.status_case(700, 512, cid, numa)
    words = np.unique(np.concatenate([st.rows[k] for k in st.order]))
    assert words.size >= 4
    for w in words.tolist():
        code, _ = abi.reason_string(abi.status_code(w), abi.status_scalar_mask(w))
        assert code in (1, 2) and abi.status_framework_code(w) == code, hex(w)
    if numa:
        assert {abi.status_framework_code(w) for w in words.tolist()} == {1, 2}


def test_preemption_candidates(lib):
    U, R = abi.GS_FAIL_FIT_CPU, abi.GS_NUMA_MISSING_NUMA_RESOURCES << S    # Unschedulable, ...AndUnresolvable
    assert abi.status_framework_code(U) == 1 and abi.status_framework_code(R) == 2
    n, nodes = abi.preemption_candidates(np.full(9, R, np.uint16))          # none
    assert n == 0 and nodes.size == 0
    n, nodes = abi.preemption_candidates(np.full(9, U, np.uint16))          # all
    assert n == 9 and nodes.tolist() == list(range(9))
    row = np.array([U, R, R, U | abi.GS_FAIL_FIT_MEMORY, abi.GS_FAIL_LOADAWARE, R, abi.GS_NUMA_ALLOCATE_FAILED << S, R,
                    0x1010], np.uint16)
    n, nodes = abi.preemption_candidates(row)
    assert n == 5 and nodes.tolist() == [0, 3, 4, 6, 8]
    n, nodes = abi.preemption_candidates(row, cap=2)                        # cap smaller than the count
    assert n == 5 and nodes.tolist() == [0, 3]
    guard = np.full(4, 77, np.uint32)                                       # nothing past cap is written
    assert lib.gs_preemption_candidates(abi.ptr(row), 9, abi.ptr(guard), 2) == 5 and guard.tolist() == [0, 3, 77, 77]
    assert lib.gs_preemption_candidates(abi.ptr(row), 9, None, 0) == 5      # counting alone
    for w, want in ((U, [0]), (R, [])):                                     # one node
        n, nodes = abi.preemption_candidates(np.array([w], np.uint16))
        assert n == len(want) and nodes.tolist() == want
    assert lib.gs_preemption_candidates(None, 9, abi.ptr(guard), 4) == abi.GS_EINVAL
    assert lib.gs_preemption_candidates(abi.ptr(row), 9, None, 4) == abi.GS_EINVAL


def test_round_trip_names_exactly_the_short_slots():
    """gs_reason_string(GS_STATUS_CODE(w), GS_STATUS_SCALAR_MASK(w)) names exactly the slots of bits 12..15."""
    names = ["kubernetes.io/batch-cpu", "kubernetes.io/batch-memory", "kubernetes.io/mid-cpu", "kubernetes.io/mid-memory"]
    for bits in range(1, 16):
        w = abi.GS_FAIL_FIT_CPU | abi.GS_FAIL_FIT_SCALAR | bits << 12
        code, msg = abi.reason_string(abi.status_code(w), abi.status_scalar_mask(w))
        want = ["Insufficient cpu"] + [f"Insufficient {names[s]}" for s in range(4) if bits >> s & 1]
        assert code == 1 and msg == ", ".join(want), (bits, msg)
    # a word with unknown bits is refused as before: bits 12..15 are not part of the code
    assert abi.reason_string(0x1010)[0] < 0 and abi.reason_string(abi.status_code(0x1010), 8) == \
        (1, "Insufficient kubernetes.io/batch-cpu")
    for w, msg in ((abi.GS_FAIL_LOADAWARE | abi.GS_FAIL_LA_MEMORY, "node(s) memory usage exceed threshold"),
                   (abi.GS_NUMA_AFFINITY_ERROR << S, "node(s) NUMA Topology affinity error")):
        assert abi.reason_string(abi.status_code(w), abi.status_scalar_mask(w)) == (1, msg)


def test_null_arguments(lib):
    m = abi.GsStatusMap()
    assert lib.gs_schedule_diag_nodes(None, None, 0, None, None, None, C.byref(m)) == abi.GS_EINVAL
    t = C.c_uint64()
    assert lib.gs_schedule_submit_diag_nodes(None, None, 0, None, None, None, C.byref(m), C.byref(t)) == abi.GS_EINVAL


@pytest.mark.parametrize("cid,numa,moved,distinct", [(0, False, 60, 4), (3, True, 40, 10)])
def test_truth_is_demanding(cid, numa, moved, distinct):
    """Most rows differ from the row at their 128-pod window's start and from the one at its end (the oracle alone:
    84 of 121 and 64 of 143 pods), only on nodes the window landed on; no entry is 0; the rows' histograms are the
    diagnosis' truth."""
    c, t, st = fs.status_case(700, 512, cid, numa)
    assert st.order == np.nonzero(t.fit_errors)[0].tolist()
    assert np.array_equal(st.placements, t.placements)
    mv = st.moved()
    assert len(mv) >= moved, len(mv)
    for k in st.order:
        row = st.rows[k]
        assert row.shape == (700,) and (row != 0).all()
        landed = st.landed[k // fd.WINDOW]
        for other in (st.start[k], st.end[k]):
            assert set(np.nonzero(row != other)[0].tolist()) <= landed, k
        assert np.array_equal(fd.histogram(row & 0xFFF, fd.scalar_mask_of(c.pods[k])), t.hist[k]), k
        assert np.array_equal(fs.word_histogram(row), t.hist[k]), k
    assert len(np.unique(st.matrix())) == distinct
