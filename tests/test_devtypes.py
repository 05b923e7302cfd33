"""RDMA and FPGA as DeviceShare device types, without a GPU: the integer restatement of tests/devtypes_util.py reproduces
the reference's own test vectors (tests/golden/devtypes.json), the edge inputs of the GPU test reach the branches they
aim at (shown on the truth alone), and the ABI declares the new calls and structs."""
import ctypes as C
import json
import os

import numpy as np

from koordinator_amd import abi
from tests import devtypes_util as du
from tests import ext_edges_util as xu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "devtypes.json")))
T_OF = {"rdma": du.RDMA, "fpga": du.FPGA}


def test_desired_requests_and_count_vectors():
    for v in GOLDEN["desired"]:
        inst, count, _ = du.py_aux_desired(v["q"], abi.AUX_STRATEGY[v["strategy"]], v["exclusive"], v["devices"])
        assert (inst, count) == (v["want_inst"], v["want_count"]), v["name"]


def test_allocate_vectors():
    for v in GOLDEN["allocate"] + GOLDEN["no_devices"]:
        devs = [du.dev(total=d["total"], used=d["used"], minor=d["minor"]) for d in v["devices"]]
        for weight, most in ((0, False), (1, False), (1, True)):
            ok, _, alloc = du.py_aux_type(devs, v["q"], du.NONE, 0, weight, most)
            assert ok == v["want_ok"], v["name"]
            if ok and not most:
                assert alloc[0] == v["want_minors"] and alloc[1] == v["want_inst"] and alloc[2] == 1, v["name"]
        aux = du.aux_pod(**{v["type"]: v["q"]})
        node = du.aux_node(**{v["type"]: devs})
        assert du.py_aux_node(node, 1, aux, (1, 1), False)[0] == v["want_ok"], v["name"]
        assert du.py_aux_node(node, 0, aux, (1, 1), False) == (True, 0, {})   # no Device object: DeviceShare passes


def test_percentage_validation():
    for q, ok in ((0, True), (1, True), (100, True), (101, False), (150, False), (200, True), (300, True), (250, False)):
        for s in du.STRATEGIES:
            assert du.py_aux_valid(du.aux_pod(rdma=q, strategy=(s, du.NONE))) == ok, (q, s)
            assert du.py_aux_valid(du.aux_pod(fpga=q, rdma=50, strategy=(du.NONE, s))) == ok, (q, s)
    assert du.py_aux_desired(200, du.COUNT, 1, 3)[:2] == (100, 2)    # the multi-device branch ignores the hint
    assert du.py_aux_desired(200, du.ALL, 0, 3)[:2] == (100, 2)
    assert du.py_aux_desired(7, du.ALL, 0, 3)[:2] == (7, 3)


def test_order_by_score_then_minor():
    devs = [du.dev(minor=31, used=10), du.dev(minor=3, used=50), du.dev(minor=17, used=10)]
    take = lambda w, most, q=10, s=du.NONE: du.py_aux_type(devs, q, s, 0, w, most)[2][0]   # noqa: E731
    assert take(0, False) == [3]             # no weight: every device scores 0, the minor decides
    assert take(1, False) == [17]            # least allocated: the emptier devices, the lower minor of the two
    assert take(1, True) == [3]              # most allocated: the fullest usable device
    assert take(1, True, q=60) == [17]       # ... that still fits
    assert take(1, False, q=2, s=du.COUNT) == [17, 31]


def test_edge_inputs_reach_their_branches():
    """every failure branch, every strategy branch and both scorers occur; the anchors do what they are named for"""
    seen = set()
    for vi in range(len(du.ROW_VARIANTS)):
        seen |= du.variant_truth(vi)[1]
    assert seen >= du.COVERAGE, du.COVERAGE - seen
    names = [n for n, _, _ in du.row_pods()]
    for vi, (_, aw, _, rot) in enumerate(du.ROW_VARIANTS):
        rows = du.variant_truth(vi)[0]
        where = du.cluster(rot)[4]
        row = lambda n: rows[names.index(n)]   # noqa: E731
        r50 = row("rdma50-s0-x0")
        assert r50["feasible"][where["nodev"]] == 1 and r50["ds_raw"][where["nodev"]] == 0
        for a in ("no-rdma", "unhealthy-only", "full", "noinfo-all", "rdma-full", "fit-short"):
            assert r50["feasible"][where[a]] == 0, a
        for a in ("no-fpga", "over", "noinfo-some", "minors", "half", "fpga-full", "gpu-full", "unhealthy-mixed"):
            assert r50["feasible"][where[a]] == 1, a
        assert row("rdma1-s1-x0")["feasible"][where["unhealthy-only"]] == 0       # ApplyForAll on an unhealthy entry
        assert row("rdma1-s1-x0")["feasible"][where["unhealthy-mixed"]] == 0      # ... counts the unhealthy entries
        assert row("rdma200-s2-x0")["feasible"][where["two-usable"]] == 1         # exactly count usable devices
        assert row("rdma200-s2-x0")["feasible"][where["one-usable"]] == 0         # count - 1
        assert row("rdma300-s0-x0")["feasible"][where["two-usable"]] == 0 and \
            row("rdma300-s0-x0")["feasible"][where["three-usable"]] == 1
        assert row("fpga1-s0")["feasible"][where["no-rdma"]] == 1 and row("fpga1-s0")["feasible"][where["no-fpga"]] == 0
        for n in ("both", "gpu-both"):
            assert row(n)["feasible"][where["fpga-full"]] == 0 and row(n)["feasible"][where["rdma-full"]] == 0
        assert row("both")["feasible"][where["gpu-full"]] == 1 and row("gpu-both")["feasible"][where["gpu-full"]] == 0
        for n in names:
            q = n.startswith("rdma101") or n.startswith("rdma150") or n in ("both-bad-fpga", "gpu-bad-both")
            assert (row(n)["fail_code"] == abi.GS_EXT_FAIL_POD) == q, n
        top = int(row("gpu-both")["ds_raw"].max())
        assert (top > 100) == (aw != (0, 0)), (vi, top)                           # the sum over the types passes 100
        if aw == (0, 0):
            assert np.array_equal(row("both")["ds_raw"], np.zeros(du.N, np.int32))
        # a single node at the raw maximum moves the normalization; all-equal raw scores keep the base's ties
        if aw != (0, 0):
            assert len(set(r50["ds_raw"][r50["feasible"] == 1].tolist())) > 2
        assert row("plain")["ties"] >= du.N - len(where) and row("plain")["node"] >= 0


def test_abi_declares_the_calls_and_structs():
    text = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "gpuscore.h")).read()
    assert "#define GS_ABI_VERSION 6u" in text and abi.GS_ABI_VERSION == 6
    new = ("gs_ext_configure_aux", "gs_node_aux_devices_upsert", "gs_node_aux_devices_get", "gs_schedule_ext_aux",
           "gs_ext_aux_reserved_get", "gs_debug_ext_rows_aux")
    lib = abi.load()
    for sym in new:
        assert sym in abi.header_symbols() and sym in abi.SIGNATURES and hasattr(lib, sym), sym
    for st in ("gs_aux_device", "gs_node_aux_devices", "gs_pod_aux", "gs_aux_placement"):
        assert "} %s;" % st in text, st
    sizes = {**abi.STRUCT_SIZES, **abi.AUX_STRUCT_SIZES}   # gs_abi_sizes: the earlier structs, then the four new ones
    names = list(sizes)
    assert names[-4:] == ["gs_aux_device", "gs_node_aux_devices", "gs_pod_aux", "gs_aux_placement"] and len(names) == 34
    arr = (C.c_uint64 * (len(names) + 1))()
    lib.gs_abi_sizes(arr, len(names) + 1)
    assert [int(x) for x in arr] == [sizes[n] for n in names] + [0]
    assert [sizes[n] for n in names[-4:]] == [32, 8 + 2 * 8 * 32, 32, 32]
    assert (abi.GS_MAX_AUX_DEVICES, abi.GS_NUM_AUX_TYPES) == (8, 2) and "#define GS_MAX_AUX_DEVICES 8" in text
    assert xu.ext_args().device_weights[1] == 1   # (the GPU defaults stay)
