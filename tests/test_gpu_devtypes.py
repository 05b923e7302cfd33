"""RDMA and FPGA as DeviceShare device types on the device path (gs_schedule_ext_aux: eval_aux_type in gs_ext.hip,
aux_reserve_row / aux_unreserve_row in gs_engine.cpp) against the truth of tests/devtypes_util.py: the oracle for Fit,
LoadAware and the GPU type plus an integer restatement of the two types, never the code under test. 513 nodes: the
anchors sit on the 256-thread boundaries of ext_nodes_kernel (0, 255, 256, 511, 512; chunk boundaries of the select
passes too) and rotate over them from variant to variant; every other node is a benign filler.
Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from koordinator_amd import abi
from oracle import oracle as orc
from tests import devtypes_util as du
from tests import ext_edges_util as xu
from tests import numa_edges_util as nu

pytestmark = pytest.mark.gpu


def _engine(nodes, devs, table, args, weights, cfg=None):
    from koordinator_amd.engine import Engine
    e = Engine(cfg or du.make_cfg())
    du.load(e, nodes, devs, args)
    e.ext_configure_aux(weights)
    e.upsert_aux_devices(table.records())
    return e


def _state(e, n=du.N):
    return b"".join(e.devices(i).tobytes() + e.aux_devices(i).tobytes() for i in range(n))


def _assert_rows(got, want, what):
    d = xu.rows_equal(got, want)
    assert d is None, f"{what}: engine vs truth {d}"


@pytest.mark.parametrize("vi", range(len(du.ROW_VARIANTS)), ids=[str(v) for v in du.ROW_VARIANTS])
def test_rows_match_truth_and_leave_no_state(vi):
    gw, aw, strategy, rot = du.ROW_VARIANTS[vi]
    nodes, devs, table, _, _ = du.cluster(rot)
    e = _engine(nodes, devs, table, xu.ext_args(strategy, gw), aw)
    before = _state(e)
    want = du.variant_truth(vi)[0]
    for k, (name, aux, gpu) in enumerate(du.row_pods()):
        _assert_rows(e.ext_rows_aux(du.one_pod(k), du.ext_of(aux, gpu), aux, k), want[k], f"{du.ROW_VARIANTS[vi]} {name}")
    assert e.mirror_check() == 0 and _state(e) == before
    assert all(e.ext_reserved(int(du.one_pod(k)["uid"])) is None and e.ext_aux_reserved(int(du.one_pod(k)["uid"])) is None
               for k in range(len(want)))


def _flat(aux_used=0, cpu_used=None):
    """513 identical nodes: two RDMA devices and one FPGA device each"""
    nodes = xu.base_nodes(du.N)
    if cpu_used is not None:
        nodes["requested"][:, 0] = nodes["nonzero_requested"][:, 0] = cpu_used
    devs = np.array([xu.device(du.GPUS4)] * du.N, abi.NODE_DEVICES_DTYPE)
    devs["xres_allocatable"][:, :2] = 1600
    table = du.AuxTable([du.aux_node(rdma=[du.dev(used=aux_used), du.dev(used=aux_used)], fpga=[du.dev()])] * du.N)
    return nodes, devs, table


def test_select_equal_aux_scores_keep_the_ties_and_one_maximum_moves_the_normalization():
    cpu = np.full(du.N, 32000)
    high = [0, 255, 256, 511, 512, 300]
    cpu[high] = 0                                  # the base's ties: six emptier nodes on the boundaries
    nodes, devs, table = _flat(aux_used=40, cpu_used=cpu)
    args, aw = xu.ext_args("LeastAllocated", (0, 1, 0)), (2, 1)
    aux, pod = du.aux_pod(rdma=20), du.one_pod(1)
    ext = du.ext_of(aux)
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)
    e = _engine(nodes, devs, table, args, aw)
    for seq in range(12):
        want = t.rows(pod, ext, aux, seq)[0]
        assert want["ties"] == len(high) and want["node"] in high and want["ds_norm"] == 100
        _assert_rows(e.ext_rows_aux(pod, ext, aux, seq), want, f"equal aux scores, seq {seq}")
    # node 257 alone has free RDMA devices: it is the raw maximum, every other node's normalized score drops, and with
    # DeviceShare at weight 1000 it wins over the base's emptier nodes
    table.nodes[257][du.RDMA] = [du.dev(minor=0), du.dev(minor=1)]
    args = xu.ext_args("LeastAllocated", (0, 1, 0), w_ds=1000)
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)
    e = _engine(nodes, devs, table, args, aw)
    want = t.rows(pod, ext, aux, 3)[0]
    assert want["node"] == 257 and want["ties"] == 1 and want["ds_norm"] == 100
    assert 0 < want["total"][0] - want["base"][0] < 100 * 1000
    _assert_rows(e.ext_rows_aux(pod, ext, aux, 3), want, "one node at the raw maximum")


def _run_queue(e, t, queue, forget_every=0):
    """(pod, ext, aux) in turn through gs_schedule_ext_aux and the truth; every forget_every-th placement is forgotten"""
    placed = 0
    for k, (pod, ext, aux) in enumerate(queue):
        seq = 5000 + k
        out, eo, ao = e.schedule_ext_aux([pod], [ext], [aux], np.array([seq], np.uint64))
        node, feasible, want_ao = t.schedule(pod, ext, aux, seq)
        assert (int(out["node"][0]), int(out["feasible"][0])) == (node, feasible), f"pod {k}: {out[0]} vs {node}, {feasible}"
        assert ao[0].tobytes() == want_ao.tobytes(), f"pod {k}: {ao[0]} vs {want_ao}"
        if node < 0:
            continue
        uid = int(pod["uid"])
        rec = e.ext_aux_reserved(uid)
        if any(int(q) for q in aux["request"]):
            assert rec is not None and rec[0] == node and rec[1].tobytes() == want_ao.tobytes()
        placed += 1
        if forget_every and placed % forget_every == 0:
            assert t.forget(pod) == node
            e.forget(np.array([node], np.uint32), np.array([pod], abi.POD_DTYPE))
            assert e.ext_aux_reserved(uid) is None and e.ext_reserved(uid) is None
    return placed


def _same_state(e, t):
    for i in range(du.N):
        assert e.aux_devices(i).tobytes() == du.aux_record(t.table.nodes[i]).tobytes(), f"aux row {i}"
        assert e.devices(i).tobytes() == t.o.devices(i).tobytes(), f"Device row {i}"
    assert e.mirror_check() == 0


@pytest.mark.parametrize("strategy,aw", [("LeastAllocated", (0, 0)), ("LeastAllocated", (1, 1)), ("MostAllocated", (1, 1))],
                         ids=str)
def test_fill_an_anchor_device_by_device(strategy, aw):
    """only node 256 has RDMA devices (minors 17, 3, 31 with 40, 40 and 80 free): 40-unit pods fill them one by one in
    the order the scorer and the minor give, a two-device pod takes two where two are usable, and the first pod that fits
    nowhere gets node -1 with feasible 0"""
    nodes, devs, _ = _flat()
    table = du.AuxTable([du.aux_node()] * du.N)
    table.nodes[256] = du.aux_node(rdma=[du.dev(minor=17, used=60), du.dev(minor=3, used=60), du.dev(minor=31, used=20)])
    args = xu.ext_args(strategy, (0, 1, 0))
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)
    e = _engine(nodes, devs, table, args, aw)
    two = du.aux_pod(rdma=2, strategy=(du.COUNT, du.NONE))
    asks = [du.aux_pod(rdma=40), du.aux_pod(rdma=40), two, du.aux_pod(rdma=40), du.aux_pod(rdma=30),
            du.aux_pod(rdma=2, strategy=(du.COUNT, du.NONE), exclusive=(1, 0))]
    masks = []
    for k, aux in enumerate(asks):
        pod, ext = du.one_pod(100 + k), du.ext_of(aux)
        want = t.rows(pod, ext, aux, k)[0]
        _assert_rows(e.ext_rows_aux(pod, ext, aux, k), want, f"pod {k} before its Reserve")
        out, eo, ao = e.schedule_ext_aux([pod], [ext], [aux], np.array([k], np.uint64))
        node, feasible, want_ao = t.schedule(pod, ext, aux, k)
        assert (int(out["node"][0]), int(out["feasible"][0])) == (node, feasible) and ao[0].tobytes() == want_ao.tobytes(), k
        masks.append(int(ao["minor_mask"][0][du.RDMA]))
    # least allocated starts on the emptiest device (31), then score ties go to the lowest minor (3): 17 and 31 keep 40
    # each, the two-device pod takes both, and 40 then fits nowhere. Unweighted, and most allocated (the fullest usable
    # device), start on 3, then 17: only 31 is left, the two-device pod fits nowhere, the 40 and the 30 land on 31.
    least = (strategy, aw) == ("LeastAllocated", (1, 1))
    assert masks[:2] == ([1 << 31, 1 << 3] if least else [1 << 3, 1 << 17])
    assert [bin(m).count("1") for m in masks] == ([1, 1, 2, 0, 1, 0] if least else [1, 1, 0, 1, 1, 0])
    _same_state(e, t)


def _mixed_queue(n, uid0):
    """plain, GPU-only and aux-only pods in turn; the aux asks walk the strategies and sizes"""
    asks = [du.aux_pod(rdma=30), du.aux_pod(rdma=100, fpga=50), du.aux_pod(rdma=200), du.aux_pod(fpga=100),
            du.aux_pod(rdma=10, strategy=(du.ALL, du.NONE)), du.aux_pod(rdma=2, fpga=1, strategy=(du.COUNT, du.COUNT)),
            du.aux_pod(rdma=1, strategy=(du.COUNT, du.NONE), exclusive=(1, 0)), du.aux_pod(rdma=150), du.aux_pod(rdma=60)]
    gpus = [{xu.KG: 100}, {xu.CO: 50, xu.RA: 50}, {xu.NV: 2}, {xu.ME: 40 * xu.GiB}]
    out = []
    for k in range(n):
        pod = du.one_pod(uid0 + k, cpu=1000 + 500 * (k % 5))
        if k % 3 == 0:
            aux = asks[(k // 3) % len(asks)]
            out.append((pod, du.ext_of(aux), aux))
        elif k % 3 == 1:
            out.append((pod, du.ext_of(du.aux_pod(), gpus[(k // 3) % len(gpus)]), du.aux_pod()))
        else:
            out.append((pod, du.ext_of(du.aux_pod()), du.aux_pod()))
    return out


def test_mixed_queue_against_the_sequential_truth():
    nodes, devs, table, _, _ = du.cluster(3)
    args, aw = xu.ext_args("MostAllocated", (1, 1, 1)), (3, 2)
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)
    e = _engine(nodes, devs, table, args, aw)
    assert _run_queue(e, t, _mixed_queue(150, 1000)) >= 140
    _same_state(e, t)


def test_forget_every_third_placement():
    nodes, devs, table, _, _ = du.cluster(7)
    args, aw = xu.ext_args("LeastAllocated", (0, 1, 0)), (1, 1)
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)
    e = _engine(nodes, devs, table, args, aw)
    assert _run_queue(e, t, _mixed_queue(60, 2000), forget_every=3) >= 55
    _same_state(e, t)


def test_forget_restores_used_and_the_next_rows():
    from koordinator_amd.engine import GpuScoreError
    nodes, devs, table, _, _ = du.cluster(0)
    args, aw = xu.ext_args("MostAllocated", (0, 1, 0)), (1, 1)
    e = _engine(nodes, devs, table, args, aw)
    fresh = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)     # never sees the forgotten pod
    before = _state(e)
    aux = du.aux_pod(rdma=200, fpga=30)
    pod, ext = du.one_pod(300), du.ext_of(aux)
    out, eo, ao = e.schedule_ext_aux([pod], [ext], [aux], np.array([9], np.uint64))
    node = int(out["node"][0])
    want_row, alloc = fresh.rows(pod, ext, aux, 9)
    assert node == want_row["node"] >= 0 and ao[0].tobytes() == du.placement_of(alloc).tobytes() and _state(e) != before
    with pytest.raises(GpuScoreError, match="was assumed on node"):    # the wrong node: GS_EINVAL, nothing changes
        e.forget(np.array([(node + 1) % du.N], np.uint32), np.array([pod], abi.POD_DTYPE))
    assert e.ext_aux_reserved(int(pod["uid"]))[0] == node
    e.forget(np.array([node], np.uint32), np.array([pod], abi.POD_DTYPE))
    assert _state(e) == before and e.ext_aux_reserved(int(pod["uid"])) is None and e.mirror_check() == 0
    nxt = du.aux_pod(rdma=100, fpga=100)
    _assert_rows(e.ext_rows_aux(du.one_pod(301), du.ext_of(nxt), nxt, 10),
                 fresh.rows(du.one_pod(301), du.ext_of(nxt), nxt, 10)[0], "the next pod after the forget")
    # the aux row loses a minor and shrinks the other's used between Reserve and forget: the lost minor is skipped, the
    # subtraction floors at 0
    out, eo, ao = e.schedule_ext_aux([pod], [ext], [aux], np.array([9], np.uint64))
    assert int(out["node"][0]) == node and bin(int(ao["minor_mask"][0][du.RDMA])).count("1") == 2
    row = e.aux_devices(node).copy()
    keep = int(row["dev"][du.RDMA][0]["minor"])
    assert int(ao["minor_mask"][0][du.RDMA]) >> keep & 1
    others = [k for k in range(int(row["num"][du.RDMA])) if k != 0 and not int(ao["minor_mask"][0][du.RDMA]) >> int(row["dev"][du.RDMA][k]["minor"]) & 1]
    row["num"][du.RDMA] = 1 + len(others)
    kept = [row["dev"][du.RDMA][0].copy()] + [row["dev"][du.RDMA][k].copy() for k in others]
    for k, d in enumerate(kept):
        row["dev"][du.RDMA][k] = d
    row["dev"][du.RDMA][0]["used"] = 30
    e.upsert_aux_devices(np.array([row], abi.NODE_AUX_DEVICES_DTYPE), np.array([node], np.uint32))
    e.forget(np.array([node], np.uint32), np.array([pod], abi.POD_DTYPE))
    after = e.aux_devices(node)
    assert int(after["num"][du.RDMA]) == 1 + len(others) and int(after["dev"][du.RDMA][0]["used"]) == 0
    assert int(after["dev"][du.FPGA][0]["used"]) == int(du.aux_record(table.nodes[node])["dev"][du.FPGA][0]["used"])
    assert e.devices(node).tobytes() == devs[node].tobytes() and e.mirror_check() == 0


def test_gpu_and_aux_pod_reserves_all_three_types():
    """a pod asking GPU + RDMA + FPGA on a fixed state: the node by the truth's rows, the GPU minors by the oracle's own
    scheduleOne on a one-node cluster holding the chosen node's rows, the aux minors by the restatement"""
    nodes, devs, table, _, _ = du.cluster(11)
    args, aw = xu.ext_args("LeastAllocated", (1, 1, 1)), (3, 2)
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, aw)
    e = _engine(nodes, devs, table, args, aw)
    aux, gpu = du.aux_pod(rdma=200, fpga=40), {xu.NV: 2}
    pod, ext = du.one_pod(400), du.ext_of(aux, gpu)
    want, alloc = t.rows(pod, ext, aux, 21)
    out, eo, ao = e.schedule_ext_aux([pod], [ext], [aux], np.array([21], np.uint64))
    node = int(out["node"][0])
    assert node == want["node"] >= 0 and int(out["score"][0]) == want["score"] and int(out["ties"][0]) == want["ties"]
    assert ao[0].tobytes() == du.placement_of(alloc).tobytes() and int(eo["deviceshare_score"][0]) == want["ds_norm"]
    assert orc.device_allocate(devs[node], ext) == 0
    from koordinator_amd import config
    o1 = orc.Oracle(config.make_config(1, enabled=xu.FIT))
    du.load(o1, nodes[node:node + 1], devs[node:node + 1], args)
    w_out, w_eo = o1.schedule_ext(np.array([pod], abi.POD_DTYPE), np.array([ext], abi.POD_EXT_DTYPE), np.array([21], np.uint64))
    assert int(w_out["node"][0]) == 0
    for f in ("gpu_minor_mask", "gpu_count", "gpu_per_instance"):
        assert np.array_equal(eo[f][0], w_eo[f][0]), f
    assert e.devices(node).tobytes() == o1.devices(0).tobytes() and e.mirror_check() == 0
    rec = e.ext_reserved(int(pod["uid"]))
    assert rec[0] == node and int(rec[1]["gpu_minor_mask"]) == int(eo["gpu_minor_mask"][0])


def test_unchanged_path_through_the_new_entry_point():
    """a small Reservation + DeviceShare case through gs_schedule_ext, gs_schedule_ext_aux(aux = NULL) and an all-zero
    aux array: the same placements, gs_ext_placement records and final device and reservation bytes"""
    from koordinator_amd.engine import Engine
    case = xu.rsv_case()
    results = []
    for mode in ("ext", "aux-null", "aux-zero"):
        e = Engine(case.cfg())
        case.load(e)
        seq = np.arange(len(case.pods), dtype=np.uint64) + 40
        if mode == "ext":
            out, eo = e.schedule_ext(case.pods, case.ext, seq)
        else:
            aux = None if mode == "aux-null" else np.zeros(len(case.pods), abi.POD_AUX_DTYPE)
            out, eo, ao = e.schedule_ext_aux(case.pods, case.ext, aux, seq)
            assert ao.tobytes() == np.zeros(len(case.pods), abi.AUX_PLACEMENT_DTYPE).tobytes()
        state = b"".join(e.devices(i).tobytes() for i in range(case.n)) + \
            b"".join(e.reservation(int(r["uid"])).tobytes() for r in case.reservations)
        results.append((out.tobytes(), eo.tobytes(), state))
        assert e.mirror_check() == 0 and (out["node"] >= 0).sum() >= 25
    assert results[0] == results[1] == results[2]


def test_refusals():
    from koordinator_amd.engine import Engine, GpuScoreError
    nodes, devs, table, _, _ = du.cluster(0)
    args = xu.ext_args()
    e = _engine(nodes, devs, table, args, (1, 1))
    aux, pod = du.aux_pod(rdma=50), du.one_pod(500)
    for ext, msg in ((xu.ext_records(owner=[7])[0], "reservation owner or a required reservation"),
                     (xu.ext_records(owner=[0], required=[1])[0], "reservation owner or a required reservation")):
        for call in (lambda: e.ext_rows_aux(pod, ext, aux, 0), lambda: e.schedule_ext_aux([pod], [ext], [aux])):
            with pytest.raises(GpuScoreError, match=msg):
                call()
    with pytest.raises(GpuScoreError, match=r"RDMA / FPGA request outside \[0, 2\^53\)"):
        e.ext_rows_aux(pod, du.ext_of(aux), du.aux_pod(rdma=1 << 53), 0)
    one = np.array([5], np.uint32)
    rec = lambda *ds: np.array([du.aux_record(du.aux_node(rdma=list(ds)))], abi.NODE_AUX_DEVICES_DTYPE)   # noqa: E731
    for r, msg in ((rec(du.dev(minor=4), du.dev(minor=4)), "duplicate RDMA / FPGA minor on node 5"),
                   (rec(du.dev(minor=32)), "RDMA / FPGA minor outside 0..31"),
                   (rec(du.dev(total=1 << 53)), r"RDMA / FPGA quantity outside \[0, 2\^53\)")):
        before = e.aux_devices(5).tobytes()
        with pytest.raises(GpuScoreError, match=msg):
            e.upsert_aux_devices(r, one)
        assert e.aux_devices(5).tobytes() == before
    e.upsert_aux_devices(rec(du.dev(minor=31, total=(1 << 53) - 1)), one)
    e.upsert_aux_devices(table.records()[5:6], one)
    # the context stays usable: the same pod without the refused inputs matches the truth
    t = du.Truth(du.make_cfg(), nodes, devs, table, args, (1, 1))
    _assert_rows(e.ext_rows_aux(pod, du.ext_of(aux), aux, 4), t.rows(pod, du.ext_of(aux), aux, 4)[0], "after the refusals")
    assert e.mirror_check() == 0 and e.ext_aux_reserved(int(pod["uid"])) is None
    # any node with a NUMA topology policy
    zone = (8000, 32 * xu.GiB)
    numa_nodes = tuple(nu.Node(f"n{i}", "Restricted" if i == 2 else "", (zone, zone)) for i in range(4))
    case = xu.Case("aux-numa", np.zeros(4, abi.NODE_DTYPE), np.array([xu.device(du.GPUS4)] * 4, abi.NODE_DEVICES_DTYPE),
                   xu.pod_records([{0: 2000, 1: 4 * xu.GiB}], 0xDF0000), xu.ext_records(gpu=[{}]), xu.ext_args(),
                   enabled=xu.FIT | abi.GS_ENABLE_NUMA_FILTER | abi.GS_ENABLE_NUMA_SCORE, numa_nodes=numa_nodes)
    e2 = Engine(case.cfg())
    case.load(e2)
    e2.upsert_aux_devices(du.AuxTable([du.FILLER] * 4).records())
    with pytest.raises(GpuScoreError, match="while node 2 has a NUMA topology policy"):
        e2.schedule_ext_aux(case.pods, case.ext, [aux])
    out, eo, ao = e2.schedule_ext_aux(case.pods, case.ext, [du.aux_pod()])    # without the request the pod goes through
    assert int(out["node"][0]) >= 0 and e2.mirror_check() == 0
