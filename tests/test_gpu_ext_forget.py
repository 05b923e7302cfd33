"""gs_pods_forget of pods gs_schedule_ext placed: the DeviceShare and Reservation Unreserves and the scalar part of
NodeInfo.RemovePod on the host state, and the lazy uploads that carry them to the HBM images the next gs_schedule_ext
reads (the Device rows, and the mirror rows with the unmatched-reservation restore). The reference side is the CPU
oracle with tests/ext_forget_util.oracle_forget_ext in place of the forget. Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from koordinator_amd import abi, config, synth
from oracle import coscheduling as oc
from oracle import oracle as orc
from tests import ext_forget_util as xf
from tests import test_gang_ext as tg

pytestmark = pytest.mark.gpu

GiB = 1 << 30
GPU_MEM = 80 * GiB
RA = abi.GPU_NAMES["koordinator.sh/gpu-memory-ratio"]
GPU_NODE, RSV_NODE = 1, 2
RSV_UID, OWNER = 0xA11C, 7


def hip_engine(cfg):
    from koordinator_amd.engine import Engine
    cfg.device = 0
    return Engine(cfg)


def tiny_cluster(used_ratio, n_pods=6):
    """4 idle nodes without metrics; node GPU_NODE has one GPU per entry of used_ratio (minor g used that much, by a
    registered `used`) and 4 of extended resource 0, one of them requested; every pod asks 1 cpu / 1 GiB."""
    c = synth.make_cluster(4, n_pods, config_id=41)
    c.nodes["requested"][:] = 0
    c.nodes["nonzero_requested"][:] = 0
    c.nodes["pod_count"][:] = 0
    c.nodes["custom_flags"][:] = 0
    c.nodes["raw_allocatable_mask"][:] = 0
    c.metrics = np.zeros(4, abi.METRIC_DTYPE)
    c.pod_metrics = np.zeros(0, abi.POD_METRIC_DTYPE)
    c.pm_offsets = np.zeros(5, np.uint32)
    c.assigned_node, c.assigned_pods, c.assigned_ts = c.assigned_node[:0], c.assigned_pods[:0], c.assigned_ts[:0]
    p = c.pods
    p["requests"][:] = 0
    p["requests"][:, 0], p["requests"][:, 1] = 1000, GiB
    p["limits"][:] = p["requests"]
    p["nonzero_requests"][:, 0], p["nonzero_requests"][:, 1] = 1000, GiB
    p["request_mask"][:] = 3
    p["priority_class"][:] = abi.GS_PRIO_PROD
    devs = np.zeros(4, abi.NODE_DEVICES_DTYPE)
    G = len(used_ratio)
    d = devs[GPU_NODE]
    d["has_device"], d["num_gpus"] = 1, G
    for g, ur in enumerate(used_ratio):
        gg = d["gpus"][g]
        gg["minor"], gg["has_info"], gg["numa_node"] = g, 1, -1
        gg["total"] = (100, 100, GPU_MEM)
        gg["used"] = (ur, ur, ur * GPU_MEM // 100)
    tot = sum(used_ratio)
    d["allocatable"] = (G, 100 * G, 100 * G, GPU_MEM * G, 100 * G)
    d["requested"] = (sum(u == 100 for u in used_ratio), tot, tot, tot * GPU_MEM // 100, tot)
    d["xres_allocatable"][0], d["xres_requested"][0] = 4, 1
    c.ext = {"devices": devs, "reservations": np.zeros(0, abi.RESERVATION_DTYPE),
             "pod_ext": np.zeros(n_pods, abi.POD_EXT_DTYPE)}
    return c


def gpu_pod(c, k, ratio, xres=True):
    x = c.ext["pod_ext"][k]
    x["gpu_request_mask"] = 1 << RA
    x["gpu_requests"][RA] = ratio
    if xres:
        x["xres_request_mask"] = 1
        x["xres_requests"][0] = 1


def owner_pod(c, k, required=1):
    x = c.ext["pod_ext"][k]
    x["reservation_owner"], x["reservation_required"] = OWNER, required


def add_reservation(c, policy="Default", allocate_once=0, assigned=0):
    """One reservation of 4 cpu / 8 GiB on RSV_NODE; `assigned` pods of 1 cpu / 1 GiB already in it. NodeInfo holds the
    reserve pod and the assigned pods."""
    r = np.zeros(1, abi.RESERVATION_DTYPE)
    r["uid"], r["owner_key"], r["node"] = RSV_UID, OWNER, RSV_NODE
    r["allocate_policy"] = abi.RSV_POLICY[policy]
    r["available"], r["allocate_once"], r["assigned_pods"] = 1, allocate_once, assigned
    r["allocatable"][0, 0], r["allocatable"][0, 1] = 4000, 8 * GiB
    r["allocatable_mask"] = r["resource_names_mask"] = 3
    if assigned:
        r["allocated"][0, 0], r["allocated"][0, 1] = 1000 * assigned, GiB * assigned
        r["allocated_mask"] = 3
    n = c.nodes[RSV_NODE]
    for s in (0, 1):
        n["requested"][s] += r["allocatable"][0, s] + r["allocated"][0, s]
        n["nonzero_requested"][s] += r["allocatable"][0, s] + r["allocated"][0, s]
    n["pod_count"] += 1 + assigned
    c.ext["reservations"] = r
    return r


def make_pair(c, make_engine, enabled=abi.GS_ENABLE_LA_FIT):
    """The engine under test and the reference (an OracleExt) with the same state."""
    cfg = config.make_config(c.num_nodes, enabled=enabled)
    e, o = make_engine(cfg), orc.Oracle(cfg)
    for x in (e, o):
        synth.load_into(x, c)
        synth.load_ext_into(x, c, orc.ext_args_default())
    return e, xf.OracleExt(o, c.pods, c.ext["pod_ext"])


def both_schedule(c, e, ref, ks, seq0=0):
    """schedule_ext of pods ks on both sides; asserts equal results; returns (placements, ext placements)."""
    ks = np.atleast_1d(ks)
    seq = seq0 + np.arange(len(ks), dtype=np.uint64)
    got, gx = e.schedule_ext(c.pods[ks], c.ext["pod_ext"][ks], seq)
    want, wx = ref.schedule_ext(c.pods[ks], c.ext["pod_ext"][ks], seq)
    for f in ("node", "feasible"):
        assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
    placed = want["node"] >= 0
    for f in ("score", "ties"):
        assert np.array_equal(got[f][placed], want[f][placed]), f
    assert gx.tobytes() == wx.tobytes(), (gx, wx)
    return got, gx


def both_forget(c, e, ref, nodes, ks):
    ks = np.atleast_1d(ks)
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), np.uint32)
    e.forget(nodes, c.pods[ks])
    ref.forget(nodes, c.pods[ks])


def device_bytes(e, n=4):
    return [e.devices(i).tobytes() for i in range(n)]


def same_reservation(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        assert a.tobytes() == b.tobytes(), (a, b)


DEVICE_CASES = {   # used ratio of each minor, the pod's gpu-memory-ratio, the minors it must take
    "share": ((50, 100), 50, 0b01),
    "whole": ((50, 0, 100), 100, 0b010),
    "multi": ((50, 0, 0, 100), 200, 0b0110),
}


def run_forget_restores_device_state(make_engine, case):
    used, ratio, minors = DEVICE_CASES[case]
    c = tiny_cluster(used)
    gpu_pod(c, 0, ratio)
    gpu_pod(c, 1, ratio)
    e, ref = make_pair(c, make_engine)
    # the reference never sees pod 0: the probe's placement on it is what a restored state must give
    before = device_bytes(e)
    uid = int(c.pods["uid"][0])
    assert e.ext_reserved(uid) is None
    got, gx = e.schedule_ext(c.pods[:1], c.ext["pod_ext"][:1], np.array([0], np.uint64))
    assert got["node"][0] == GPU_NODE and gx["gpu_minor_mask"][0] == minors and gx["gpu_count"][0] == bin(minors).count("1")
    rec = e.ext_reserved(uid)
    assert rec is not None and rec[0] == GPU_NODE
    for f in ("reservation_uid", "gpu_minor_mask", "gpu_count", "gpu_per_instance"):
        assert np.array_equal(rec[1][f], gx[f][0]), f
    for f in ("deviceshare_score", "reservation_score", "fail_code"):
        assert rec[1][f] == 0, f
    d = e.devices(GPU_NODE)
    assert d.tobytes() != before[GPU_NODE] and d["xres_requested"][0] == 2 and d["requested"][RA] == sum(used) + ratio
    e.forget(np.array([GPU_NODE], np.uint32), c.pods[:1])
    assert device_bytes(e) == before
    assert e.ext_reserved(uid) is None
    assert e.mirror_check() == 0
    got, gx = both_schedule(c, e, ref, 1, seq0=0)
    assert got["node"][0] == GPU_NODE and gx["gpu_minor_mask"][0] == minors
    assert device_bytes(e) == device_bytes(ref)
    assert e.mirror_check() == 0


@pytest.mark.parametrize("case", list(DEVICE_CASES))
def test_forget_restores_device_state(case):
    run_forget_restores_device_state(hip_engine, case)


def run_forget_restores_reservation(make_engine, case):
    c = tiny_cluster((0, 0))
    r0 = add_reservation(c, policy="Restricted" if case == "restricted" else "Default",
                         allocate_once=int(case == "allocate_once"), assigned=0 if case == "allocate_once" else 1)[0]
    for k in (0, 1, 2):
        owner_pod(c, k)
    e, ref = make_pair(c, make_engine)
    uid = int(c.pods["uid"][0])
    got, gx = both_schedule(c, e, ref, 0, seq0=0)
    assert got["node"][0] == RSV_NODE and gx["reservation_uid"][0] == RSV_UID
    rec = e.ext_reserved(uid)
    assert rec is not None and rec[0] == RSV_NODE and rec[1]["reservation_uid"] == RSV_UID and rec[1]["gpu_count"] == 0
    r1 = e.reservation(RSV_UID)
    same_reservation(r1, ref.reservation(RSV_UID))
    assert r1["assigned_pods"] == r0["assigned_pods"] + 1
    assert list(r1["allocated"][:2]) == [r0["allocated"][0] + 1000, r0["allocated"][1] + GiB]
    if case == "allocate_once":   # used: the same owner's next pod does not get it (and requires one: unschedulable)
        got, gx = both_schedule(c, e, ref, 1, seq0=1)
        assert got["node"][0] == -1 and gx["reservation_uid"][0] == 0
    both_forget(c, e, ref, RSV_NODE, 0)
    assert e.ext_reserved(uid) is None
    r2 = e.reservation(RSV_UID)
    same_reservation(r2, ref.reservation(RSV_UID))
    assert r2["assigned_pods"] == r0["assigned_pods"]
    assert list(r2["allocated"][:2]) == list(r0["allocated"][:2])
    assert int(r2["allocated_mask"]) & int(r0["allocated_mask"]) == int(r0["allocated_mask"])
    assert int(r2["allocated_mask"]) == 3   # the subtraction keeps the keys the pod's requests brought
    assert e.mirror_check() == 0
    # the same owner's next pod gets the reservation again; a plain pod sees the restored row
    got, gx = both_schedule(c, e, ref, 2, seq0=2)
    assert got["node"][0] == RSV_NODE and gx["reservation_uid"][0] == RSV_UID
    both_schedule(c, e, ref, [3, 4], seq0=3)
    same_reservation(e.reservation(RSV_UID), ref.reservation(RSV_UID))
    assert e.mirror_check() == 0


@pytest.mark.parametrize("case", ["default", "restricted", "allocate_once"])
def test_forget_restores_reservation(case):
    run_forget_restores_reservation(hip_engine, case)


def _gpu_and_owner_cluster():
    """pods 0 and 2: a whole GPU each; pod 1: assumed into the reservation; pods 3-5: a GPU probe, an owner probe, a
    plain probe"""
    c = tiny_cluster((50, 0, 0, 0))
    add_reservation(c, assigned=1)
    for k in (0, 2, 3):
        gpu_pod(c, k, 100)
    for k in (1, 4):
        owner_pod(c, k)
    return c


def run_forget_floors_and_vanished_state(make_engine):
    # (a) the Device row upserted with used = 0 between Reserve and forget: the subtraction floors at 0
    c = _gpu_and_owner_cluster()
    e, ref = make_pair(c, make_engine)
    both_schedule(c, e, ref, [0, 1, 2])
    row = np.zeros(1, abi.NODE_DEVICES_DTYPE)
    row[0] = e.devices(GPU_NODE)
    row["gpus"]["used"][:] = 0
    for x in (e, ref):
        x.upsert_devices(row, idx=[GPU_NODE])
    both_forget(c, e, ref, [GPU_NODE, GPU_NODE], [0, 2])
    d = e.devices(GPU_NODE)
    assert (d["gpus"]["used"] == 0).all() and d["xres_requested"][0] == 1 and d["requested"][RA] == 50
    assert device_bytes(e) == device_bytes(ref) and e.mirror_check() == 0
    both_schedule(c, e, ref, [3, 4, 5], seq0=3)
    # (b) the recorded minor dropped from the row: skipped, the other minors untouched
    c = _gpu_and_owner_cluster()
    e, ref = make_pair(c, make_engine)
    got, gx = both_schedule(c, e, ref, [0, 1, 2])
    taken = int(gx["gpu_minor_mask"][0])
    row = np.zeros(1, abi.NODE_DEVICES_DTYPE)
    row[0] = e.devices(GPU_NODE)
    keep = [g for g in range(4) if not taken >> int(row["gpus"]["minor"][0, g]) & 1]
    assert len(keep) == 3
    gpus = row["gpus"][0, keep].copy()
    row["gpus"][0] = 0
    row["gpus"][0, :3] = gpus
    row["num_gpus"] = 3
    for x in (e, ref):
        x.upsert_devices(row, idx=[GPU_NODE])
    both_forget(c, e, ref, GPU_NODE, 0)
    d = e.devices(GPU_NODE)
    assert d["num_gpus"] == 3 and d["gpus"][:3].tobytes() == gpus.tobytes()
    assert device_bytes(e) == device_bytes(ref) and e.mirror_check() == 0
    both_schedule(c, e, ref, [3, 4, 5], seq0=3)
    # (c) the reservation removed: GS_OK, NodeInfo and the devices still undone
    c = _gpu_and_owner_cluster()
    e, ref = make_pair(c, make_engine)
    before = device_bytes(e)
    got, gx = both_schedule(c, e, ref, [0, 1, 2])
    assert gx["reservation_uid"][1] == RSV_UID
    for x in (e, ref):
        x.remove_reservations([RSV_UID])
    both_forget(c, e, ref, [GPU_NODE, RSV_NODE, GPU_NODE], [0, 1, 2])
    assert e.reservation(RSV_UID) is None and device_bytes(e) == before
    assert all(e.ext_reserved(int(u)) is None for u in c.pods["uid"][:3])
    assert e.mirror_check() == 0
    c.ext["pod_ext"][4]["reservation_required"] = 0   # (no reservation is left to require)
    both_schedule(c, e, ref, [3, 4, 5], seq0=3)
    # (d) the reservation upserted with allocated = 0 and no assigned pods: both stay 0
    c = _gpu_and_owner_cluster()
    e, ref = make_pair(c, make_engine)
    both_schedule(c, e, ref, [0, 1, 2])
    r = c.ext["reservations"].copy()
    r["allocated"][:] = 0
    r["allocated_mask"] = 0
    r["assigned_pods"] = 0
    for x in (e, ref):
        x.upsert_reservations(r)
    both_forget(c, e, ref, RSV_NODE, 1)
    r2 = e.reservation(RSV_UID)
    same_reservation(r2, ref.reservation(RSV_UID))
    assert r2["assigned_pods"] == 0 and (r2["allocated"] == 0).all()
    assert e.mirror_check() == 0
    both_schedule(c, e, ref, [3, 4, 5], seq0=3)


def test_forget_floors_and_vanished_state():
    run_forget_floors_and_vanished_state(hip_engine)


def run_forget_wrong_node_is_einval_and_atomic(make_engine):
    c = _gpu_and_owner_cluster()
    e, ref = make_pair(c, make_engine)
    got, gx = both_schedule(c, e, ref, [0, 1, 2])
    assert list(got["node"]) == [GPU_NODE, RSV_NODE, GPU_NODE]
    devs, rsv = device_bytes(e), e.reservation(RSV_UID).tobytes()
    recs = [e.ext_reserved(int(u)) for u in c.pods["uid"][:3]]
    assert all(x is not None for x in recs)
    for wrong in (0, c.num_nodes):   # another node, then no node at all
        with pytest.raises(Exception, match=f"rc={abi.GS_EINVAL}"):
            e.forget(np.array([GPU_NODE, wrong, GPU_NODE], np.uint32), c.pods[:3])
        assert device_bytes(e) == devs and e.reservation(RSV_UID).tobytes() == rsv
        for u, x in zip(c.pods["uid"][:3], recs):
            y = e.ext_reserved(int(u))
            assert y is not None and y[0] == x[0] and y[1].tobytes() == x[1].tobytes()
        assert e.mirror_check() == 0
    # the state is whole: the right call undoes all three, as on the reference
    both_forget(c, e, ref, [GPU_NODE, RSV_NODE, GPU_NODE], [0, 1, 2])
    assert device_bytes(e) == device_bytes(ref)
    same_reservation(e.reservation(RSV_UID), ref.reservation(RSV_UID))
    both_schedule(c, e, ref, [3, 4, 5], seq0=3)
    assert e.mirror_check() == 0


def test_forget_wrong_node_is_einval_and_atomic():
    run_forget_wrong_node_is_einval_and_atomic(hip_engine)


def run_forget_interleaved(make_engine, numa):
    c = synth.make_cluster(600, 300, config_id=22 if numa else 21)
    if numa:
        synth.make_numa(c, numa_policy_pct=40, cpuset_pod_pct=10)
    synth.make_ext(c, gpu_node_pct=50, gpu_pod_pct=40, rsv_node_pct=40, owners=10, owner_pod_pct=40, required_pct=10)
    e, ref = make_pair(c, make_engine, enabled=abi.GS_ENABLE_ALL if numa else abi.GS_ENABLE_LA_FIT)
    P = len(c.pods)
    seq = np.arange(P, dtype=np.uint64)
    ext = c.ext["pod_ext"]
    for k in range(3):
        sl = slice(k * P // 3, (k + 1) * P // 3)
        got, gx = e.schedule_ext(c.pods[sl], ext[sl], seq[sl])
        want, wx = ref.schedule_ext(c.pods[sl], ext[sl], seq[sl])
        for f in ("node", "feasible"):
            bad = np.nonzero(got[f] != want[f])[0]
            assert not len(bad), f"chunk {k}: {f} differs at pods {bad[:10]}"
        placed = want["node"] >= 0
        for f in ("score", "ties"):
            assert np.array_equal(got[f][placed], want[f][placed]), (k, f)
        for f in ("reservation_uid", "gpu_minor_mask", "gpu_count", "gpu_per_instance", "deviceshare_score",
                  "reservation_score", "fail_code"):
            bad = np.nonzero((gx[f] != wx[f]).reshape(len(gx), -1).any(axis=1))[0]
            assert not len(bad), f"chunk {k}: ext {f} differs at pods {bad[:10]}"
        drop = np.flatnonzero(placed)[::3]   # every third placed pod of the chunk is forgotten
        nodes = want["node"][drop].astype(np.uint32)
        e.forget(nodes, c.pods[sl][drop])
        ref.forget(nodes, c.pods[sl][drop])
        for u in c.pods["uid"][sl][drop]:
            assert e.ext_reserved(int(u)) is None
    xf.same_ext_state(c, e, ref)
    assert e.mirror_check() == 0
    # the oracle alone gives 34 / 36 / 24 / 39 (plain) and 38 / 33 / 26 / 28 (numa)
    print("forgotten GPU pods", len(ref.forgot_gpu), "reservation pods", len(ref.forgot_rsv),
          "reused minors", ref.reused_gpu, "reused reservations", ref.reused_rsv)
    assert len(ref.forgot_gpu) >= 20 and len(ref.forgot_rsv) >= 20
    assert ref.reused_gpu >= 10 and ref.reused_rsv >= 10


@pytest.mark.parametrize("numa", [False, True], ids=["plain", "numa"])
def test_forget_interleaved_matches_oracle(numa):
    run_forget_interleaved(hip_engine, numa)


def test_gangs_with_extension_pods_hip_engine():
    """tests/test_gang_ext.py's first workload with the HIP engine under the batched driver."""
    c, pgs, gang_ids = tg.ext_gang_workload(5)

    def make(cfg):
        e = hip_engine(cfg)
        synth.load_into(e, c)
        synth.load_ext_into(e, c, orc.ext_args_default())
        return e
    e, ref, got, gres, want, wres = tg.run_ext_pair(make, c, pgs, gang_ids)
    tg.check_ext_pair(c, e, ref, got, gres, want, wres)
    tg.forget_floors(ref, wres, rejected=10, gpu=5, rsv=3)
    assert (wres["state"] == oc.ST_REJECTED).sum() >= 10
    assert e.mirror_check() == 0
