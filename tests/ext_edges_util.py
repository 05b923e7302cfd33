"""Input builders for the extension path (gs_schedule_ext: koordinator_amd/csrc/gs_ext.hip, ext_schedule_one and
ext_device_reserve in gs_engine.cpp) at its request, device, reservation and select edges, and a plain integer
restatement of the reference's arithmetic.

Every input is a Case: nodes, Device objects, reservations, pods and plugin args, loaded into an Engine and an Oracle
alike. The per-node view of a pod (Engine.ext_rows / Oracle.ext_rows) shows every node's Filter verdict and raw scores,
so a pairs cluster checks every (pod, node) pair at once and leaves no state behind.

Lines of gs_ext.hip each family is aimed at:

* ds_case(strategy, weights) — the DeviceShare pairs cluster (DS_NODES x DS_PODS, no NUMA):
  - no Device object with / without GPU-name allocatable: fit_names_ok (:61-65) and eval_device's early pass (:78);
  - num_gpus 0, every GPU without info, every GPU zero-total, a zero-total first GPU, a 40 GiB first GPU among 80 GiB
    ones: gpu_desired's search for the first healthy GPU (:31-36) and the candidate loop (:88-94);
  - one GPU, eight GPUs, minors 5 / 0 / 31 out of order, has_info gaps: the candidate sums of scoreNode (:91, :98-106);
  - every GPU fully used (all_zero, :84-85), a GPU free in one key only and used above total (:92, dev_image's floor);
  - free equal to the per-instance request on every key and one short on each key in turn: fits_inst (:53-57);
  - 100 GiB totals with free ratio 28 and 27 for the 29 / 57 / 58 GiB requests: memoryBytesToRatio's float64 floor (:38);
  - a memory total 100 does not divide: memoryRatioToBytes' floor (:39);
  - exactly `count` and `count - 1` fitting GPUs: the multi-device split (:42-46) and `ok_n < count` (:96);
  - GPU-name Fit free exact, one short and negative, with and without fit_ignored_gpu_names (:61-65);
  - device_weights (0, 1, 0), (1, 1, 1), (3, 0, 2): the weighted sum and the truncating ns / ws of scoreNode (:98-106);
* ds_mem0_case() — a memory total of 0 beside core and ratio totals, ratio requests only: a byte request there divides
  by zero in the reference's memoryBytesToRatio (devicehandler_gpu.go:96), so none is issued;
* policy_case() — NUMA-policy nodes with 1-4 zones, the GPUs on one zone, split over the zones, without topology and
  with has_info gaps, counts 1, 2, 4 and 8: gpu_hint_word (:134-168), on_aff (:69-71) and ext_numa_kernel (:224-252);
* rsv_case() / rsv_case(fit_filter=False) / rsv_wide_case(nrec) — reservations: fits_node with slots 3-6 and the
  pod-count term (:171-183; the term decides only with Fit's own Filter off), reservation_fits over Default, Aligned and
  Restricted with an exact and a short remainder and a disjoint names mask (:186-197), score_reservation with req > alloc,
  a zero allocatable entry and allocated above allocatable (:202-211), nomination by order and by score with equal scores
  (:329-346), 1, 2 and 8 reservations on a node, and 255 / 256 / 257 / 600 matched records for the `k += SEL_BLOCK`
  stride and the equal-order tie of ext_matched_kernel's reduction (:367-387);
* select_case(n, shape) — identical nodes, ties on chunk and block boundaries, in a partial last block and on the last
  node alone: the three select passes (:421-572), `per > 1` of the last block's scan (:516-541) at 262145 nodes;
* scoring variants (variant_args): plugin weights default and coprime, each plugin bit alone, all-zero raw DeviceShare
  scores (MDS == 0, :464), inexact 100 * ds / MDS, and PreScore's preferred node (raw 1000, the others 100 * r / 1000).

py_* is an integer restatement written from the reference's Go text (deviceshare/utils.go ConvertDeviceRequest,
devicehandler_gpu.go CalcDesiredRequestsAndCount, device_allocator.go defaultAllocateDevices, scoring.go scoreNode,
reservation/scoring.go scoreReservation, [upstream] DefaultNormalizeScore). It is held against the oracle in
tests/test_ext_edges.py; it is never the expected value of a GPU test. The oracle's results are cached, computed once.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from koordinator_amd import abi, config
from oracle import oracle as orc
from tests import numa_edges_util as nu

GiB = 1 << 30
NV, KG, CO, ME, RA = (abi.GPU_NAMES[k] for k in ("nvidia.com/gpu", "koordinator.sh/gpu", "koordinator.sh/gpu-core",
                                                  "koordinator.sh/gpu-memory", "koordinator.sh/gpu-memory-ratio"))
FIT = abi.GS_ENABLE_FIT_FILTER | abi.GS_ENABLE_FIT_SCORE
SEQS = tuple(range(64))
ROW_KEYS = abi.EXT_ROW_KEYS + ("nominated_uid",)
RES_KEYS = abi.EXT_ROWS_RESULT_KEYS
WEIGHTS = ((0, 1, 0), (1, 1, 1), (3, 0, 2))
STRATEGIES = ("LeastAllocated", "MostAllocated")


def ext_args(strategy="LeastAllocated", weights=(0, 1, 0), w_ds=None, w_rs=None, enabled=None, ignored=0):
    a = orc.ext_args_default()
    a.device_scoring_type = abi.GS_SCORING_MOST_ALLOCATED if strategy == "MostAllocated" else abi.GS_SCORING_LEAST_ALLOCATED
    for r in range(3):
        a.device_weights[r] = weights[r]
    if w_ds is not None:
        a.weight_deviceshare = w_ds
    if w_rs is not None:
        a.weight_reservation = w_rs
    if enabled is not None:
        a.enabled = enabled
    a.fit_ignored_gpu_names = ignored
    return a


def copy_args(a) -> abi.GsExtArgs:
    return abi.GsExtArgs.from_buffer_copy(bytes(a))


# the scoring variants of a case: (name, changes to its args)
VARIANTS = (("default", {}), ("coprime", {"w_ds": 3, "w_rs": 7}), ("ds-only", {"enabled": abi.GS_EXT_DEVICESHARE}),
            ("rs-only", {"enabled": abi.GS_EXT_RESERVATION}))


def variant_args(a, changes) -> abi.GsExtArgs:
    b = copy_args(a)
    if "w_ds" in changes:
        b.weight_deviceshare = changes["w_ds"]
    if "w_rs" in changes:
        b.weight_reservation = changes["w_rs"]
    if "enabled" in changes:
        b.enabled = changes["enabled"]
    return b


@dataclass
class Case:
    name: str
    nodes: np.ndarray                      # NODE_DTYPE
    devices: np.ndarray                    # NODE_DEVICES_DTYPE
    pods: np.ndarray                       # POD_DTYPE
    ext: np.ndarray                        # POD_EXT_DTYPE
    args: abi.GsExtArgs
    reservations: np.ndarray = field(default_factory=lambda: np.zeros(0, abi.RESERVATION_DTYPE))
    enabled: int = FIT
    numa_nodes: tuple | None = None        # numa_edges_util.Node per node (policy_case): loaded with nu.load
    node_names: tuple = ()
    pod_names: tuple = ()

    @property
    def n(self) -> int:
        return len(self.nodes)

    def cfg(self):
        return config.make_config(self.n, enabled=self.enabled)

    def load(self, e, args=None) -> None:
        if self.numa_nodes is not None:
            nu.load(e, self.numa_nodes)
        else:
            e.set_now(0)
            e.upsert_nodes(self.nodes)
            e.upsert_metrics(np.zeros(self.n, abi.METRIC_DTYPE))
        e.ext_configure(self.args if args is None else args)
        e.upsert_devices(self.devices)
        if len(self.reservations):
            e.upsert_reservations(self.reservations)

    def oracle(self, args=None):
        o = orc.Oracle(self.cfg())
        self.load(o, args)
        return o


def base_nodes(n, cpu=64000, mem=256 * GiB, pods=110) -> np.ndarray:
    """n identical empty nodes; slots 3-6 (batch / mid cpu and memory) are allocatable too"""
    recs = np.zeros(n, abi.NODE_DTYPE)
    recs["allocatable"][:, 0] = cpu
    recs["allocatable"][:, 1] = mem
    recs["allocatable"][:, 2] = 500 * GiB
    recs["allocatable"][:, 3] = recs["allocatable"][:, 5] = 32000
    recs["allocatable"][:, 4] = recs["allocatable"][:, 6] = 128 * GiB
    recs["allowed_pod_number"] = pods
    recs["custom_agg_type"] = abi.GS_AGG_NONE
    return recs


def pod_records(reqs, uid0) -> np.ndarray:
    """reqs: one {slot: value} per pod"""
    out = np.zeros(len(reqs), abi.POD_DTYPE)
    for k, rq in enumerate(reqs):
        mask = 0
        for s, v in rq.items():
            out[k]["requests"][s] = out[k]["limits"][s] = v
            mask |= 1 << s
        out[k]["nonzero_requests"][0] = rq[0] if 0 in rq else 100
        out[k]["nonzero_requests"][1] = rq[1] if 1 in rq else 200 << 20
        out[k]["request_mask"] = mask
        out[k]["priority_class"] = abi.GS_PRIO_PROD
        out[k]["qos_class"] = abi.GS_QOS_LS
        out[k]["uid"] = uid0 + k
        out[k]["name_key"] = uid0 + k
    return out


def ext_records(gpu=(), owner=(), required=()) -> np.ndarray:
    """gpu: one {GPU name: value} per pod (a key with value 0 stays in the mask)"""
    n = max(len(gpu), len(owner))
    out = np.zeros(n, abi.POD_EXT_DTYPE)
    for k in range(n):
        for name, v in (gpu[k] if k < len(gpu) else {}).items():
            out[k]["gpu_requests"][name] = v
            out[k]["gpu_request_mask"] |= 1 << name
        out[k]["reservation_owner"] = owner[k] if k < len(owner) else 0
        out[k]["reservation_required"] = required[k] if k < len(required) else 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Device objects

FREE80 = ((100, 100, 80 * GiB), (0, 0, 0))
BIG_ALLOC = (64, 6400, 6400, 1 << 45, 6400)


def gpu(total=(100, 100, 80 * GiB), used=(0, 0, 0), minor=None, info=1, numa=-1):
    return {"total": total, "used": used, "minor": minor, "info": info, "numa": numa}


def used_pct(p, mem=80 * GiB):
    return gpu((100, 100, mem), (p, p, p * mem // 100))


def device(gpus, has_device=1, alloc=BIG_ALLOC, requested=(0, 0, 0, 0, 0)) -> np.ndarray:
    d = np.zeros(1, abi.NODE_DEVICES_DTYPE)[0]
    d["has_device"] = has_device
    d["num_gpus"] = len(gpus)
    for k, g in enumerate(gpus):
        x = d["gpus"][k]
        x["minor"] = k if g["minor"] is None else g["minor"]
        x["has_info"] = g["info"]
        x["numa_node"] = g["numa"]
        x["total"] = g["total"]
        x["used"] = g["used"]
    d["allocatable"] = alloc
    d["requested"] = requested
    return d


def _fit_alloc(name, free):
    """GPU-name allocatable / requested whose free of `name` is `free` (the other names stay roomy)"""
    req = [0] * 5
    req[name] = BIG_ALLOC[name] - free
    return BIG_ALLOC, tuple(req)


def ds_nodes():
    """(name, gs_node_devices) of the pairs cluster"""
    G = 80 * GiB
    H = 100 * GiB
    half = (50, 50, 40 * GiB)
    out = [
        ("nodev-noalloc", device([], has_device=0, alloc=(0, 0, 0, 0, 0))),
        ("nodev-alloc", device([], has_device=0)),
        ("gpus0", device([])),
        ("noinfo", device([gpu(info=0) for _ in range(4)])),
        ("zerotot", device([gpu(total=(0, 0, 0)) for _ in range(4)])),
        ("first-zero", device([gpu(total=(0, 0, 0))] + [gpu() for _ in range(3)])),
        ("first-40", device([gpu(total=(100, 100, 40 * GiB))] + [gpu() for _ in range(3)])),
        ("one", device([gpu()])),
        ("eight", device([gpu() for _ in range(8)])),
        ("minors", device([used_pct(25) | {"minor": 5}, used_pct(0) | {"minor": 0}, used_pct(60) | {"minor": 31}])),
        ("gaps", device([gpu(info=k % 2 == 0) for k in range(8)])),
        ("gaps-used", device([used_pct(0 if k % 2 else 75) | {"info": int(k % 2 == 0)} for k in range(6)])),
        ("full", device([used_pct(100) for _ in range(4)])),
        ("onekey", device([gpu(used=(0, 100, G)), used_pct(100), used_pct(100)])),
        ("over", device([gpu(used=(250, 120, 3 * G)), gpu(used=(130, 10, G // 10)), used_pct(40)])),
        ("exact", device([gpu(used=half) for _ in range(4)])),
        ("short-core", device([gpu(used=(51, 50, 40 * GiB)) for _ in range(4)])),
        ("short-ratio", device([gpu(used=(50, 51, 40 * GiB)) for _ in range(4)])),
        ("short-mem", device([gpu(used=(50, 50, 40 * GiB + 1)) for _ in range(4)])),
        ("t100", device([gpu(total=(100, 100, H)) for _ in range(4)])),
        ("t100-r28", device([gpu(total=(100, 100, H), used=(0, 72, 42 * GiB)) for _ in range(2)])),
        ("t100-r27", device([gpu(total=(100, 100, H), used=(0, 73, 42 * GiB)) for _ in range(2)])),
        ("t100-r56", device([gpu(total=(100, 100, H), used=(0, 44, 42 * GiB)) for _ in range(2)])),
        ("t100-r55", device([gpu(total=(100, 100, H), used=(0, 45, 42 * GiB)) for _ in range(2)])),
        ("odd-total", device([gpu(total=(100, 100, G + 7), used=(30, 30, 24 * GiB + 3)) for _ in range(3)])),
        ("odd-total-free", device([gpu(total=(97, 100, G + 33)) for _ in range(2)])),
        ("count2", device([gpu(), gpu()] + [used_pct(10) for _ in range(6)])),
        ("count1", device([gpu()] + [used_pct(10) for _ in range(7)])),
        ("count7", device([gpu() for _ in range(7)] + [gpu(used=(1, 0, 0))])),
        ("fit-exact", device([gpu() for _ in range(4)], requested=_fit_alloc(KG, 50)[1])),
        ("fit-short", device([gpu() for _ in range(4)], requested=_fit_alloc(KG, 49)[1])),
        ("fit-neg", device([gpu() for _ in range(4)], requested=_fit_alloc(KG, -1)[1])),
        ("fit-nv-exact", device([gpu() for _ in range(8)], requested=_fit_alloc(NV, 2)[1])),
        ("fit-nv-short", device([gpu() for _ in range(8)], requested=_fit_alloc(NV, 1)[1])),
    ]
    for p in (10, 25, 33, 60, 90, 99):
        out.append((f"used{p}", device([used_pct(p) for _ in range(4)])))
    out.append(("mixed", device([used_pct(p) for p in (0, 10, 50, 75, 90, 100, 100, 30)])))
    out.append(("mixed-core", device([gpu(used=(c, r, r * G // 100)) for c, r in ((0, 60), (80, 0), (20, 20), (95, 5))])))
    return out


def ds_pods():
    """(name, GPU-name requests) of the pairs cluster"""
    out = [(f"nvidia{v}", {NV: v}) for v in (1, 2, 8, 9)]
    out += [(f"koord{v}", {KG: v}) for v in (1, 50, 100, 200, 800)]
    out += [(f"core{c}-ratio{r}", {CO: c, RA: r}) for c, r in ((1, 1), (100, 100), (50, 300), (30, 200), (50, 50))]
    out += [(f"ratio{v}", {RA: v}) for v in (1, 50, 99, 100, 400)]
    out += [("bytes1", {ME: 1})] + [(f"bytes{v}G", {ME: v * GiB}) for v in (29, 40, 57, 58, 100, 120, 160, 200)]
    out += [("core50-bytes40G", {CO: 50, ME: 40 * GiB}), ("core100-bytes80G", {CO: 100, ME: 80 * GiB}),
            ("core30-bytes160G", {CO: 30, ME: 160 * GiB})]
    out += [("ratio0", {RA: 0}), ("koord0", {KG: 0}), ("core0-ratio0", {CO: 0, RA: 0})]
    out += [("invalid150", {CO: 150, RA: 150}), ("invalid250", {KG: 250})]
    out += [("bad-nv-koord", {NV: 1, KG: 100}), ("bad-core", {CO: 50}), ("bad-core-ratio-mem", {CO: 50, RA: 50, ME: GiB}),
            ("bad-mem-ratio", {ME: GiB, RA: 50}), ("bad-nv-ratio", {NV: 1, RA: 50})]
    out += [("plain", {})]
    return out


def _ds(nodes, pods, name, strategy, weights, ignored=0):
    recs = base_nodes(len(nodes))
    devs = np.array([d for _, d in nodes], abi.NODE_DEVICES_DTYPE)
    reqs = pod_records([{0: 1000, 1: GiB}] * len(pods), 0xD50000)
    ext = ext_records(gpu=[g for _, g in pods])
    return Case(name, recs, devs, reqs, ext, ext_args(strategy, weights, ignored=ignored),
                node_names=tuple(n for n, _ in nodes), pod_names=tuple(n for n, _ in pods))


@functools.lru_cache(maxsize=None)
def ds_case(strategy="LeastAllocated", weights=(0, 1, 0), ignored=0) -> Case:
    return _ds(ds_nodes(), ds_pods(), f"ds-{strategy}-{weights}-{ignored}", strategy, weights, ignored)


IGNORE_KOORD = (1 << KG) | (1 << CO) | (1 << ME) | (1 << RA)


@functools.lru_cache(maxsize=None)
def ds_mem0_case(strategy="LeastAllocated") -> Case:
    nodes = [("mem0", device([gpu(total=(100, 100, 0)) for _ in range(4)])),
             ("mem0-used", device([gpu(total=(100, 100, 0), used=(40, 40, 0)) for _ in range(4)])),
             ("eight", device([gpu() for _ in range(8)]))]
    pods = [(n, g) for n, g in ds_pods() if ME not in g]
    return _ds(nodes, pods, f"ds-mem0-{strategy}", strategy, (1, 1, 1))


# ---------------------------------------------------------------------------------------------------------------------
# NUMA-policy nodes

@functools.lru_cache(maxsize=None)
def policy_case() -> Case:
    """<= 48 NUMA-policy nodes of 1-4 zones; every GPU with a topology sits on one of its node's zones"""
    names, nodes, devs = [], [], []
    zone = (8000, 32 * GiB)
    k = 0
    for nz in (1, 2, 3, 4):
        for policy in nu.POLICIES:
            layouts = {
                "onezone": [nz - 1] * 8,
                "split": [g * nz // 8 for g in range(8)],
                "notopo": [-1] * 8,
                "gaps": [g % nz for g in range(8)],
            }
            for lname, zs in layouts.items():
                if k >= 48:
                    break
                gpus = [gpu(numa=z, info=int(not (lname == "gaps" and g % 3 == 1)),
                            used=(0, 0, 0) if (g + k) % 4 or k % 3 == 0 else (50, 50, 40 * GiB))
                        for g, z in enumerate(zs)]   # (every third node has all its GPUs free: a count of 8 can fit)
                names.append(f"{policy}-{nz}z-{lname}")
                nodes.append(nu.Node(names[-1], policy, (zone,) * nz))
                devs.append(device(gpus))
                k += 1
    gpus = [{KG: 100}, {KG: 200}, {KG: 400}, {KG: 800}, {NV: 1}, {NV: 2}, {NV: 4}, {NV: 8},
            {CO: 50, RA: 50}, {RA: 200}, {ME: 40 * GiB}, {ME: 160 * GiB}, {CO: 100, ME: 320 * GiB}, {KG: 50},
            {RA: 400}, {KG: 300}]
    pods = pod_records([{0: 2000, 1: 4 * GiB}] * len(gpus), 0xD60000)
    recs = np.zeros(len(nodes), abi.NODE_DTYPE)   # (nu.load builds the node records itself)
    return Case("policy", recs, np.array(devs, abi.NODE_DEVICES_DTYPE), pods, ext_records(gpu=gpus),
                ext_args(weights=(1, 1, 1)), enabled=FIT | abi.GS_ENABLE_NUMA_FILTER | abi.GS_ENABLE_NUMA_SCORE,
                numa_nodes=tuple(nodes), node_names=tuple(names), pod_names=tuple(str(g) for g in gpus))


# ---------------------------------------------------------------------------------------------------------------------
# reservations

def rsv(uid, owner, node, alloc, allocated=None, names=None, policy="Default", order=0, once=0, assigned=0, unsched=0,
        allocated_mask=None):
    r = np.zeros(1, abi.RESERVATION_DTYPE)[0]
    r["uid"], r["owner_key"], r["node"] = uid, owner, node
    r["allocate_policy"] = abi.RSV_POLICY[policy]
    r["order"], r["available"], r["unschedulable"], r["allocate_once"], r["assigned_pods"] = order, 1, unsched, once, assigned
    for s, v in alloc.items():
        r["allocatable"][s] = v
        r["allocatable_mask"] |= 1 << s
    for s, v in (allocated or {}).items():
        r["allocated"][s] = v
        r["allocated_mask"] |= 1 << s
    if allocated_mask is not None:
        r["allocated_mask"] = allocated_mask
    r["resource_names_mask"] = r["allocatable_mask"] if names is None else names
    return r


def hold(nodes, rs) -> None:
    """NodeInfo holds every reservation's reserve pod (its requests = Allocatable) and the pods assigned to it"""
    for r in rs:
        i = int(r["node"])
        for s in range(7):
            held = (int(r["allocatable"][s]) if r["allocatable_mask"] >> s & 1 else 0) + \
                   (int(r["allocated"][s]) if r["allocated_mask"] >> s & 1 else 0)
            nodes["requested"][i, s] += held
            if s < 2:
                nodes["nonzero_requested"][i, s] += held
        nodes["pod_count"][i] += 1 + int(r["assigned_pods"])


CM = {0: 4000, 1: 8 * GiB}
# owner keys of the reservation cluster
(O_DEFAULT, O_ALIGNED, O_RESTRICTED, O_SLOTS, O_DISJOINT, O_OVER, O_REQGT, O_ZEROALLOC, O_TWO, O_EIGHT, O_ONCE,
 O_UNSCHED, O_ORDER, O_SCORE, O_EQSCORE, O_ORDER2, O_ORDERBAD, O_PODS, O_NONE, O_GPU, O_Q46) = range(1, 22)
N_RSV = 64


def _rsv_reservations():
    """the reservation cluster's reservations; node k of a scenario is free for it alone where the text says so"""
    rs, uid = [], [0x5000]

    def add(owner, node, alloc=CM, **kw):
        uid[0] += 1
        rs.append(rsv(uid[0], owner, node, alloc, **kw))

    add(O_DEFAULT, 1)
    add(O_ALIGNED, 2, policy="Aligned", allocated={0: 1000, 1: GiB}, assigned=1)
    add(O_RESTRICTED, 3, policy="Restricted", allocated={0: 2000, 1: 2 * GiB}, assigned=1)   # remainder cpu 2000, mem 6 GiB
    slots = {0: 4000, 1: 8 * GiB, 3: 6000, 4: 12 * GiB, 5: 3000, 6: 6 * GiB}
    add(O_SLOTS, 4, alloc=slots, policy="Restricted", allocated={3: 2000, 4: 4 * GiB, 5: 1000}, assigned=1)
    add(O_SLOTS, 5, alloc={3: 6000, 4: 12 * GiB}, policy="Default")
    add(O_SLOTS, 6, alloc=slots, policy="Aligned", allocated={6: 6 * GiB}, assigned=1)
    add(O_DISJOINT, 7, names=1 << 1)                       # names {memory}: disjoint from a cpu-only pod's mask
    add(O_DISJOINT, 8, alloc={4: 8 * GiB}, names=1 << 4)   # names {batch-memory}
    add(O_OVER, 9, allocated={0: 6000, 1: 9 * GiB}, assigned=2)
    add(O_OVER, 10, policy="Restricted", allocated={0: 6000}, assigned=1)
    add(O_REQGT, 11, allocated={0: 2000}, assigned=1)      # a pod of cpu 3000: 5000 > 4000 in slot 0 alone
    add(O_ZEROALLOC, 12, alloc={0: 4000, 1: 0})
    add(O_ZEROALLOC, 13, alloc={0: 0, 1: 0})               # every allocatable entry zero: w == 0
    for k in range(2):
        add(O_TWO, 14, alloc={0: 2000 + 2000 * k, 1: 4 * GiB})
    for k in range(8):
        add(O_EIGHT, 15, alloc={0: 1000 + 500 * k, 1: (1 + k) * GiB}, policy=("Default", "Restricted", "Aligned")[k % 3],
            allocated={0: 100 * k} if k % 2 else None, assigned=k % 2)
    for k in range(2):
        add(O_ONCE, 16, once=1, assigned=1, allocated={0: 1000, 1: GiB})
    for k in range(2):
        add(O_UNSCHED, 17, unsched=1, assigned=k, allocated={0: 1000} if k else None)
    for order, cpu in ((0, 2000), (5, 4000), (3, 8000), (3, 3000)):   # by order: the first of the two with order 3
        add(O_ORDER, 18, alloc={0: cpu, 1: 8 * GiB}, order=order)
    for cpu in (8000, 2000, 4000):                                   # by score: the smallest allocatable scores highest
        add(O_SCORE, 19, alloc={0: cpu, 1: 8 * GiB})
    for k in range(3):                                               # equal scores: the first in uid order
        add(O_EQSCORE, 20, alloc={0: 4000, 1: 8 * GiB})
    add(O_ORDER2, 22, order=7)                                       # equal lowest order on two nodes: the first node
    add(O_ORDER2, 21, order=7)
    add(O_ORDER2, 23, order=9)
    add(O_ORDER2, 24, order=0)
    add(O_ORDERBAD, 25, order=1)                                     # the lowest order on a node without room
    add(O_ORDERBAD, 26, order=2)
    add(O_ORDERBAD, 27, order=0)
    for node in (28, 29, 30):                                        # pod-count edge (see _rsv_nodes)
        add(O_PODS, node)
        add(O_PODS, node, alloc={0: 2000, 1: 4 * GiB})
    for node in (0, 1, 2, 40):                                       # a GPU owner pod nominates none
        add(O_GPU, node)
    q = 1 << 46
    add(O_Q46, 41, alloc={1: q, 4: q}, allocated={1: q - 1}, assigned=1)   # 100 * 1000 * q stays inside int64
    add(O_Q46, 42, alloc={1: q, 4: q}, policy="Restricted", allocated={1: 1, 4: q // 3}, assigned=1)
    return rs


def _rsv_nodes(rs, n=N_RSV):
    nodes = base_nodes(n, mem=(1 << 48))
    nodes["allocatable"][:, 4] = 1 << 48
    hold(nodes, rs)
    # the node of O_ORDERBAD's lowest order has no cpu left beyond the reserve pod (and the pods to come ask more)
    # (the restore takes the reserve pod's 4000 out again: 1000 stay free)
    nodes["requested"][25, 0] = nodes["allocatable"][25, 0] + 4000 - 1000
    nodes["nonzero_requested"][25, 0] = nodes["requested"][25, 0]
    # pod-count edge: 2 matched reservations on each; with p pods on the node the restored NodeInfo holds p - 2 and
    # fitsNode counts p - 4 + 1 against allowed: equal on node 28, one below on 29, one above on 30
    for node, allowed in ((28, 0), (29, 1), (30, -1)):
        p = int(nodes["pod_count"][node])
        nodes["allowed_pod_number"][node] = p - 3 + allowed
    return nodes


def _rsv_pods():
    """(name, requests, owner, required, GPU names)"""
    c2 = {0: 2000, 1: 2 * GiB}
    out = [
        ("default", c2, O_DEFAULT, 0, {}), ("default-req", c2, O_DEFAULT, 1, {}),
        ("aligned", c2, O_ALIGNED, 1, {}),
        ("restricted-eq", {0: 2000, 1: 6 * GiB}, O_RESTRICTED, 1, {}),
        ("restricted-cpu+1", {0: 2001, 1: 6 * GiB}, O_RESTRICTED, 1, {}),
        ("restricted-mem+1", {0: 2000, 1: 6 * GiB + 1}, O_RESTRICTED, 1, {}),
        ("restricted-eq-free", {0: 2000, 1: 6 * GiB}, O_RESTRICTED, 0, {}),
        ("slots", {0: 1000, 1: GiB, 3: 4000, 4: 8 * GiB, 5: 2000, 6: 6 * GiB}, O_SLOTS, 1, {}),
        ("slots+1", {0: 1000, 1: GiB, 3: 4001, 4: 8 * GiB, 5: 2000, 6: 6 * GiB}, O_SLOTS, 1, {}),
        ("slots-batch", {3: 6000, 4: 12 * GiB}, O_SLOTS, 0, {}),
        ("slots-mid", {5: 2000, 6: 1}, O_SLOTS, 1, {}),
        ("disjoint-cpu", {0: 1000}, O_DISJOINT, 1, {}), ("disjoint-mem", {1: GiB}, O_DISJOINT, 1, {}),
        ("disjoint-free", {0: 1000}, O_DISJOINT, 0, {}),
        ("over", c2, O_OVER, 0, {}), ("over-req", c2, O_OVER, 1, {}),
        ("reqgt", {0: 3000, 1: 2 * GiB}, O_REQGT, 0, {}),
        ("zeroalloc", c2, O_ZEROALLOC, 0, {}),
        ("two", c2, O_TWO, 1, {}), ("eight", {0: 1500, 1: 2 * GiB}, O_EIGHT, 1, {}), ("eight-free", c2, O_EIGHT, 0, {}),
        ("once", c2, O_ONCE, 0, {}), ("once-req", c2, O_ONCE, 1, {}), ("unsched-req", c2, O_UNSCHED, 1, {}),
        ("order", c2, O_ORDER, 0, {}), ("score", c2, O_SCORE, 0, {}), ("eqscore", c2, O_EQSCORE, 1, {}),
        ("order2", c2, O_ORDER2, 0, {}), ("orderbad", c2, O_ORDERBAD, 0, {}),
        ("pods", c2, O_PODS, 1, {}), ("pods-free", c2, O_PODS, 0, {}), ("pods-zero", {0: 0}, O_PODS, 1, {}),
        ("none-req", c2, O_NONE, 1, {}), ("none", c2, O_NONE, 0, {}), ("no-owner", c2, 0, 0, {}),
        ("gpu-owner", c2, O_GPU, 0, {KG: 100}), ("gpu-owner-req", c2, O_GPU, 1, {CO: 50, RA: 50}),
        ("q46", {1: 1, 4: (1 << 46) - (1 << 46) // 3}, O_Q46, 1, {}), ("q46+1", {1: 2, 4: 5}, O_Q46, 1, {}),
    ]
    return out


@functools.lru_cache(maxsize=None)
def rsv_case(fit_filter=True) -> Case:
    rs = _rsv_reservations()
    nodes = _rsv_nodes(rs)
    devs = np.zeros(N_RSV, abi.NODE_DEVICES_DTYPE)
    for i in range(0, 48):   # GPUs on most nodes (a GPU owner pod passes Fit's scalars only where a Device object is)
        devs[i] = device([used_pct((7 * i) % 60), gpu(), used_pct((11 * i) % 100), gpu()])
    pods = _rsv_pods()
    recs = pod_records([p[1] for p in pods], 0xD70000)
    ext = ext_records(gpu=[p[4] for p in pods], owner=[p[2] for p in pods], required=[p[3] for p in pods])
    return Case("rsv" if fit_filter else "rsv-nofit", nodes, devs, recs, ext, ext_args(),
                reservations=np.array(rs, abi.RESERVATION_DTYPE),
                enabled=FIT if fit_filter else abi.GS_ENABLE_FIT_SCORE, pod_names=tuple(p[0] for p in pods))


N_WIDE = 640
WIDE_NREC = (255, 256, 257, 600)


@functools.lru_cache(maxsize=None)
def rsv_wide_case(nrec: int) -> Case:
    """one owner with a reservation on each of the first nrec of 640 nodes. Orders: equal lowest (4) on nodes 300, 44,
    261 and 6 where nrec reaches them (44 and 300 fall to one thread of ext_matched_kernel, 6 and 261 to another; the
    lowest node index wins), order 2 on node 250 whose node has no room, and a second owner whose lowest order sits on
    the last record alone"""
    rs = []
    for i in range(nrec):
        order = 4 if i in (300, 44, 261, 6) else 2 if i == 250 else (10 + i % 7 if i % 5 == 0 else 0)
        rs.append(rsv(0x9000 + i, 1, i, {0: 2000 + 100 * (i % 11), 1: 8 * GiB}, order=order,
                      allocated={0: 100 * (i % 9)} if i % 4 == 1 else None, assigned=int(i % 4 == 1)))
        rs.append(rsv(0xA000 + i, 2, i, CM, order=3 if i == nrec - 1 else 0))
    nodes = base_nodes(N_WIDE)
    hold(nodes, rs)
    # (owner 1's restore takes its reserve pod's 2800 out again: 1000 stay free for its pods)
    nodes["requested"][250, 0] = nodes["allocatable"][250, 0] + 2800 - 1000
    nodes["nonzero_requested"][250, 0] = nodes["requested"][250, 0]
    c2 = {0: 2000, 1: 2 * GiB}
    pods = [("wide", c2, 1, 0), ("wide-req", c2, 1, 1), ("wide2", c2, 2, 0), ("wide2-req", c2, 2, 1)]
    recs = pod_records([p[1] for p in pods], 0xD80000)
    ext = ext_records(owner=[p[2] for p in pods], required=[p[3] for p in pods])
    return Case(f"rsv-wide-{nrec}", nodes, np.zeros(N_WIDE, abi.NODE_DEVICES_DTYPE), recs, ext, ext_args(),
                reservations=np.array(rs, abi.RESERVATION_DTYPE), pod_names=tuple(p[0] for p in pods))


# ---------------------------------------------------------------------------------------------------------------------
# select shapes

SELECT_N = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
SELECT_BIG = 262145
SELECT_SHAPES = ("all-tie", "boundary", "last-max", "last-only", "none", "last-block")
BOUNDARY = (0, 255, 256, 1023, 1024)


def boundary_ties(n):
    """ties on the chunk and block boundaries and on the last node; beyond 256 blocks also around the middle block and
    on the last full block's last node (the last block's threads then own more than one block count each)"""
    extra = (1024 * 128 - 1, 1024 * 128, n - 2) if n > 262144 else ()
    return sorted({i for i in BOUNDARY + extra + (n - 1,) if 0 <= i < n})


def select_case(n: int, shape: str) -> Case:
    """n identical nodes. A node is `high` (empty: the best Fit score), `low` (half its cpu requested: feasible, a
    lower score) or `full` (no cpu left: infeasible for the pod)"""
    nodes = base_nodes(n)
    cpu = int(nodes["allocatable"][0, 0])
    high = np.zeros(n, bool)
    full = np.zeros(n, bool)
    if shape == "all-tie":
        high[:] = True
    elif shape == "boundary":
        high[boundary_ties(n)] = True
    elif shape == "last-max":
        high[n - 1] = True
    elif shape == "last-only":
        full[:n - 1] = True
        high[n - 1] = True
    elif shape == "none":
        full[:] = True
    elif shape == "last-block":
        high[(n - 1) // 1024 * 1024:] = True
    else:
        raise ValueError(shape)
    req = np.where(full, cpu, np.where(high, 0, cpu // 2))
    nodes["requested"][:, 0] = req
    nodes["nonzero_requested"][:, 0] = req
    pods = pod_records([{0: 1000, 1: GiB}], 0xD90000)
    return Case(f"select-{n}-{shape}", nodes, np.zeros(n, abi.NODE_DEVICES_DTYPE), pods, ext_records(gpu=[{}]),
                ext_args())


def select_ties(n: int, shape: str):
    """the node indices that tie at the maximum (in node order)"""
    if shape == "all-tie":
        return list(range(n))
    if shape == "boundary":
        return boundary_ties(n)
    if shape in ("last-max", "last-only"):
        return [n - 1]
    if shape == "none":
        return []
    return list(range((n - 1) // 1024 * 1024, n))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's view, computed once

def rows_of(x, case: Case, pods=None, seqs=(0,)):
    """[pod][seq] -> ext_rows dict of an Engine / Oracle holding the case"""
    pods = range(len(case.pods)) if pods is None else pods
    return [[x.ext_rows(case.pods[j], case.ext[j], s) for s in seqs] for j in pods]


def rows_equal(a: dict, b: dict):
    """the first key on which two ext_rows dicts differ (None: equal), with the first node"""
    for k in ROW_KEYS:
        if not np.array_equal(a[k], b[k]):
            i = int(np.nonzero(a[k] != b[k])[0][0])
            return f"{k}[{i}]: {a[k][i]} != {b[k][i]}"
    for k in RES_KEYS:
        if a[k] != b[k]:
            return f"{k}: {a[k]} != {b[k]}"
    return None


def assert_rows_equal(got, want, what):
    for j, (gj, wj) in enumerate(zip(got, want)):
        for s, (g, w) in enumerate(zip(gj, wj)):
            d = rows_equal(g, w)
            assert d is None, f"{what}: pod {j} seq #{s}: engine vs oracle {d}"


@functools.lru_cache(maxsize=None)
def oracle_rows(kind: str, *key):
    """cached oracle rows: ("ds", strategy, weights, ignored) | ("mem0", strategy) | ("policy",) | ("rsv", fit_filter) |
    ("wide", nrec), each followed by a variant name of VARIANTS"""
    *key, variant = key
    case = case_of(kind, *key)
    o = case.oracle(variant_args(case.args, dict(VARIANTS)[variant]))
    return rows_of(o, case)


def case_of(kind: str, *key) -> Case:
    return {"ds": ds_case, "mem0": ds_mem0_case, "policy": policy_case, "rsv": rsv_case, "wide": rsv_wide_case}[kind](*key)


# every stateless (kind, key..., variant) the CPU and the GPU test walk
def stateless_keys():
    out = [("ds", s, w, 0, "default") for s in STRATEGIES for w in WEIGHTS]
    out += [("ds", "LeastAllocated", (0, 1, 0), IGNORE_KOORD, "default"), ("ds", "MostAllocated", (1, 1, 1), 1 << NV, "coprime")]
    out += [("ds", "MostAllocated", (0, 0, 0), 0, "default")]   # no weighted resource: every raw score 0 (MDS == 0)
    out += [("mem0", s, "default") for s in STRATEGIES]
    out += [("policy", "default")]
    out += [("rsv", True, v) for v, _ in VARIANTS] + [("rsv", False, "default")]
    out += [("wide", n, "default") for n in WIDE_NREC] + [("wide", 257, "coprime")]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the integer restatement (from the reference's Go text)

def py_pod_request(e):
    """deviceshare/utils.go ValidateDeviceRequest + ConvertDeviceRequest, GPU type: {} no request, None invalid, else
    {"core" | "ratio" | "mem": value}"""
    names = {n: int(e["gpu_requests"][n]) for n in range(5) if int(e["gpu_request_mask"]) >> n & 1}
    if not names:
        return {}
    for n in (KG, CO, RA):   # ValidatePercentageResource
        if n in names and names[n] > 100 and names[n] % 100 != 0:
            return None
    ks = frozenset(names)
    if ks == {NV}:
        return {"core": names[NV] * 100, "ratio": names[NV] * 100}
    if ks == {KG}:
        return {"core": names[KG], "ratio": names[KG]}
    if ks == {ME}:
        return {"mem": names[ME]}
    if ks == {RA}:
        return {"ratio": names[RA]}
    if ks == {CO, ME}:
        return {"core": names[CO], "mem": names[ME]}
    if ks == {CO, RA}:
        return {"core": names[CO], "ratio": names[RA]}
    return None


KEYS = ("core", "ratio", "mem")


def _gpus(d):
    return [{"minor": int(g["minor"]), "info": bool(g["has_info"]),
             "total": dict(zip(KEYS, (int(v) for v in g["total"]))),
             "free": {k: max(0, int(t) - int(u)) for k, t, u in zip(KEYS, g["total"], g["used"])}}
            for g in d["gpus"][:int(d["num_gpus"])]]


def py_desired(gpus, req):
    """devicehandler_gpu.go:38-97 CalcDesiredRequestsAndCount: (per-instance requests, count) or None"""
    if not gpus:
        return None
    total = next((g["total"] for g in gpus if any(g["total"].values())), None)   # fillGPUTotalMem: the first healthy
    if total is None:
        return None
    req = dict(req)
    if "mem" in req:
        req["ratio"] = int(float(req["mem"]) / float(total["mem"]) * 100)        # memoryBytesToRatio
    else:
        req["mem"] = req.get("ratio", 0) * total["mem"] // 100                   # memoryRatioToBytes
    ratio = req["ratio"]
    if ratio > 100 and ratio % 100 == 0:
        n = ratio // 100
        return {"core": req.get("core", 0) // n, "mem": req["mem"] // n, "ratio": ratio // n}, n
    return req, 1


def py_least(requested, capacity):
    return 0 if capacity == 0 or requested > capacity else (capacity - requested) * 100 // capacity


def py_most(requested, capacity):
    return 0 if capacity == 0 else min(requested, capacity) * 100 // capacity


def py_score_node(inst, cands, weights, most):
    """scoring.go:213-243 scoreNode + the least / most scorers (:254-308)"""
    ns = ws = 0
    for k, w in zip(KEYS, weights):
        if not w:
            continue
        total = sum(g["total"][k] for g in cands)
        if total == 0:
            continue
        free = sum(g["free"][k] for g in cands)
        rq = total
        if total >= free:
            rq = total - free + inst.get(k, 0)
        ns += (py_most(rq, total) if most else py_least(rq, total)) * w
        ws += w
    return 0 if ws == 0 else ns // ws


def py_device_pair(d, e, args):
    """(feasible, raw DeviceShare score) of one pod on one node without NUMA affinity: Fit's GPU-name scalars, the
    DeviceShare Filter (plugin.go:272-322 -> defaultAllocateDevices) and Score; None for a PreFilter failure"""
    req = py_pod_request(e)
    if req is None:
        return None
    if not req:
        return True, 0
    for n in range(5):   # [upstream] fitsRequest over the scalar names
        if int(e["gpu_request_mask"]) >> n & 1 and not args.fit_ignored_gpu_names >> n & 1:
            if int(e["gpu_requests"][n]) > int(d["allocatable"][n]) - int(d["requested"][n]):
                return False, 0
    if not d["has_device"]:
        return True, 0
    gpus = _gpus(d)
    des = py_desired(gpus, req)
    if des is None:
        return False, 0
    inst, count = des
    if all(not any(g["free"].values()) for g in gpus):   # nodeDevice.filter drops a type without free resources
        return False, 0
    cands = [g for g in gpus if g["info"]]
    ok = sum(1 for g in cands if any(g["free"].values()) and all(v <= g["free"][k] for k, v in inst.items()))
    if ok < count:
        return False, 0
    weights = tuple(args.device_weights)
    return True, py_score_node(inst, cands, weights, args.device_scoring_type == abi.GS_SCORING_MOST_ALLOCATED)


def py_score_reservation(pod, r):
    """reservation/scoring.go:183-203 scoreReservation with allocated = Allocated (milli values: cpu is in milli)"""
    s = w = 0
    for k in range(7):
        cap = int(r["allocatable"][k]) if int(r["allocatable_mask"]) >> k & 1 else 0
        if cap == 0:
            continue
        w += 1
        req = (int(pod["requests"][k]) if int(pod["request_mask"]) >> k & 1 else 0) + \
              (int(r["allocated"][k]) if int(r["allocated_mask"]) >> k & 1 else 0)
        if req <= cap:
            m = 1 if k == 0 else 1000
            s += 100 * (req * m) // (cap * m)
    return s // w if w else 0


def py_normalize(scores):
    """[upstream] DefaultNormalizeScore(100, false)"""
    mx = max(scores, default=0)
    return list(scores) if mx == 0 else [100 * v // mx for v in scores]


def py_totals(row, args):
    """the `total` row from the oracle's base and raw rows: both normalizations, PreScore's preferred node and the
    plugin weights, over the feasible nodes"""
    fl = np.nonzero(row["feasible"])[0]
    ds = py_normalize([int(row["ds_raw"][i]) for i in fl])
    rs = py_normalize([1000 if i == row["pref_node"] else int(row["rs_raw"][i]) for i in fl])
    out = np.full(len(row["feasible"]), -1, np.int64)
    ds_on, rs_on = args.enabled & abi.GS_EXT_DEVICESHARE, args.enabled & abi.GS_EXT_RESERVATION
    for k, i in enumerate(fl):
        out[i] = int(row["base"][i]) + (ds[k] * args.weight_deviceshare if ds_on else 0) + \
            (rs[k] * args.weight_reservation if rs_on else 0)
    return out
