"""Truth for RDMA and FPGA as DeviceShare device types (gs_schedule_ext_aux: eval_aux_type in gs_ext.hip, aux_reserve_row
and aux_unreserve_row in gs_engine.cpp). The truth never calls the code under test: it is the oracle plus an integer
restatement of the reference's Go text.

For a pod with an RDMA / FPGA request:
 1. Oracle.ext_rows(pod, ext) gives every node's feasibility, base total and raw GPU score (Fit with the two names as
    registered extended resources, LoadAware, the GPU type);
 2. py_aux_node adds each node's verdict and raw score of the two types from a Python-held device table (AuxTable);
 3. feasible' = feasible and aux_ok, ds_raw' = ds_raw + aux_raw;
 4. both normalizations and the plugin weights as ext_edges_util.py_totals (the Reservation score is 0 for these pods);
 5. selectHost as the reservoir loop over node order with oracle.tiebreak_intn (tests/test_sampling.py).

Go text restated (pkg/scheduler/plugins/deviceshare): utils.go:84-90,147-175,232-252 (ValidatePercentageResource:
q > 100 with q % 100 != 0 is invalid), devicehandler_default.go:44-93 (CalcDesiredRequestsAndCount),
device_allocator.go:77-97 (Prepare), :139-163 (filterNodeDevice), device_cache.go:344-395 (nodeDevice.filter),
device_allocator.go:397-467 (defaultAllocateDevices), device_resources.go:171-208 (the sort), scoring.go:186-243
(scoreDevice, scoreNode; the scorers :254-308 range over the requested names, so a type's one weight only switches its
score on), device_allocator.go:513-536 (score: the sum over the types), plugin.go:377-451 (Reserve / Unreserve).

Sequences: after each pod the truth's node is replayed into the oracle (schedule_replay for the base assume, the Device
row's xres_requested by get / modify / upsert) and the Reserve applied to the AuxTable. Sequence pods are plain, GPU-only
(placed by Oracle.schedule_ext) or aux-only: the oracle cannot replay a GPU Reserve on a given node.
"""
from __future__ import annotations

import copy
import functools

import numpy as np

from koordinator_amd import abi, config
from oracle import oracle as orc
from tests import ext_edges_util as xu
from tests import ext_forget_util as xf

RDMA, FPGA = abi.GS_AUX_RDMA, abi.GS_AUX_FPGA
TYPES = (RDMA, FPGA)
NONE, ALL, COUNT = abi.GS_AUX_STRATEGY_NONE, abi.GS_AUX_APPLY_FOR_ALL, abi.GS_AUX_REQUESTS_AS_COUNT
STRATEGIES = (NONE, ALL, COUNT)
XRES_OF = {RDMA: 0, FPGA: 1}      # the two names as the caller's registered extended resources 0 and 1
N = 513
BOUNDARY = (0, 255, 256, 511, 512)


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def dev(total=100, used=0, minor=None, info=1, numa=-1):
    return {"total": total, "used": used, "minor": minor, "info": info, "numa": numa}


def aux_node(rdma=(), fpga=()):
    """{type: [device]} with minors filled in by position"""
    out = {}
    for T, ds in ((RDMA, rdma), (FPGA, fpga)):
        out[T] = [dict(d, minor=k if d["minor"] is None else d["minor"]) for k, d in enumerate(ds)]
    return out


def aux_record(node) -> np.ndarray:
    r = np.zeros(1, abi.NODE_AUX_DEVICES_DTYPE)[0]
    for T in TYPES:
        r["num"][T] = len(node[T])
        for k, d in enumerate(node[T]):
            x = r["dev"][T][k]
            x["minor"], x["has_info"], x["numa_node"], x["total"], x["used"] = d["minor"], d["info"], d["numa"], d["total"], d["used"]
    return r


def aux_pod(rdma=0, fpga=0, strategy=(NONE, NONE), exclusive=(0, 0)) -> np.ndarray:
    a = np.zeros(1, abi.POD_AUX_DTYPE)[0]
    a["request"] = (rdma, fpga)
    a["strategy"] = strategy
    a["device_exclusive"] = exclusive
    return a


def ext_of(aux, gpu=None) -> np.ndarray:
    """the gs_pod_ext beside a gs_pod_aux: the two names as extended-resource requests, and the GPU names"""
    e = xu.ext_records(gpu=[gpu or {}])[0]
    for T in TYPES:
        if int(aux["request"][T]):
            e["xres_requests"][XRES_OF[T]] = int(aux["request"][T])
            e["xres_request_mask"] |= 1 << XRES_OF[T]
    return e


class AuxTable:
    """the Python-held RDMA / FPGA device table: one aux_node per node"""

    def __init__(self, nodes):
        self.nodes = [copy.deepcopy(n) for n in nodes]

    def records(self) -> np.ndarray:
        return np.array([aux_record(n) for n in self.nodes], abi.NODE_AUX_DEVICES_DTYPE)

    def clone(self):
        return AuxTable(self.nodes)


# ---------------------------------------------------------------------------------------------------------------------
# the integer restatement

def py_aux_valid(aux) -> bool:
    """ValidatePercentageResource, whatever the strategy"""
    return all(not (int(q) > 100 and int(q) % 100 != 0) for q in aux["request"])


def py_aux_desired(q, strategy, exclusive, n):
    """CalcDesiredRequestsAndCount on a node listing n devices of the type: (inst, count, branch)"""
    if q > 100 and q % 100 == 0:
        return 100, q // 100, "multi"
    if strategy == ALL:
        return q, n, "all"
    if strategy == COUNT:
        return (100 if exclusive else 1), q, "count"
    return q, 1, "none"


def _free(d):
    return max(0, d["total"] - d["used"])


def py_score_one(total, free, inst, weight, most):
    """scoreDevice / scoreNode over one resource name"""
    if not weight or total == 0:
        return 0
    rq = total
    if total >= free:
        rq = total - free + inst
    return xu.py_most(rq, total) if most else xu.py_least(rq, total)


def py_aux_type(devs, q, strategy, exclusive, weight, most, seen=None):
    """one type on one node: (ok, raw score, minors the Reserve takes or None)"""
    tag = (seen.add if seen is not None else (lambda t: None))
    if not devs:
        tag("fail:no-devices")
        return False, 0, None
    inst, count, branch = py_aux_desired(q, strategy, exclusive, len(devs))
    tag("branch:" + branch)
    if all(_free(d) == 0 for d in devs):
        tag("fail:all-zero")
        return False, 0, None
    cands = [d for d in devs if d["info"]]
    usable = [d for d in cands if _free(d) != 0 and inst <= _free(d)]
    if len(usable) < count:
        tag("fail:short")
        return False, 0, None
    raw = py_score_one(sum(d["total"] for d in cands), sum(_free(d) for d in cands), inst, weight, most)
    order = sorted(usable, key=lambda d: (-py_score_one(d["total"], _free(d), inst, weight, most), d["minor"]))
    tag("ok")
    tag("most" if most else "least")
    return True, raw, ([d["minor"] for d in order[:count]], inst, count)


def py_aux_node(node, has_device, aux, weights, most, seen=None):
    """every requested type on one node: (ok, summed raw score, {type: (minors, inst, count)})"""
    if not has_device:
        if seen is not None:
            seen.add("pass:no-device-object")
        return True, 0, {}
    raw, alloc = 0, {}
    for T in TYPES:
        q = int(aux["request"][T])
        if not q:
            continue
        ok, r, a = py_aux_type(node[T], q, int(aux["strategy"][T]), int(aux["device_exclusive"][T]), weights[T], most, seen)
        if not ok:
            return False, 0, {}
        raw += r
        alloc[T] = a
    return True, raw, alloc


def py_reserve(node, alloc) -> None:
    for T, (minors, inst, _) in alloc.items():
        for d in node[T]:
            if d["minor"] in minors:
                d["used"] += inst


def py_forget(node, alloc) -> None:
    """Unreserve: max(0, used - inst) on the recorded minors the row still holds"""
    for T, (minors, inst, _) in alloc.items():
        for d in node[T]:
            if d["minor"] in minors:
                d["used"] = max(0, d["used"] - inst)


def placement_of(alloc) -> np.ndarray:
    a = np.zeros(1, abi.AUX_PLACEMENT_DTYPE)[0]
    for T, (minors, inst, count) in alloc.items():
        a["minor_mask"][T] = sum(1 << m for m in minors)
        a["count"][T] = count
        a["per_instance"][T] = inst
    return a


def select_host(total, seed, seq):
    """[upstream] selectHost: (node, score, ties) by the reservoir over node order"""
    sel, best, cnt = -1, -1, 0
    for i, t in enumerate(total):
        t = int(t)
        if t < 0:
            continue
        if t > best:
            sel, best, cnt = i, t, 1
        elif t == best:
            cnt += 1
            if orc.tiebreak_intn(seed, int(seq), cnt) == 0:
                sel = i
    return sel, best, cnt


def truth_rows(o, table, has_device, pod, ext, aux, args, weights, seed, seq=0, seen=None, base_row=None):
    """the ext_rows dict the engine must return for the pod, and the chosen node's aux allocation"""
    n = len(table.nodes)
    if not py_aux_valid(aux) or (args.enabled & abi.GS_EXT_DEVICESHARE and xu.py_pod_request(ext) is None):
        row = {"feasible": np.zeros(n, np.int32), "base": np.full(n, -1, np.int32), "ds_raw": np.zeros(n, np.int32),
               "rs_raw": np.zeros(n, np.int32), "total": np.full(n, -1, np.int32), "nominated_uid": np.zeros(n, np.uint64)}
        row.update({k: 0 for k in xu.RES_KEYS})
        row.update(node=-1, pref_node=-1, fail_code=abi.GS_EXT_FAIL_POD)
        return row, {}
    row = dict(o.ext_rows(pod, ext, seq) if base_row is None else base_row)
    most = args.device_scoring_type == abi.GS_SCORING_MOST_ALLOCATED
    feas, base, ds = row["feasible"].copy(), row["base"].copy(), row["ds_raw"].copy()
    allocs = {}
    asks = any(int(q) for q in aux["request"]) and args.enabled & abi.GS_EXT_DEVICESHARE
    for i in range(n):
        if not feas[i] or not asks:
            continue
        ok, raw, alloc = py_aux_node(table.nodes[i], has_device[i], aux, weights, most, seen)
        if ok:
            ds[i] += raw
            allocs[i] = alloc
        else:
            feas[i], base[i], ds[i] = 0, -1, 0
    row.update(feasible=feas, base=base, ds_raw=ds, rs_raw=np.zeros(n, np.int32))
    total = xu.py_totals(dict(row, pref_node=-1), args)
    node, score, ties = select_host(total, seed, seq)
    fl = [int(ds[i]) for i in np.nonzero(feas)[0]]
    norm = dict(zip(np.nonzero(feas)[0].tolist(), xu.py_normalize(fl)))
    row.update(total=total.astype(np.int32), node=node, score=max(score, 0), ties=ties, feasible_count=int(feas.sum()),
               pref_node=-1, ds_norm=(norm[node] if node >= 0 and args.enabled & abi.GS_EXT_DEVICESHARE else 0), rs_norm=0,
               fail_code=0)
    return row, allocs.get(node, {})


# ---------------------------------------------------------------------------------------------------------------------
# the 513-node cluster: anchors on the 256-thread boundaries of ext_nodes_kernel (which are SEL_BLOCK chunk boundaries of
# the select passes too), benign fillers everywhere else

FILLER = aux_node(rdma=[dev(), dev()], fpga=[dev()])
GPUS4 = [xu.gpu() for _ in range(4)]


def anchors():
    """(name, aux_node, has_device, GPUs, xres allocatable of the two names)"""
    roomy = (1600, 1600)
    used = lambda *us: [dev(used=u) for u in us]   # noqa: E731
    return [
        ("nodev", aux_node(rdma=used(0, 0), fpga=used(0)), 0, [], roomy),
        ("no-rdma", aux_node(fpga=used(0)), 1, GPUS4, roomy),
        ("no-fpga", aux_node(rdma=used(0, 0)), 1, GPUS4, roomy),
        ("unhealthy-only", aux_node(rdma=[dev(total=0)], fpga=[dev(total=0)]), 1, GPUS4, roomy),
        ("full", aux_node(rdma=used(100, 100), fpga=used(100)), 1, GPUS4, roomy),
        ("over", aux_node(rdma=used(150, 30), fpga=used(120, 0)), 1, GPUS4, roomy),
        ("noinfo-all", aux_node(rdma=[dev(info=0), dev(info=0)], fpga=[dev(info=0)]), 1, GPUS4, roomy),
        ("noinfo-some", aux_node(rdma=[dev(info=0), dev(used=20), dev(info=0, used=90)], fpga=[dev(info=0), dev()]), 1, GPUS4, roomy),
        ("two-usable", aux_node(rdma=used(0, 0, 1, 100), fpga=used(0, 0, 50)), 1, GPUS4, roomy),
        ("one-usable", aux_node(rdma=used(0, 1, 1, 100), fpga=used(0, 50, 50)), 1, GPUS4, roomy),
        ("three-usable", aux_node(rdma=used(0, 0, 0, 1), fpga=used(0, 0, 0)), 1, GPUS4, roomy),
        ("minors", aux_node(rdma=[dev(minor=31, used=10), dev(minor=3, used=50), dev(minor=17, used=10)],
                            fpga=[dev(minor=17), dev(minor=3)]), 1, GPUS4, roomy),
        ("half", aux_node(rdma=used(50, 51, 99), fpga=used(50, 99)), 1, GPUS4, roomy),
        ("eight", aux_node(rdma=used(0, 10, 20, 30, 40, 50, 60, 70), fpga=used(*([0] * 8))), 1, GPUS4, roomy),
        ("unhealthy-mixed", aux_node(rdma=[dev(total=0), dev(), dev(total=0)], fpga=[dev(total=0), dev()]), 1, GPUS4, roomy),
        ("odd-total", aux_node(rdma=[dev(total=97, used=13), dev(total=33, used=32)], fpga=[dev(total=7, used=2)]), 1, GPUS4, roomy),
        ("fpga-full", aux_node(rdma=used(0, 0), fpga=used(100, 100)), 1, GPUS4, roomy),
        ("rdma-full", aux_node(rdma=used(100), fpga=used(0)), 1, GPUS4, roomy),
        ("gpu-full", aux_node(rdma=used(0, 0, 0), fpga=used(0, 0, 0)), 1, [xu.used_pct(100) for _ in range(4)], roomy),
        ("fit-short", aux_node(rdma=used(0, 0, 0), fpga=used(0, 0, 0)), 1, GPUS4, (40, 40)),
        ("busy", aux_node(rdma=used(90, 90, 90), fpga=used(90, 90, 90)), 1, [xu.used_pct(90) for _ in range(4)], roomy),
    ]


POSITIONS = BOUNDARY + (1, 254, 257, 510, 100, 300, 400, 128, 384, 64, 192, 320, 448, 2, 509, 253)


def cluster(rot=0):
    """(node records, Device rows, AuxTable, has_device, {anchor name: node}): anchor k sits on POSITIONS[(k + rot) % ..]"""
    an = anchors()
    assert len(an) <= len(POSITIONS)
    nodes = xu.base_nodes(N)
    devs = np.array([xu.device(GPUS4)] * N, abi.NODE_DEVICES_DTYPE)
    devs["xres_allocatable"][:, 0] = devs["xres_allocatable"][:, 1] = 1600
    aux = [FILLER] * N
    where = {}
    for k, (name, a, has_device, gpus, alloc) in enumerate(an):
        i = POSITIONS[(k + rot) % len(POSITIONS)]
        where[name] = i
        aux[i] = a
        devs[i] = xu.device(gpus, has_device=has_device)
        devs[i]["xres_allocatable"][:2] = alloc
    return nodes, devs, AuxTable(aux), [int(h) for h in devs["has_device"]], where


QS = (1, 50, 100, 101, 150, 200, 300)


def row_pods():
    """(name, gs_pod_aux, GPU names) of the stateless rows"""
    out = []
    for q in QS:
        for s in STRATEGIES:
            for x in (0, 1):
                out.append((f"rdma{q}-s{s}-x{x}", aux_pod(rdma=q, strategy=(s, NONE), exclusive=(x, 0)), None))
    out += [(f"fpga{q}-s{s}", aux_pod(fpga=q, strategy=(NONE, s)), None) for q in (1, 100, 200) for s in STRATEGIES]
    out += [("both", aux_pod(rdma=50, fpga=50), None), ("both-all", aux_pod(rdma=10, fpga=10, strategy=(ALL, ALL)), None),
            ("both-count", aux_pod(rdma=2, fpga=3, strategy=(COUNT, COUNT), exclusive=(1, 0)), None),
            ("both-bad-fpga", aux_pod(rdma=50, fpga=250), None),
            ("gpu-both", aux_pod(rdma=50, fpga=50), {xu.KG: 50}), ("gpu2-both", aux_pod(rdma=200, fpga=1), {xu.NV: 2}),
            ("gpu-rdma", aux_pod(rdma=100), {xu.CO: 50, xu.RA: 50}), ("gpu-bad-both", aux_pod(rdma=1, fpga=1), {xu.KG: 250}),
            ("gpu-only", aux_pod(), {xu.KG: 100}), ("plain", aux_pod(), None)]
    return out


# (GPU weights, aux weights, strategy, anchor rotation) of the stateless rows
ROW_VARIANTS = (((0, 1, 0), (0, 0), "LeastAllocated", 0), ((0, 1, 0), (1, 0), "LeastAllocated", 5),
                ((1, 1, 1), (3, 2), "MostAllocated", 10), ((1, 1, 1), (3, 2), "LeastAllocated", 16))
COVERAGE = {"pass:no-device-object", "fail:no-devices", "fail:all-zero", "fail:short", "ok", "least", "most",
            "branch:none", "branch:all", "branch:count", "branch:multi"}


def one_pod(k=0, cpu=1000):
    return xu.pod_records([{0: cpu, 1: xu.GiB}], 0xDE0000 + k)[0]


def load(x, nodes, devs, args):
    x.set_now(0)
    x.upsert_nodes(nodes)
    x.upsert_metrics(np.zeros(len(nodes), abi.METRIC_DTYPE))
    x.ext_configure(args)
    x.upsert_devices(devs)


def make_cfg():
    return config.make_config(N, enabled=xu.FIT)


@functools.lru_cache(maxsize=None)
def variant_truth(vi):
    """(the truth's rows of every row_pods() pod on ROW_VARIANTS[vi], the branches they reached): computed once"""
    gw, aw, strategy, rot = ROW_VARIANTS[vi]
    nodes, devs, table, has_device, _ = cluster(rot)
    args, cfg = xu.ext_args(strategy, gw), make_cfg()
    o = orc.Oracle(cfg)
    load(o, nodes, devs, args)
    seen, rows = set(), []
    for k, (_, aux, gpu) in enumerate(row_pods()):
        rows.append(truth_rows(o, table, has_device, one_pod(k), ext_of(aux, gpu), aux, args, aw, cfg.seed, k, seen)[0])
    return rows, frozenset(seen)


# ---------------------------------------------------------------------------------------------------------------------
# sequences against the oracle

class Truth:
    """the sequential truth: an Oracle for everything but the two types, an AuxTable for them"""

    def __init__(self, cfg, nodes, devs, table, args, weights):
        self.o = orc.Oracle(cfg)
        load(self.o, nodes, devs, args)
        self.table, self.args, self.weights, self.seed = table.clone(), args, weights, cfg.seed
        self.has_device = [int(h) for h in devs["has_device"]]
        self.placed = {}    # uid -> (node, aux allocation or None, gs_pod_ext, the oracle's gs_ext_placement or None)

    def rows(self, pod, ext, aux, seq, seen=None):
        return truth_rows(self.o, self.table, self.has_device, pod, ext, aux, self.args, self.weights, self.seed, seq, seen)

    def _xres(self, node, ext, sign):
        d = self.o.devices(node).copy()
        for x in range(abi.GS_MAX_XRES):
            if int(ext["xres_request_mask"]) >> x & 1:
                d["xres_requested"][x] += sign * int(ext["xres_requests"][x])
        self.o.upsert_devices(np.array([d], abi.NODE_DEVICES_DTYPE), np.array([node], np.uint32))

    def schedule(self, pod, ext, aux, seq):
        """(node, feasible count, aux placement record) after the Reserve"""
        pods, s = np.array([pod], abi.POD_DTYPE), np.array([seq], np.uint64)
        if not any(int(q) for q in aux["request"]):   # plain or GPU-only: the oracle's own scheduleOne
            out, xo = self.o.schedule_ext(pods, np.array([ext], abi.POD_EXT_DTYPE), s)
            node = int(out["node"][0])
            if node >= 0:
                self.placed[int(pod["uid"])] = (node, None, ext, xo[0].copy())
            return node, int(out["feasible"][0]), placement_of({})
        row, alloc = self.rows(pod, ext, aux, seq)
        node = row["node"]
        if node < 0:
            return -1, row["feasible_count"], placement_of({})
        self.o.schedule_replay(pods, np.array([node], np.int32), s)
        self._xres(node, ext, +1)
        py_reserve(self.table.nodes[node], alloc)
        self.placed[int(pod["uid"])] = (node, alloc, ext, None)
        return node, row["feasible_count"], placement_of(alloc)

    def forget(self, pod):
        node, alloc, ext, xo = self.placed.pop(int(pod["uid"]))
        if alloc is None:   # placed by the oracle: its Unreserves as tests/ext_forget_util.py restates them
            xf.oracle_forget_ext(self.o, node, pod, ext, xo)
            return node
        self.o.forget(np.array([node], np.uint32), np.array([pod], abi.POD_DTYPE))
        self._xres(node, ext, -1)
        py_forget(self.table.nodes[node], alloc)
        return node
