"""Input builders for the device cpuset Reserve (koordinator_amd/csrc/gs_cpuset_dev.h as the commit kernels compile it,
cpuset_reserve in gs_eval_dev.h) at its topology and request-size edges. Every directed scenario is a one-node cluster
(its own topology, gs_node_numa record, existing allocations and pods) whose pods are issued in one gs_schedule call, so
that every Reserve after the first reads the CPU state the device itself wrote; a second call of a few pods follows on
the state the host re-derived. edge_cluster(seed) is the random family: 8 nodes drawn from the same topologies, 128 pods.

Lines of gs_cpuset_dev.h each family is aimed at:

* ladder-small (1, cpc-1, cpc, cpc+1, cpn-1, cpn, cpn+1 CPUs): pick_full_node / pick_cpus (:338-386) at needed == and
  needed > the list length, the `needed <= cpn` / `needed <= cps` gates of td_take_cpus_t (:481-482, :534), take_head_cores
  ending on a partial core (:286-294), take_spread_cpu_list's `L <= cpc` shortcut (:327);
* ladder-large (more than two sockets' worth, cps+1, cps, every remaining CPU): the socket-spanning part of
  td_take_cpus_t (:488-528: the (size, id) insertion into TdPack8 entries 0-7, td_go_sort's gap-6 pass :451-454 at 7 and
  8 sockets, the unsatisfied lists :511-526) and take_free_cpus (:390-444: its TdPack8 of up to 8 NUMA nodes, the colo
  key after a partial take);
* shapes: td_all at n == bits (:131-134) and the last dwords of cpu_core / cpu_pos through td_u8 (:107-114) on
  (1,1,64,4); core rank 64 across the words of cm_t (td_ctz / td_pc :98-101, td_unpack / td_pack :142-153) on
  (1,1,65,2) and (2,2,32,2); the cpc == 1 branch (:479) on (2,4,16,1); sibling-interleaved numbering (core_cpu /
  cpu_core / cpu_pos, take_cpu_order :297-320);
* state: RefCount-1 planes (ref_level :252-258, td_rth :208-217, td_reserve_update's maxRefCount-2 branch :644-646 and
  CM_XSTALE :652), exclusive cores and NUMA nodes (keep_xp / keep_xn :261-264, :654-656), reserved CPUs
  (td_available :556-561), MostAllocated / LeastAllocated (sless / dir :241-242);
* NUMA policies: the per-zone loop of td_allocate_cpuset_t (:592-615), td_zone_node (:553) with zones that name
  non-adjacent NUMA nodes, the last one and an id the topology lacks, and the zal / zfree updates
  (td_reserve_update_t :657-663, cpuset_reserve's td_counts per zone);
* out of scope (TopoDev.ok = 0 or maxRefCount 3): cs.topo < 0, the batch is cut and the host selects.

Everything is cached together with the oracle's results (computed once; tests/test_cpuset_edges.py proves from them
that the inputs reach their edges, tests/test_gpu_cpuset_edges.py compares the engine with them; neither changes them).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from koordinator_amd import abi, config, numa
from oracle import oracle as orc

FIELDS = ("node", "score", "ties", "feasible")
RESERVE_MASK = abi.GS_PLACED_NUMA | abi.GS_PLACED_CPUSET | (0xF << abi.GS_PLACED_AFFINITY_SHIFT)
GiB = 1 << 30
FULL, SPREAD = "FullPCPUs", "SpreadByPCPUs"
PCPU, NUMAX = "PCPULevel", "NUMANodeLevel"

# (sockets, NUMA nodes per socket, cores per node, CPUs per core)
T_NARROW_LIMIT = (1, 1, 64, 4)
T_WIDE_MIN = (1, 1, 65, 2)
T_WIDE_LIMIT = (2, 2, 32, 2)
T_WIDE_SMT1 = (2, 4, 16, 1)
T_8S = (8, 1, 8, 2)
T_8S_WIDE = (8, 1, 16, 2)
T_7S = (7, 1, 4, 2)
T_8N_SMT4 = (1, 8, 4, 4)
IN_SCOPE = (T_NARROW_LIMIT, T_WIDE_MIN, T_WIDE_LIMIT, T_WIDE_SMT1, T_8S, T_8S_WIDE, T_7S, T_8N_SMT4)


@dataclass(frozen=True)
class Pod:
    cpus: int
    bind: str = ""          # CPU bind policy
    required: bool = False  # ... as ResourceSpec.RequiredCPUBindPolicy (else the preferred one)
    excl: str = ""          # PreferredCPUExclusivePolicy


@dataclass(frozen=True)
class Alloc:                # an existing PodAllocation
    cpus: tuple
    excl: str = ""


@dataclass(frozen=True)
class Scenario:
    name: str
    topo: tuple
    pods: tuple                     # the first gs_schedule call
    more: tuple = ()                # the second one
    interleave: bool = False        # sibling-interleaved CPU numbering: cpu = thread * cores + core
    sparse: bool = False            # NUMA node ids 1, 3, 5, ...
    zones: tuple | None = None      # NUMA node indexes of the NRT zones (None: the first GS_MAX_NUMA); -1: an absent id
    policy: str = ""                # numa-topology-policy of the node
    node_bind: str = ""
    strategy: str = ""
    max_ref: int = 1
    reserved: tuple = ()
    allocs: tuple = ()
    zone_memory: bool = True        # the NRT zones report memory (then a pod's memory hint, one zone wide, narrows the
                                    # merged affinity to one zone: no cpuset beyond cpn passes a NUMA-policy node)
    fit_factor: float | None = None  # NodeResourcesFit admits this many times the CPUs (None: max_ref times)
    scope: str = "device"           # "device": no cut; "host": outside the device scope; "xstale": CM_XSTALE cut

    @property
    def shape(self):
        s, n, c, p = self.topo
        return dict(sockets=s, nodes=s * n, cores=s * n * c, cpc=p, cpn=c * p, cps=n * c * p, total=s * n * c * p)


# ---------------------------------------------------------------------------------------------------------------------
# topology

def cpu_id(sc: Scenario | tuple, core: int, thread: int, interleave: bool | None = None) -> int:
    topo = sc.topo if isinstance(sc, Scenario) else sc
    il = sc.interleave if interleave is None else interleave
    s, n, c, p = topo
    return thread * (s * n * c) + core if il else core * p + thread


def node_id(sc: Scenario, idx: int) -> int:
    return 2 * idx + 1 if sc.sparse else idx


def build_topology(sc: Scenario) -> np.void:
    s, n, c, p = sc.topo
    cpus = [None] * (s * n * c * p)
    g = 0
    for sk in range(s):
        for nn in range(n):
            for co in range(c):
                for t in range(p):
                    cpus[cpu_id(sc, g, t)] = (sk, node_id(sc, sk * n + nn), nn * c + co)
                g += 1
    return numa.topology(cpus)


def cpu_place(sc: Scenario) -> dict:
    """cpu id -> (socket, NUMA node index, core rank)"""
    s, n, c, p = sc.topo
    out = {}
    for g in range(s * n * c):
        for t in range(p):
            out[cpu_id(sc, g, t)] = (g // (n * c), g // c, g)
    return out


def zone_indexes(sc: Scenario) -> tuple:
    if sc.zones is not None:
        return sc.zones
    return tuple(range(min(sc.shape["nodes"], abi.GS_MAX_NUMA)))


# ---------------------------------------------------------------------------------------------------------------------
# loading a scenario list into an Engine / Oracle

def _pod_records(pods, uid0):
    out = np.zeros(len(pods), abi.POD_DTYPE)
    for k, p in enumerate(pods):
        out[k]["requests"][abi.GS_RES_CPU] = out[k]["limits"][abi.GS_RES_CPU] = p.cpus * 1000
        out[k]["nonzero_requests"][0] = p.cpus * 1000
        out[k]["requests"][abi.GS_RES_MEMORY] = out[k]["limits"][abi.GS_RES_MEMORY] = 1 << 20
        out[k]["nonzero_requests"][1] = 1 << 20
        out[k]["request_mask"] = (1 << abi.GS_RES_CPU) | (1 << abi.GS_RES_MEMORY)
        out[k]["priority_class"] = abi.GS_PRIO_PROD
        out[k]["qos_class"] = abi.GS_QOS_LSR if k % 3 else abi.GS_QOS_LSE
        out[k]["required_cpu_bind_policy" if p.required else "preferred_cpu_bind_policy"] = abi.CPU_BIND[p.bind]
        out[k]["preferred_cpu_exclusive_policy"] = abi.CPU_EXCLUSIVE[p.excl]
        out[k]["uid"] = uid0 + k
    return out


@dataclass
class Case:
    scenarios: tuple
    cfg_kw: dict
    calls: list                      # POD_DTYPE arrays, one per gs_schedule call
    want: list = field(default_factory=list)        # the oracle's placements per call
    want_alloc: list = field(default_factory=list)  # per call: {pod index: allocation bytes}
    want_cpus: list = field(default_factory=list)   # per call: {pod index: [cpu ids]}

    def config(self, **kw):
        return config.make_config(len(self.scenarios), enabled=abi.GS_ENABLE_ALL, **{**self.cfg_kw, **kw})


def load(e, scenarios) -> None:
    """node i of the cluster = scenarios[i]"""
    N = len(scenarios)
    nodes = np.zeros(N, abi.NODE_DTYPE)
    recs, allocs, alloc_nodes = [], [], []
    for i, sc in enumerate(scenarios):
        sh = sc.shape
        # (maxRefCount > 1: the pods share CPUs, NodeResourcesFit must not bind before the cpuset does)
        nodes[i]["allocatable"][abi.GS_RES_CPU] = int(sh["total"] * 1000 * (sc.max_ref if sc.fit_factor is None else sc.fit_factor))
        nodes[i]["allocatable"][abi.GS_RES_MEMORY] = 1 << 40
        nodes[i]["allowed_pod_number"] = 400
        # NodeInfo.Requested holds the existing cpuset pods and stands in for the reserved CPUs, so that NodeResourcesFit
        # rejects what the CPUs cannot hold (without a NUMA policy the plugin's Filter counts no CPUs; a Reserve that
        # fails after a feasible Filter is an error on both engines)
        held = (sum(len(a.cpus) for a in sc.allocs) + len(sc.reserved) * sc.max_ref) * 1000
        nodes[i]["requested"][abi.GS_RES_CPU] = nodes[i]["nonzero_requested"][0] = held
    e.set_now(0)
    e.upsert_nodes(nodes)
    e.upsert_metrics(np.zeros(N, abi.METRIC_DTYPE))
    for i, sc in enumerate(scenarios):
        sh = sc.shape
        tid = e.register_topology(build_topology(sc))
        zones = []
        for zi in zone_indexes(sc):
            # an id the topology lacks: one past the last NUMA node's. It reports memory only: a zone with cpu but no
            # CPUs draws hints whose Allocate fails after the admit, on the reference too
            zid = node_id(sc, zi) if zi >= 0 else node_id(sc, sh["nodes"] - 1) + 1
            zones.append((zid, sh["cpn"] * 1000 * sc.max_ref if zi >= 0 else None, 64 * GiB if sc.zone_memory else None))
        recs.append(numa.node_numa(tid, zones=zones, numa_policy=sc.policy, node_cpu_bind=sc.node_bind,
                                   numa_allocate_strategy=sc.strategy, max_ref_count=sc.max_ref,
                                   reserved_cpus=sc.reserved))
        place = cpu_place(sc)
        zids = {z[0] for z in zones}
        for j, a in enumerate(sc.allocs):
            per = {}
            for c in a.cpus:
                nid = node_id(sc, place[c][1])
                per[nid] = per.get(nid, 0) + 1
            # on a NUMA-policy node the allocation carries its NUMA resources (the zones the NRT reports)
            res = [(nid, cnt * 1000, 1 << 20) for nid, cnt in sorted(per.items()) if nid in zids] if sc.policy else []
            allocs.append(numa.pod_allocation(0xA110C000 + 256 * i + j, a.cpus, res[:abi.GS_MAX_NUMA], exclusive=a.excl))
            alloc_nodes.append(i)
    e.upsert_numa(np.array(recs, abi.NODE_NUMA_DTYPE))
    if allocs:
        e.update_allocations(np.array(alloc_nodes, np.uint32), np.array(allocs, abi.POD_ALLOCATION_DTYPE))


def run_calls(e, case: Case):
    """the case's gs_schedule calls on a loaded engine -> (placements, {pod: allocation bytes}, {pod: cpus}) per call"""
    outs = []
    lo = 0
    for pods in case.calls:
        got = e.schedule(pods, np.arange(lo, lo + len(pods), dtype=np.uint64))
        lo += len(pods)
        al, cp = {}, {}
        for j in np.nonzero(got["flags"] & (abi.GS_PLACED_CPUSET | abi.GS_PLACED_NUMA))[0]:
            a = e.allocation(int(got["node"][j]), int(pods["uid"][j]))
            al[int(j)] = None if a is None else a.tobytes()
            if a is not None:
                cp[int(j)] = numa.cpus_of(a["cpuset"])
        outs.append((got, al, cp))
    return outs


def _with_oracle(case: Case) -> Case:
    o = orc.Oracle(case.config())
    load(o, case.scenarios)
    for got, al, cp in run_calls(o, case):
        case.want.append(got)
        case.want_alloc.append(al)
        case.want_cpus.append(cp)
    return case


# ---------------------------------------------------------------------------------------------------------------------
# directed scenarios

def _styled(sizes, sc_cpc, style, excl=()):
    """pods of `sizes` CPUs; style: "full" / "spread" (preferred), "mixed": preferred and required FullPCPUs /
    SpreadByPCPUs in turn (a required FullPCPUs only for whole cores), "node": none (the node's policy decides);
    excl: the exclusive policies, cycled"""
    out = []
    for k, n in enumerate(sizes):
        x = excl[k % len(excl)] if excl else ""
        if style == "full":
            out.append(Pod(n, FULL, False, x))
        elif style == "spread":
            out.append(Pod(n, SPREAD, False, x))
        elif style == "node":
            out.append(Pod(n, "", False, x))
        else:
            kind = k % 4
            if kind == 2 and n % sc_cpc:
                kind = 0
            out.append(Pod(n, FULL if kind in (0, 2) else SPREAD, kind >= 2, x))
    return tuple(out)


def small_sizes(topo):
    s, n, c, p = topo
    cpn = c * p
    seen, out = set(), []
    # (one NUMA node: also around one CPU per core, the longest required SpreadByPCPUs set)
    for v in (1, p - 1, p, p + 1) + ((c - 1, c, c + 1) if s * n == 1 else ()) + (cpn - 1, cpn, cpn + 1):
        if v >= 1 and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def ladder_small(name, topo, style="mixed", excl=(), **kw):
    """1, cpc-1, cpc, cpc+1, cpn-1, cpn, cpn+1 CPUs while they fit (every size at least once on a node of several NUMA
    nodes), then in the second call: cpc, 1 and every remaining CPU"""
    s, n, c, p = topo
    mr = kw.get("max_ref", 1)
    total = s * n * c * p * mr
    taken = len(kw.get("reserved", ())) * mr + sum(len(a.cpus) for a in kw.get("allocs", ()))
    sizes, used = [], taken + p + 1 + 1
    for v in small_sizes(topo):
        if used + v <= total:
            sizes.append(v)
            used += v
    rest = total - used + 1
    if mr > 1:   # (the shared CPUs may be full: Fit counts requests, not CPUs; half the node's CPUs are surely available)
        rest = min(rest, (s * n * c * p - len(kw.get("reserved", ()))) // 2)
    return Scenario(name, topo, _styled(sizes, p, style, excl), _styled([p, 1, rest], p, "full"), **kw)


def ladder_large(name, topo, style="full", excl=(), **kw):
    """more than two sockets' worth, cps+1, cps, (one socket: 2 cpn + 1, cpn + 1, cpn; one NUMA node: all but a core and
    three CPUs) while they fit, then every remaining CPU — all in the first call; the second call asks for one more
    core, which nothing holds any more"""
    s, n, c, p = topo
    cpn, cps = c * p, n * c * p
    total = s * n * c * p
    taken = len(kw.get("reserved", ())) + sum(len(a.cpus) for a in kw.get("allocs", ()))
    want = [2 * cps + 1, cps + 1, cps] if s >= 3 else [cps + 1, cpn + 1] if s == 2 else [2 * cpn + 1, cpn + 1, cpn]
    if s == 1 and n == 1:
        want = [total - taken - p - 3, 2]
    sizes, used = [], taken
    for v in want:
        if used + v < total:
            sizes.append(v)
            used += v
    sizes.append(total - used)
    return Scenario(name, topo, _styled(sizes, p, style, excl), _styled([p], p, "full"), **kw)


def _thread0_of_every_other_core(topo, interleave=False):
    s, n, c, p = topo
    return tuple(cpu_id(topo, g, 0, interleave) for g in range(0, s * n * c, 2))


def _cores(topo, cores, interleave=False, threads=None):
    p = topo[3]
    return tuple(cpu_id(topo, g, t, interleave) for g in cores for t in (range(p) if threads is None else threads))


def directed_scenarios() -> tuple:
    S = []
    # ---- every table topology: the small and the large ladder on an empty node
    S.append(ladder_small("narrow-limit/small", T_NARROW_LIMIT, strategy="MostAllocated"))
    S.append(ladder_large("narrow-limit/large", T_NARROW_LIMIT, style="spread", strategy="LeastAllocated"))
    S.append(ladder_small("wide-min/small", T_WIDE_MIN, interleave=True))
    S.append(ladder_large("wide-min/large", T_WIDE_MIN, strategy="MostAllocated"))
    S.append(ladder_small("wide-limit/small", T_WIDE_LIMIT, strategy="LeastAllocated", excl=("", PCPU)))
    S.append(ladder_large("wide-limit/large", T_WIDE_LIMIT, interleave=True, strategy="MostAllocated"))
    S.append(ladder_small("wide-smt1/small", T_WIDE_SMT1, style="spread", sparse=True))
    S.append(ladder_large("wide-smt1/large", T_WIDE_SMT1, style="mixed", strategy="MostAllocated"))
    S.append(ladder_small("8s/small", T_8S, strategy="MostAllocated", zones=(0, 2, 5, 7)))
    S.append(ladder_large("8s/large", T_8S, strategy="LeastAllocated", zones=(1, 3, 6, 7)))
    S.append(ladder_small("8s-wide/small", T_8S_WIDE, interleave=True, zones=(0, 3, 5, 7), excl=("", "", NUMAX)))
    S.append(ladder_large("8s-wide/large", T_8S_WIDE, strategy="MostAllocated", zones=(0, 2, 4, 7)))
    S.append(ladder_small("7s/small", T_7S, sparse=True, zones=(0, 2, 4, 6)))
    S.append(ladder_large("7s/large", T_7S, strategy="MostAllocated", zones=(1, 3, 5, 6)))
    S.append(ladder_small("8n-smt4/small", T_8N_SMT4, strategy="LeastAllocated", zones=(0, 2, 5, 7)))
    S.append(ladder_large("8n-smt4/large", T_8N_SMT4, style="spread", strategy="MostAllocated", zones=(0, 3, 6, 7)))
    # ---- node state
    # one sibling taken on every other core: half the node has no full core
    S.append(ladder_small("siblings/8n-smt4", T_8N_SMT4, allocs=(Alloc(_thread0_of_every_other_core(T_8N_SMT4)),),
                          zones=(0, 2, 5, 7), strategy="MostAllocated"))
    S.append(Scenario("siblings/wide-limit", T_WIDE_LIMIT, _styled([65, 33, 3, 64, 27], 2, "mixed"),
                      _styled([2], 2, "full"), interleave=True,
                      allocs=(Alloc(_thread0_of_every_other_core(T_WIDE_LIMIT, True)),)))
    # 7 / 8 sockets, all but one with equal free sizes, MostAllocated: the (size, id) order starts with the smaller
    # socket, so sort.Slice's gap-6 pass swaps entries 0 and 6 and the equal sockets leave id order (Go 1.18 is not stable)
    for nm_, topo in (("8s", T_8S), ("8s-wide", T_8S_WIDE), ("7s", T_7S)):
        cps = topo[1] * topo[2] * topo[3]
        S.append(Scenario(f"equal-sockets/{nm_}", topo,
                          _styled([2 * cps + 2, cps + 2, 2, cps], topo[3], "full"), _styled([2, 1], topo[3], "full"),
                          allocs=(Alloc(_cores(topo, [0])),), strategy="MostAllocated", zones=(0, 2, 4, 6)))
    # every socket but one and a CPU: all 7 / 8 entries of the socket lists are sorted, taken and the last one split
    for nm_, topo, kw in (("8s", T_8S, dict(strategy="LeastAllocated")), ("8s-wide", T_8S_WIDE, dict(interleave=True)),
                          ("7s", T_7S, dict(strategy="MostAllocated", sparse=True))):
        cps, total = topo[1] * topo[2] * topo[3], topo[0] * topo[1] * topo[2] * topo[3]
        big = (topo[0] - 1) * cps + 1
        S.append(Scenario(f"all-sockets/{nm_}", topo, _styled([big, 2, 1, total - big - 3], 2, "full"),
                          _styled([2], 2, "full"), zones=(0, 2, 4, 6), **kw))
    # one socket clearly fuller than the rest, LeastAllocated and unset
    S.append(Scenario("fuller-socket/8s", T_8S, _styled([17, 33, 16, 7, 9], 2, "mixed"), _styled([2, 3], 2, "spread"),
                      allocs=(Alloc(_cores(T_8S, range(24, 30)), ""),), strategy="LeastAllocated", zones=(0, 3, 4, 7)))
    S.append(Scenario("fuller-socket/wide-limit", T_WIDE_LIMIT, _styled([129, 3, 24, 2], 2, "full"),
                      _styled([2, 1], 2, "full"), allocs=(Alloc(_cores(T_WIDE_LIMIT, range(64, 110))),)))
    # reserved CPUs: the last CPU ids of the narrow limit, a sibling of core rank 64 on the smallest wide shape
    S.append(ladder_small("reserved/narrow-limit", T_NARROW_LIMIT, style="spread", reserved=(0, 5, 254, 255),
                          strategy="MostAllocated"))
    S.append(ladder_large("reserved/wide-min", T_WIDE_MIN, style="mixed", reserved=(1, 128, 129), strategy="LeastAllocated"))
    # maxRefCount 2 with CPUs at RefCount 1 (no exclusive CPUs: the exclusivity state stays exact)
    S.append(Scenario("maxref2/8s", T_8S, _styled([3, 17, 16, 33, 5, 2, 64, 9], 2, "mixed"), _styled([2, 30], 2, "spread"),
                      max_ref=2, strategy="MostAllocated", zones=(0, 2, 5, 7),
                      allocs=(Alloc(_cores(T_8S, range(0, 20))), Alloc(_cores(T_8S, range(40, 50), threads=(0,))))))
    S.append(Scenario("maxref2/narrow-limit", T_NARROW_LIMIT, _styled([255, 256, 1], 4, "full"), _styled([4], 4, "full"),
                      max_ref=2, strategy="LeastAllocated"))
    S.append(Scenario("maxref2/wide-limit", T_WIDE_LIMIT, _styled([65, 129, 2, 3, 128, 63], 2, "mixed"),
                      _styled([2, 1, 64], 2, "full"), max_ref=2, interleave=True,
                      allocs=(Alloc(_cores(T_WIDE_LIMIT, range(60, 70))), Alloc(_cores(T_WIDE_LIMIT, range(100, 128), False, (1,))))))
    # existing PCPULevel- and NUMANodeLevel-exclusive allocations, exclusive pods
    S.append(Scenario("exclusive/8n-smt4", T_8N_SMT4,
                      _styled([1, 2, 3, 5, 15, 16, 17, 4, 6], 4, "spread", excl=(PCPU, NUMAX, "")),
                      _styled([2, 4], 4, "spread", excl=(PCPU, NUMAX)), zones=(0, 2, 5, 7),
                      allocs=(Alloc(_cores(T_8N_SMT4, [0, 5], threads=(0, 1)), PCPU), Alloc(_cores(T_8N_SMT4, [13], threads=(0,)), NUMAX))))
    S.append(Scenario("exclusive/wide-limit", T_WIDE_LIMIT,
                      _styled([1, 3, 2, 63, 65, 5, 31], 2, "mixed", excl=(NUMAX, PCPU, "", PCPU)),
                      _styled([2, 3], 2, "spread", excl=(PCPU, NUMAX)),
                      allocs=(Alloc(_cores(T_WIDE_LIMIT, [64, 65, 100], threads=(0,)), PCPU), Alloc(_cores(T_WIDE_LIMIT, [1]), NUMAX))))
    # the node's own cpu bind policy decides
    S.append(Scenario("node-bind-full/7s", T_7S, _styled([2, 4, 8, 10, 6, 18], 2, "node"), _styled([2, 4, 2], 2, "node"),
                      node_bind="FullPCPUsOnly", zones=(0, 2, 4, 6)))
    S.append(ladder_small("node-bind-spread/wide-smt1", T_WIDE_SMT1, style="node", node_bind="SpreadByPCPUs"))
    S.append(Scenario("node-bind-spread/8n-smt4", T_8N_SMT4, _styled([1, 3, 4, 5, 17, 32, 31], 4, "node"),
                      _styled([4, 1, 29], 4, "node"), node_bind="SpreadByPCPUs", interleave=True, zones=(0, 1, 6, 7)))
    # ---- NUMA topology policies: the per-zone selection; zones name non-adjacent NUMA nodes up to the last one
    S.append(Scenario("single-numa/8s", T_8S, _styled([1, 2, 4, 8, 16, 2, 14, 6], 2, "mixed"), _styled([2, 1, 5], 2, "full"),
                      policy="SingleNUMANode", zones=(0, 2, 5, 7), strategy="MostAllocated"))
    # (zones without memory: the cpu hint alone decides the affinity, so a request beyond cpn is split over zones)
    S.append(Scenario("restricted/wide-limit", T_WIDE_LIMIT, _styled([65, 1, 3, 32, 63, 2, 31], 2, "mixed"),
                      _styled([2, 1, 16], 2, "full"), policy="Restricted", interleave=True, zone_memory=False))
    S.append(Scenario("best-effort/8n-smt4", T_8N_SMT4, _styled([17, 3, 16, 5, 4, 8], 4, "mixed", excl=("", PCPU)),
                      _styled([4, 1], 4, "spread"), policy="BestEffort", zones=(0, 3, 6, 7), sparse=True,
                      strategy="LeastAllocated", zone_memory=False))
    S.append(Scenario("best-effort/8s-wide", T_8S_WIDE, _styled([33, 1, 65, 3, 2, 5], 2, "mixed"),
                      _styled([2, 1], 2, "full"), policy="BestEffort", zones=(1, 3, 4, 7), zone_memory=False))
    # a zone id the topology lacks (the device keeps that zone's summaries zero)
    S.append(Scenario("absent-zone/8s", T_8S, _styled([1, 3, 16, 8, 2, 4, 12], 2, "mixed"), _styled([2, 5], 2, "spread"),
                      policy="Restricted", zones=(0, 3, 6, -1)))
    S.append(ladder_small("absent-zone/wide-smt1", T_WIDE_SMT1, zones=(0, 2, 7, -1), strategy="MostAllocated"))
    # ---- CM_XSTALE: a maxRefCount-2 node that holds exclusive CPUs; a pod shares RefCount-1 CPUs of it (the policy of
    # the shared CPUs is overwritten: the device's exclusive cores / NUMA nodes may be inexact), then an exclusive pod
    # comes, whose cpuset the host selects by design (the batch ends with it; pods follow it, so the cut shows)
    S.append(Scenario("xstale/8s", T_8S, _styled([4, 124, 6, 2, 2, 3, 1], 2, "full", excl=("", "", "", PCPU, "", NUMAX, "")),
                      _styled([2, 1], 2, "full", excl=("", PCPU)), max_ref=2, scope="xstale",
                      allocs=(Alloc(_cores(T_8S, range(0, 4)), PCPU),)))
    # ---- outside the device scope: the host path
    S.append(ladder_small("host/wide-smt3", (1, 1, 65, 3), scope="host"))
    S.append(ladder_large("host/129-cores", (1, 1, 129, 1), scope="host"))
    S.append(ladder_large("host/9-sockets", (9, 1, 2, 2), scope="host", strategy="MostAllocated"))
    S.append(ladder_small("host/maxref3", T_8S, max_ref=3, scope="host", zones=(0, 2, 5, 7), strategy="MostAllocated",
                          allocs=(Alloc(_cores(T_8S, range(0, 10))),)))
    names = [s.name for s in S]
    assert len(set(names)) == len(names)
    return tuple(S)


DIRECTED = directed_scenarios()
DIRECTED_BY_NAME = {s.name: s for s in DIRECTED}
UID0 = 0xED6E0000


def _cfg_kw(sampled: bool) -> dict:
    """sampled: node sampling is on (the window commit kernel); below 100 nodes its window is every node"""
    return dict(percentage_of_nodes_to_score=50) if sampled else {}


@functools.lru_cache(maxsize=None)
def directed_case(name: str, sampled: bool = False) -> Case:
    """the one-node cluster of a directed scenario with the oracle's results of its two calls"""
    sc = DIRECTED_BY_NAME[name]
    calls = [_pod_records(sc.pods, UID0), _pod_records(sc.more, UID0 + 0x1000)]
    return _with_oracle(Case((sc,), _cfg_kw(sampled), calls))


# ---------------------------------------------------------------------------------------------------------------------
# the random family

RANDOM_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
RANDOM_NODES, RANDOM_PODS, RANDOM_MORE = 8, 128, 16
# A maxRefCount-2 node of T CPUs admits requests up to 1.5 T in all (NodeResourcesFit), so its pods come to share CPUs.
# After requests of S in all at most S / 2 CPUs are at RefCount 2, so a pod of n <= 1.5 T - S CPUs finds its n CPUs
# below maxRefCount iff n <= T / 2 in the worst case: 28 on the smallest topology (56 CPUs). A larger request could pass
# Fit and fail in Reserve, an error on both engines.
SHARED_MAX_CPUS = 28


def _random_scenario(rng, i, shared: bool) -> Scenario:
    """a node of a table topology with random numbering, zones, strategy, policy, reservations and allocations.
    shared: maxRefCount 2 on half the nodes and no exclusive CPUs anywhere (a shared exclusive CPU would end the
    device path by design, CM_XSTALE); else maxRefCount 1 and exclusive allocations."""
    topo = IN_SCOPE[int(rng.integers(len(IN_SCOPE)))]
    s, n, c, p = topo
    nodes, cores, total = s * n, s * n * c, s * n * c * p
    il = bool(rng.integers(2))
    mr = 2 if shared and rng.integers(2) else 1
    zones = None
    if nodes > abi.GS_MAX_NUMA:
        z = sorted(rng.choice(nodes - 1, abi.GS_MAX_NUMA - 1, replace=False).tolist()) + [nodes - 1]
        zones = tuple(int(v) for v in z)
    allocs = []
    kind = int(rng.integers(4))
    if kind == 1:   # one sibling on every other core
        allocs.append(Alloc(_thread0_of_every_other_core(topo, il), ""))
    elif kind == 2:   # one socket (or NUMA node) mostly taken
        per = cores // (s if s > 1 else nodes)
        k = int(rng.integers(s if s > 1 else nodes))
        allocs.append(Alloc(_cores(topo, range(k * per, k * per + max(1, per * 3 // 4)), il), ""))
    elif kind == 3:   # scattered CPUs
        pick = rng.choice(total, max(1, total // 6), replace=False)
        allocs.append(Alloc(tuple(sorted(int(v) for v in pick)), ""))
    if not shared and rng.integers(2):
        used = {c_ for a in allocs for c_ in a.cpus}
        free_cores = [g for g in range(cores) if not any(cpu_id(topo, g, t, il) in used for t in range(p))]
        if free_cores:
            g = free_cores[int(rng.integers(len(free_cores)))]
            allocs.append(Alloc(_cores(topo, [g], il, (0,)), (PCPU, NUMAX)[int(rng.integers(2))]))
    used = {c_ for a in allocs for c_ in a.cpus}
    reserved = tuple(sorted(int(v) for v in rng.choice(total, 2, replace=False) if int(v) not in used)) \
        if rng.integers(3) == 0 else ()
    return Scenario(f"random-{i}", topo, (), (), interleave=il, sparse=bool(rng.integers(2)), zones=zones,
                    policy=("", "", "SingleNUMANode", "Restricted", "BestEffort")[int(rng.integers(5))],
                    node_bind=("", "", "", "FullPCPUsOnly", "SpreadByPCPUs")[int(rng.integers(5))],
                    strategy=("", "MostAllocated", "LeastAllocated")[int(rng.integers(3))], max_ref=mr,
                    reserved=reserved, allocs=tuple(allocs), fit_factor=1.5 if mr == 2 else 1)


def _random_pods(rng, count, shared: bool, scenarios, small: bool = False):
    shapes = [sc.shape for sc in scenarios]
    out = []
    for _ in range(count):
        r = int(rng.integers(5 if small else 12))
        sh = shapes[int(rng.integers(len(shapes)))]
        if r < 6:
            n = 1 + int(rng.integers(4 if small else 8))
        elif r < 9:   # around a core or a NUMA node of one of the cluster's nodes
            n = max(1, int(rng.choice([sh["cpc"], sh["cpn"]])) + int(rng.integers(-1, 2)))
        elif r < 10:   # around a socket (of more than one NUMA node, or the node's only one)
            n = sh["cps"] + int(rng.integers(-1, 2))
        else:
            n = 9 + int(rng.integers(24))
        b = int(rng.integers(6))
        bind, req = (("", False), (FULL, False), (SPREAD, False), (SPREAD, False), (FULL, True), (SPREAD, True))[b]
        if bind == FULL and req and n % 2:
            n += 1
        if shared:
            n = min(n, SHARED_MAX_CPUS)
        x = "" if shared else ("", "", "", PCPU, NUMAX)[int(rng.integers(5))]
        out.append(Pod(n, bind, req, x))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_cluster(seed: int, sampled: bool = False) -> Case:
    """8 nodes of the table topologies, 128 random cpuset pods in one call and 16 in a second: the pods go where the
    scores send them, so every row takes many Reserves within one batch. Odd seeds: maxRefCount 2 on about half the
    nodes, nothing exclusive; even seeds: exclusive allocations and pods, maxRefCount 1."""
    rng = np.random.default_rng(0xC9E5 + seed)
    shared = bool(seed & 1)
    scs = tuple(_random_scenario(rng, i, shared) for i in range(RANDOM_NODES))
    calls = [_pod_records(_random_pods(rng, RANDOM_PODS, shared, scs), UID0 + 0x10000),
             _pod_records(_random_pods(rng, RANDOM_MORE, shared, scs, small=True), UID0 + 0x20000)]
    return _with_oracle(Case(scs, _cfg_kw(sampled), calls))


# ---------------------------------------------------------------------------------------------------------------------
# what a cpuset spans (the CPU tests' preconditions)

def span(sc: Scenario, cpus) -> dict:
    place = cpu_place(sc)
    p = sc.topo[3]
    socks = {place[c][0] for c in cpus}
    nodes = {place[c][1] for c in cpus}
    per_core = {}
    for c in cpus:
        per_core[place[c][2]] = per_core.get(place[c][2], 0) + 1
    return dict(sockets=len(socks), nodes=len(nodes),
                nodes_in_one_socket=max((sum(1 for n in nodes if n // sc.topo[1] == s) for s in socks), default=0),
                partial_core=any(v < p for v in per_core.values()), max_cpu=max(cpus, default=-1),
                max_core=max(per_core, default=-1), one_per_core=all(v == 1 for v in per_core.values()))
