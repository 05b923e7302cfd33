"""The preemption dry run's edge family: hand-built inputs and their truth.

Every cluster here is flat: N identical nodes (16 CPUs, memory that never binds, no NodeMetric so LoadAware passes, a
large allowed_pod_number), of which a few "anchor" nodes are overridden and hold designed resident lists; every other
node holds no resident and ends NO_VICTIMS. A scenario owns a quota id: only residents of the preemptor's quota are
potential victims, so the scenarios of one case do not see each other. The truth stays preempt_util.dry_run /
preempt_pdb_util.dry_run over the CPU oracle; a scenario records what it was built to produce (`expect`) and
tests/test_preempt_edges.py asserts that on the truth alone, so that no GPU test passes vacuously.

  pick_section()  N = 65,793 = 65,536 + 257: 258 parts, the smallest N at which the pick kernel takes a second stride
                  (parts 256, 257 go to threads 0, 1) and whose last workgroup owns a single node. Anchors at the ends
                  of lanes, waves, workgroups and strides; for each criterion and each anchor one configuration in
                  which that anchor wins on that criterion alone and is worse in every later one.
  numa_case()     a make_numa cluster: a policy node (second launch, parts behind all others) and a non-policy node
                  tied through criterion 5, in both index orders.
  key_case()      N = 257: keys whose 64-bit fields differ in one half only, priorities at the ends of int32, 128
                  victims, a lone victim at position 63, 64, 127.
  slot_case()     N = 257: resource slots 2..6 and the pod count as the only binding quantity.
  quota_case()    N = 257, row = -1: quota dimensions 2..7, partial masks, the floor at zero, Error through dimension 4.
  rows_case()     N = 257: hand-written status rows of every word class, nominated nodes, seven rows named out of order.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from koordinator_amd import abi, synth
from oracle import oracle as orc
from tests import fit_diag_util as fd
from tests import preempt_pdb_util as pp
from tests import preempt_util as pu
from tests import value_edges_util as ve

CPU, GI = 1000, 1 << 30
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
TRACKED = abi.GS_RESIDENT_QUOTA_TRACKED
VIOL = 7             # the PDB whose budget is -1: every pod that lists it is violating
FAR = 1 << 50        # a used_limit no case reaches


# ---- the shared builders (tests/test_preempt.py's one-node cases use them too) ----
def flat_cluster(n: int, free_cpu: int = 16 * CPU, pod_count: int = 10, allowed: int = 110) -> synth.Cluster:
    """n identical 16-CPU nodes with free_cpu milli-CPU left: memory never binds, no NodeMetric (LoadAware passes),
    nothing in the assign cache, one pending pod for pod_of to copy."""
    c = synth.make_cluster(n, 1, 0)
    nd = c.nodes
    nd["allocatable"][:] = 0
    nd["allocatable"][:, :3] = (16 * CPU, 64 * GI, 500 * GI)
    nd["requested"][:] = 0
    nd["requested"][:, 0] = 16 * CPU - free_cpu
    nd["nonzero_requested"][:, 0] = nd["requested"][:, 0]
    nd["nonzero_requested"][:, 1] = 0
    nd["pod_count"], nd["allowed_pod_number"] = pod_count, allowed
    nd["raw_allocatable_mask"] = nd["custom_flags"] = 0
    c.metrics["exists"] = 0
    c.assigned_pods = c.assigned_pods[:0]
    return c


def one_node(free_cpu: int):
    """A 16-CPU node with free_cpu milli-CPU left (memory never binds, no NodeMetric: LoadAware passes), the oracle in
    that state, and a pod builder."""
    c = flat_cluster(1, free_cpu)
    o = orc.Oracle(fd.make_cfg(c, False))
    synth.load_into(o, c)
    return c, o


def pod_of(c, cpu: int):
    p = c.pods[0].copy()
    p["requests"][:] = 0
    p["requests"][0] = p["nonzero_requests"][0] = cpu
    p["requests"][1] = p["nonzero_requests"][1] = GI
    p["limits"][:] = p["requests"]
    p["request_mask"] = 3
    return p


def resident(uid, cpu, prio, start=0, quota=pu.QUOTA, flags=TRACKED):
    r = np.zeros(1, abi.RESIDENT_POD_DTYPE)[0]
    r["uid"], r["start_time_ns"], r["priority"], r["quota"], r["flags"] = uid, start, prio, quota, flags
    r["requests"][0] = r["quota_request"][0] = cpu
    r["quota_request_mask"] = 1
    return r


def slot_pod(c, slots: dict, cpu: int = 0, mem: int = 0):
    """A pod that requests the given resource slots (and cpu / memory only when given): the classes of
    value_edges_util's pods (batch slots: Batch priority, mid slots: Mid)."""
    p = c.pods[0].copy()
    prio = abi.GS_PRIO_BATCH if set(slots) & {3, 4} else abi.GS_PRIO_MID if set(slots) & {5, 6} else abi.GS_PRIO_PROD
    ve._set_pod(p, cpu, mem, nz=(cpu or ve.DEF_CPU, mem or ve.DEF_MEM), mask=(1 if cpu else 0) | (2 if mem else 0),
                prio=prio, **{f"s{s}": v for s, v in slots.items()})
    return p


# ---- a case under construction ----
class Builder:
    """Residents, preemptors and expectations of one case on a flat cluster (or a given one)."""

    def __init__(self, n: int, c: synth.Cluster | None = None, numa: bool = False):
        self.c = c if c is not None else flat_cluster(n, allowed=1000)
        self.numa = numa
        self.node_idx, self.res, self.pdb = [], [], []
        self.pre, self.names, self.expect = [], [], []
        self.count = np.zeros(self.c.num_nodes, np.int64)
        self._uid, self._quota, self._node = 0, 100, 256

    def alloc(self, k: int = 1) -> list[int]:
        """k nodes no scenario has used, ascending; over the case they spread across both workgroups of 257 nodes"""
        out = []
        for _ in range(k):
            out.append(self._node)
            self._node = (self._node + 5) % 257
        return sorted(out)

    def quota(self) -> int:
        self._quota += 1
        return self._quota

    def full(self, node: int, slot: int = 0) -> None:
        nd = self.c.nodes
        nd["requested"][node, slot] = nd["allocatable"][node, slot]
        if slot < 2:
            nd["nonzero_requested"][node, slot] = nd["requested"][node, slot]

    def put(self, node: int, prio: int, cpu: int = 0, start: int = 0, quota: int = pu.QUOTA, flags: int = TRACKED,
            pdb=(), req: dict | None = None, qreq: dict | None = None, qmask: int | None = None) -> int:
        """One resident; req: {slot: request} beside cpu; qreq: {dimension: quota request} (default: dimension 0 = cpu),
        qmask: its quota_request_mask (default: the keys of qreq)."""
        self._uid += 1
        r = resident(self._uid * 7919 + 11, cpu, prio, start, quota, flags)
        for s, v in (req or {}).items():
            r["requests"][s] = v
        if qreq is not None:
            r["quota_request"][:] = 0
            r["quota_request_mask"] = 0
            for d, v in qreq.items():
                r["quota_request"][d] = v
                r["quota_request_mask"] |= 1 << d
        if qmask is not None:
            r["quota_request_mask"] = qmask
        self.node_idx.append(node)
        self.res.append(r)
        ids = list(pdb) + [pp.NONE] * (abi.GS_MAX_POD_PDBS - len(pdb))
        self.pdb.append(ids)
        self.count[node] += 1
        return int(r["uid"])

    def preemptor(self, name: str, pod, quota: int, used=(0, 0), limit=(FAR, FAR), row: int = -1, expect=None,
                  dims: dict | None = None, **kw) -> int:
        """dims: {dimension: (request, used, limit)} beyond cpu / memory, each joining both masks"""
        p = pu.make_preemptor(pod, row, used, limit, quota=quota, **kw)
        for d, (q, u, lim) in (dims or {}).items():
            p["quota_request"][d], p["used"][d], p["used_limit"][d] = q, u, lim
            p["quota_request_mask"] |= 1 << d
            p["limit_mask"] |= 1 << d
        self.pre.append(p)
        self.names.append(name)
        self.expect.append(expect or {})
        return len(self.pre) - 1

    def case(self, rows=None) -> "EdgeCase":
        nd = self.c.nodes
        nd["pod_count"] = np.maximum(nd["pod_count"], self.count)
        base = pu.Case(self.c, self.numa, 0, np.array(self.node_idx, np.uint32), np.array(self.res, abi.RESIDENT_POD_DTYPE),
                       rows, np.stack(self.pre))
        pdb = pp.PdbCase(base, base.preemptors, np.array(self.pdb, np.uint16).reshape(-1, abi.GS_MAX_POD_PDBS),
                         np.array([VIOL], np.uint32), np.array([-1], np.int32))
        return EdgeCase(base, pdb, list(self.names), list(self.expect))


@dataclasses.dataclass
class EdgeCase:
    base: pu.Case
    pdb: pp.PdbCase
    names: list
    expect: list          # per preemptor: {"node", "crit", "pdb_crit", "status": {node: status}, "bits": {node: [w0, w1]},
                          #                 "result", "only", "nviol": {node: count}}

    def k(self, name: str) -> int:
        return self.names.index(name)

    def ks(self, prefix: str = "") -> list[int]:
        return [k for k, n in enumerate(self.names) if n.startswith(prefix)]


def check_expect(ec: EdgeCase, k: int, a, b) -> None:
    """What preemptor k was built for, on the plain truth a and the PDB truth b."""
    e, name = ec.expect[k], ec.names[k]
    for node, st in e.get("status", {}).items():
        assert a.node_status[node] == st and b.node_status[node] == st, (name, node, a.node_status[node], b.node_status[node], st)
    for node, w in e.get("bits", {}).items():
        assert a.victim_bits[node].tolist() == w and b.victim_bits[node].tolist() == w, (name, node, a.victim_bits[node])
    for node, n in e.get("nviol", {}).items():
        assert int(b.pdb_violations[node]) == n, (name, node, b.pdb_violations[node])
    if "node" in e:
        assert a.node == e["node"] and b.node == e.get("pdb_node", e["node"]), (name, a.node, b.node, e["node"])
    if "crit" in e:
        assert a.decided_at == e["crit"] and b.decided_at == e.get("pdb_crit", e["crit"]), (name, a.decided_at, b.decided_at)
    if "result" in e:
        assert a.status == e["result"] and b.status == e["result"], (name, a.status, b.status)
    if "only" in e:
        assert a.only_bits == e["only"], (name, a.only_bits, e["only"])


# ---- the pick order with one criterion dropped or inverted ----
# criterion -> (field of the PDB-form key (node, nviol, first, sum, nvict, earliest), the better end)
STEPS = {1: (1, min), 2: (2, min), 3: (3, min), 4: (4, min), 5: (5, max), 6: (0, min)}


def pick_order(cands, drop: int | None = None, invert: int | None = None) -> int:
    """The node pickOneNodeForPreemption's order nominates with criterion `drop` left out or criterion `invert` read
    the other way round; cands in PDB form, ascending node. With criterion 6 dropped nothing orders what remains: the
    last one is taken, as a reduction does that keeps the later of two equal keys."""
    alive = list(cands)
    for crit in range(1, 7):
        if crit == drop:
            continue
        f, best = STEPS[crit]
        if crit == invert:
            best = max if best is min else min
        b = best(c[f] for c in alive)
        alive = [c for c in alive if c[f] == b]
    return alive[-1][0] if drop == 6 else alive[0][0]


def pdb_form(cands) -> list:
    """preempt_util's keys (node, first, sum, nvict, earliest) in PDB form, no violation anywhere"""
    return [(c[0], 0) + tuple(c[1:]) for c in cands]


# ---- 1. pick positions x criteria at N = 65,793 ----
PICK_N = 65_793
ANCHORS = (0, 63, 64, 255, 256, 16_383, 16_384, 65_535, 65_536, 65_792)
PICK_CPU = 6 * CPU
BATCH = 8            # preemptors per call at this N (the detail arrays are 17 bytes per preemptor and node)
PICK_BATCHES = 8     # 60 criterion x anchor configurations, the Error one and the no-candidate one
# criterion -> (the others' victims, the winner's victims) as (priority, start): the winner is strictly better in the
# criterion, tied before it and strictly worse in every later one (more victims / a larger sum / an earlier start; the
# node index only where the winner is not the lowest anchor). Sums: a victim adds priority + 2^31.
#   3: others 990 + 0 -> 990 + 2^32; winner 990 + two at INT32_MIN + 5 -> 990 + 2^31 + 10
#   4: others 990 + two at -2^30 -> 990 + 2^32; winner 990 + 0 -> the same sum with fewer victims
SHAPES = {
    1: ([(990, 1000)], [(991, 500), (991, 600)]),          # PDB call: the others' victim is violating, the winner's are not
    2: ([(990, 1000)], [(989, 500), (989, 600)]),
    3: ([(990, 1000), (0, 1000)], [(990, 500), (INT32_MIN + 5, 1), (INT32_MIN + 5, 2)]),
    4: ([(990, 1000), (-(1 << 30), 1), (-(1 << 30), 2)], [(990, 500), (0, 1)]),
    5: ([(990, 1000)], [(990, 2000)]),
    6: ([(990, 1000)], [(990, 1000)]),
}


@dataclasses.dataclass
class PickConfig:
    name: str
    crit: int            # the criterion built to decide (0: the Error / no-candidate configurations)
    winner: int          # the anchor built to win, -1: none
    present: tuple       # the anchors that hold residents
    quota: int


class PickSection:
    """One cluster, one oracle and one truth for all configurations; `batches` of at most BATCH configurations, each a
    pu.Case / pp.PdbCase over the same oracle whose table holds that batch's residents only (the GPU test switches
    with node_pods_add / node_pods_remove on one engine)."""

    def __init__(self):
        c = flat_cluster(PICK_N, allowed=1000)
        for a in ANCHORS:
            c.nodes["requested"][a, 0] = c.nodes["nonzero_requested"][a, 0] = 16 * CPU
        c.nodes["pod_count"][list(ANCHORS)] = 100
        self.c = c
        self.configs: list[PickConfig] = []
        per_config = []       # (node_idx, residents, pdb lists, preemptor)
        uid = [0]

        def add(name, crit, winner, shapes: dict, used=(0, 0), limit=(FAR, FAR), viol=()):
            """shapes: {anchor: [(priority, start, cpu)]}; viol: the anchors whose first victim lists VIOL"""
            q = 100 + len(self.configs)
            idx, res, ids = [], [], []
            for a, vs in shapes.items():
                for j, (prio, start, cpu) in enumerate(vs):
                    uid[0] += 1
                    idx.append(a)
                    res.append(resident(uid[0] * 7919 + 5, cpu, prio, start, q))
                    ids.append([VIOL if (j == 0 and a in viol) else pp.NONE] + [pp.NONE] * 3)
            pre = pu.make_preemptor(pod_of(c, PICK_CPU), -1, used, limit, quota=q)
            self.configs.append(PickConfig(name, crit, winner, tuple(shapes), q))
            per_config.append((idx, res, ids, pre))

        def spread(vs):
            return [(p, s, PICK_CPU // len(vs)) for p, s in vs]

        for crit in range(1, 6):
            others, win = SHAPES[crit]
            for w in ANCHORS:
                shapes = {a: spread(win if a == w else others) for a in ANCHORS}
                viol = [a for a in ANCHORS if a != w] if crit == 1 else ANCHORS
                add(f"c{crit}-w{w}", crit, w, shapes, viol=viol)
        for j, w in enumerate(ANCHORS):      # criterion 6: the lowest anchor present; anchors j.. are present
            add(f"c6-w{w}", 6, w, {a: spread(SHAPES[6][0]) for a in ANCHORS[j:]}, viol=ANCHORS)
        # every anchor's victim is removed twice (the Filter, then the quota): Error everywhere, no candidate
        add("error", 0, -1, {a: [(990, 1000, PICK_CPU)] for a in ANCHORS}, used=(PICK_CPU, 0), limit=(PICK_CPU - 1, FAR))
        # no candidate and no error: every second anchor cannot hold the pod with its only potential victim gone
        add("nocand", 0, -1, {a: [(990, 1000, CPU)] for a in ANCHORS[::2]})

        o, nodes, _ = pu.end_state(c, False, 0)
        self.batches: list[EdgeCase] = []
        for b in range(0, len(self.configs), BATCH):
            part = per_config[b:b + BATCH]
            idx = np.array(sum((p[0] for p in part), []), np.uint32)
            res = np.array(sum((p[1] for p in part), []), abi.RESIDENT_POD_DTYPE)
            ids = np.array(sum((p[2] for p in part), []), np.uint16)
            base = pu.Case(c, False, 0, idx, res, None, np.stack([p[3] for p in part]))
            base._state = (o, nodes, base.table())
            pdb = pp.PdbCase(base, base.preemptors, ids, np.array([VIOL], np.uint32), np.array([-1], np.int32))
            self.batches.append(EdgeCase(base, pdb, [cf.name for cf in self.configs[b:b + BATCH]], [{}] * len(part)))

    def config_of(self, b: int, k: int) -> PickConfig:
        return self.configs[b * BATCH + k]

    def answers(self, b: int):
        """(plain truth, PDB truth) of batch b's configurations, computed once"""
        ks = list(range(len(self.batches[b].names)))
        return self.batches[b].base.answers(ks), self.batches[b].pdb.answers(ks)


@functools.lru_cache(maxsize=None)
def pick_section() -> PickSection:
    return PickSection()


# ---- 2. the pick across the two launches (NUMA profile) ----
NUMA_N = 300
NUMA_CPU = 2 * CPU


def _numa_cluster() -> synth.Cluster:
    c = synth.make_cluster(NUMA_N, 1, 0)
    synth.make_numa(c)
    c.metrics["exists"] = 0                   # LoadAware passes everywhere
    c.assigned_pods = c.assigned_pods[:0]
    c.nodes["allowed_pod_number"] = 1000
    return c


def numa_pod(c):
    """A plain LS pod of NUMA_CPU: no cpuset, no bind policy"""
    p = pod_of(c, NUMA_CPU)
    p["priority_class"], p["qos_class"] = abi.GS_PRIO_PROD, abi.GS_QOS_LS
    p["required_cpu_bind_policy"] = p["preferred_cpu_bind_policy"] = p["preferred_cpu_exclusive_policy"] = 0
    return p


def _numa_builder(nodes, quotas) -> Builder:
    """Each of `nodes` full in CPU with one potential victim of NUMA_CPU; node i's resident has quota quotas[i]"""
    c = _numa_cluster()
    b = Builder(NUMA_N, c, numa=True)
    for i, q in zip(nodes, quotas):
        b.full(i)
        b.put(i, 990, NUMA_CPU, 1000, q)
    return b


@functools.lru_cache(maxsize=None)
def numa_case() -> EdgeCase:
    """Two preemptors: "policy-low" whose two candidates are a policy node and a higher-indexed non-policy node,
    "policy-high" with the policy node at the higher index; each pair identical in every key field but the node. The
    nodes are found by a probe run of the truth over the first and last policy / non-policy nodes: a policy node that
    fails NodeNUMAResource for a reason of its own is passed over."""
    c = _numa_cluster()
    policy = c.numa["node_numa"]["numa_topology_policy"] != abi.GS_NUMA_POLICY_NONE
    pol, non = np.nonzero(policy)[0].tolist(), np.nonzero(~policy)[0].tolist()
    probe_nodes = sorted(set(pol[:8] + pol[-8:] + non[:4] + non[-4:]))
    b = _numa_builder(probe_nodes, [1] * len(probe_nodes))
    b.preemptor("probe", numa_pod(b.c), 1)
    a, = b.case().base.answers([0])
    ok = [i for i in probe_nodes if a.node_status[i] == pu.CANDIDATE]
    ok_pol, ok_non = [i for i in ok if policy[i]], [i for i in ok if not policy[i]]
    low = (ok_pol[0], ok_non[-1])         # the policy node below the non-policy node
    high = (ok_non[0], ok_pol[-1])        # ... and above it
    assert low[0] < low[1] and high[0] < high[1] and len(set(low + high)) == 4
    b = _numa_builder(low + high, [1, 1, 2, 2])
    tied = {"crit": 6, "result": abi.GS_PREEMPT_NOMINATED}
    b.preemptor("policy-low", numa_pod(b.c), 1,
                expect=dict(tied, node=low[0], status={low[0]: pu.CANDIDATE, low[1]: pu.CANDIDATE}))
    b.preemptor("policy-high", numa_pod(b.c), 2,
                expect=dict(tied, node=high[0], status={high[0]: pu.CANDIDATE, high[1]: pu.CANDIDATE}))
    return b.case()


# ---- 3. key values ----
@functools.lru_cache(maxsize=None)
def key_case() -> EdgeCase:
    b = Builder(257)
    P, S = 3 * CPU, 1 << 20
    CAND = pu.CANDIDATE

    def pair(name, lo, hi, win, crit, cpu=P, prio=pu.PRIO):
        """Two full nodes with victims lo / hi [(priority, start)] on the lower / higher index, all of them victims"""
        n_lo, n_hi = b.alloc(2)
        q = b.quota()
        for node, vs in ((n_lo, lo), (n_hi, hi)):
            b.full(node)
            for p, s in vs:
                b.put(node, p, cpu // len(vs), s, q)
        b.preemptor(name, pod_of(b.c, cpu), q, priority=prio,
                    expect=dict(node=n_lo if win == "lo" else n_hi, crit=crit, status={n_lo: CAND, n_hi: CAND},
                                result=abi.GS_PREEMPT_NOMINATED))
        return n_lo, n_hi, q

    # sums exactly 2^32 apart: a compare on the low word ties and falls through to the later start and the lower
    # index, both on the other node
    pair("sum-high", [(990, S + 10), (0, 1), (0, 2)], [(990, S), (INT32_MIN, 1), (INT32_MIN, 2)], "hi", 3)
    # sums one apart, equal high words
    pair("sum-low", [(990, S + 10), (5, 1), (5, 2)], [(990, S), (5, 1), (4, 2)], "hi", 3)
    # the latest earliest start wins; the loser has the lower index
    pair("earliest-above-32", [(990, (1 << 32) + 7)], [(990, (1 << 33) + 7)], "hi", 5)
    pair("earliest-below-32", [(990, (1 << 40) + 5)], [(990, (1 << 40) + 9)], "hi", 5)
    pair("earliest-0-1", [(990, 0)], [(990, 1)], "hi", 5)
    pair("earliest-2^62", [(990, (1 << 62) - 1)], [(990, 1 << 62)], "hi", 5)
    pair("earliest-halves-disagree", [(990, (1 << 33) + 1)], [(990, (1 << 32) + 9)], "lo", 5)
    # signed priorities: the lower first priority wins
    pair("first-minus-1", [(0, S)], [(-1, S)], "hi", 2)
    pair("first-int32-min", [(INT32_MIN + 1, S)], [(INT32_MIN, S)], "hi", 2)
    # a preemptor at INT32_MAX: INT32_MAX - 1 is below it, INT32_MAX is not; at INT32_MIN nothing is below it
    n_lo, n_hi = b.alloc(2)
    q = b.quota()
    for node, p in ((n_lo, INT32_MAX - 1), (n_hi, INT32_MAX)):
        b.full(node)
        b.put(node, p, P, S, q)
    b.preemptor("preemptor-int32-max", pod_of(b.c, P), q, priority=INT32_MAX,
                expect=dict(node=n_lo, crit=0, status={n_lo: CAND, n_hi: pu.NO_VICTIMS}))
    b.preemptor("preemptor-int32-min", pod_of(b.c, P), q, priority=INT32_MIN,
                expect=dict(node=-1, status={n_lo: pu.NO_VICTIMS, n_hi: pu.NO_VICTIMS}, result=abi.GS_PREEMPT_NO_CANDIDATES))
    # 128 victims against one victim of a higher first priority
    n_lo, n_hi = b.alloc(2)
    q = b.quota()
    b.full(n_lo)
    b.full(n_hi)
    for j in range(128):
        b.put(n_lo, 900, 100, 1000 + j * 37 % 128, q)
    b.put(n_hi, 950, 12_800, S, q)
    ones = (1 << 64) - 1
    b.preemptor("128-victims", pod_of(b.c, 12_800), q,
                expect=dict(node=n_lo, crit=2, status={n_lo: CAND, n_hi: CAND}, bits={n_lo: [ones, ones]}))
    # a lone victim at position 63, 64, 127 of 128 residents (position j: priority 2000 - j). "alone": the others are
    # non-preemptible or of another quota, and the victim lists VIOL (the PDB call's lone violating victim).
    # "reprieved": all 128 are potential victims; the 8-CPU pod at the position fails its reprieve, every 10-milli
    # pod fits (the last one with nothing left)
    for pos in (63, 64, 127):
        for kind in ("alone", "reprieved"):
            node, = b.alloc(1)
            q = b.quota()
            b.full(node)
            for j in range(128):
                if j == pos:
                    b.put(node, 2000 - j, 8 * CPU, S, q, pdb=(VIOL,) if kind == "alone" else ())
                elif kind == "reprieved":
                    b.put(node, 2000 - j, 10, S, q)
                else:
                    b.put(node, 2000 - j, 10, S, q if j % 2 else 9999, flags=TRACKED | (abi.GS_RESIDENT_NON_PREEMPTIBLE if j % 2 else 0))
            w = [1 << pos, 0] if pos < 64 else [0, 1 << (pos - 64)]
            b.preemptor(f"lone-{pos}-{kind}", pod_of(b.c, 8 * CPU), q, priority=5000,
                        expect=dict(node=node, crit=0, status={node: CAND}, bits={node: w},
                                    nviol={node: 1 if kind == "alone" else 0}))
    return b.case()


# ---- 4. resource slots and the pod count ----
SLOT_Q = {2: ve.E_EPH, 3: ve.BE_CPU, 4: ve.BE_MEM, 5: ve.MID_CPU, 6: ve.MID_MEM}


@functools.lru_cache(maxsize=None)
def slot_case() -> EdgeCase:
    b = Builder(257)
    nd = b.c.nodes
    for s, q in SLOT_Q.items():
        bit = abi.GS_FAIL_FIT_EPHEMERAL if s == 2 else abi.GS_FAIL_FIT_SCALAR
        quota = b.quota()
        cand, unfit, fits, pair = b.alloc(4)
        for node in (cand, unfit, fits, pair):
            nd["allocatable"][node, s] = 4 * q
            b.full(node, s)
        b.put(cand, 990, req={s: q}, quota=quota)             # gone: q free; back: 0 free
        b.put(unfit, 990, req={s: q - 1}, quota=quota)        # gone: one unit too little
        nd["requested"][fits, s] = 3 * q
        b.put(fits, 990, req={s: q}, quota=quota)             # q free with everybody back
        b.put(pair, 990, req={s: q}, quota=quota)             # back: q - 1 free, one unit too little
        b.put(pair, 980, req={s: q - 1}, quota=quota)         # back: q free, exactly enough
        b.preemptor(f"slot-{s}", slot_pod(b.c, {s: q}), quota,
                    expect=dict(status={cand: pu.CANDIDATE, unfit: pu.UNFIT, fits: pu.FITS, pair: pu.CANDIDATE},
                                bits={cand: [1, 0], pair: [1, 0]}, only=bit))
    # the pod count alone: the node is at allowed_pod_number with everything free
    node, = b.alloc(1)
    quota = b.quota()
    nd["pod_count"][node] = nd["allowed_pod_number"][node] = 20
    b.put(node, 990, quota=quota)
    b.preemptor("pods-only", pod_of(b.c, 100), quota,
                expect=dict(node=node, status={node: pu.CANDIDATE}, bits={node: [1, 0]}, only=abi.GS_FAIL_FIT_PODS))
    # cpu, memory and mid-cpu together: each of the three reprieves fails on another slot
    node, = b.alloc(1)
    quota = b.quota()
    nd["allocatable"][node, 5] = 2 * ve.MID_CPU
    for s in (0, 1, 5):
        b.full(node, s)
    b.put(node, 990, 2 * CPU, quota=quota)
    b.put(node, 980, req={1: 2 * GI}, quota=quota)
    b.put(node, 970, req={5: ve.MID_CPU}, quota=quota)
    b.preemptor("three-slots", slot_pod(b.c, {5: ve.MID_CPU}, 2 * CPU, 2 * GI), quota,
                expect=dict(node=node, status={node: pu.CANDIDATE}, bits={node: [7, 0]},
                            only=abi.GS_FAIL_FIT_CPU | abi.GS_FAIL_FIT_MEMORY | abi.GS_FAIL_FIT_SCALAR))
    return b.case()


# ---- 5. quota dimensions and masks ----
@functools.lru_cache(maxsize=None)
def quota_case() -> EdgeCase:
    """row = -1; the nodes are free unless said otherwise, so a victim is the quota's doing."""
    b = Builder(257)
    pod = pod_of(b.c, CPU)
    for d in range(2, 8):
        node, = b.alloc(1)
        q = b.quota()
        b.put(node, 990, quota=q, qreq={d: 10})
        dims = {d: (10, 95, 100)}        # gone: 85; back: 95, and 95 + 10 exceeds 100
        b.preemptor(f"dim-{d}", pod, q, dims=dims, expect=dict(node=node, status={node: pu.CANDIDATE}, bits={node: [1, 0]}))
        k = b.preemptor(f"dim-{d}-no-limit-key", pod, q, dims=dims, expect=dict(node=-1, status={node: pu.FITS}))
        b.pre[k]["limit_mask"] = 3
        k = b.preemptor(f"dim-{d}-no-request-key", pod, q, dims=dims, expect=dict(node=-1, status={node: pu.FITS}))
        b.pre[k]["quota_request_mask"] = 3
    # a resident's value outside its own mask is no key of its request: `used` stays (moved by it, dimension 3 would
    # fall to 0 and come back as 10^9)
    node, = b.alloc(1)
    q = b.quota()
    b.put(node, 990, quota=q, qreq={2: 10, 3: 10**9}, qmask=1 << 2)
    b.preemptor("outside-own-mask", pod, q, dims={2: (10, 50, 100), 3: (10, 50, 100)},
                expect=dict(node=-1, status={node: pu.FITS}))
    # the floor at zero in dimension 5: used 1, the victim's 4 leave: 0, not -3; back: 4, and 4 + 2 exceeds 5 (1 + 2
    # would not). The untracked twin leaves `used` at 1
    tracked, untracked = b.alloc(2)
    q = b.quota()
    b.put(tracked, 990, quota=q, qreq={5: 4})
    b.put(untracked, 990, quota=q, qreq={5: 4}, flags=0)
    b.preemptor("floor-dim-5", pod, q, dims={5: (2, 1, 5)},
                expect=dict(node=tracked, status={tracked: pu.CANDIDATE, untracked: pu.FITS}))
    # a preemptor without a quota: its residents are the pods without one; `used` is left alone and never checked
    full, free = b.alloc(2)
    b.full(full)
    b.put(full, 990, CPU, quota=-1)
    b.put(free, 990, CPU, quota=-1)
    b.preemptor("skip", pod, -1, used=(99 * CPU, 0), limit=(0, 0), dims={4: (10, 100, 0)},
                expect=dict(node=full, status={full: pu.CANDIDATE, free: pu.FITS}))
    # Error through dimension 4: the Filter removes the victim, and the quota still exceeds (90 + 20 > 105)
    node, = b.alloc(1)
    q = b.quota()
    b.full(node)
    b.put(node, 990, CPU, quota=q, qreq={4: 10})
    b.preemptor("error-dim-4", pod, q, dims={4: (20, 100, 105)},
                expect=dict(node=-1, status={node: pu.ERROR}, result=abi.GS_PREEMPT_ERROR))
    return b.case()


# ---- 6. rows ----
ROW_CLASS, ROW_OTHER, ROW_UNRES, NUM_ROWS = 5, 2, 3, 7
LA = abi.GS_FAIL_LOADAWARE


def class_words() -> list[int]:
    """Every word class, one word per consecutive node: the NUMA reasons 0..15 alone, with a Fit bit, with LoadAware;
    the malformed LoadAware words (its memory / aggregated flags without its bit); bits above the code."""
    sh = abi.GS_FAIL_NUMA_SHIFT
    w = [r << sh for r in range(16)]
    w += [(r << sh) | (abi.GS_FAIL_FIT_PODS, abi.GS_FAIL_FIT_CPU, abi.GS_FAIL_FIT_MEMORY, abi.GS_FAIL_FIT_EPHEMERAL,
                       abi.GS_FAIL_FIT_SCALAR)[r % 5] for r in range(16)]
    w += [(r << sh) | LA for r in range(16)]
    w += [abi.GS_FAIL_LA_MEMORY, abi.GS_FAIL_LA_AGGREGATED, abi.GS_FAIL_LA_MEMORY | abi.GS_FAIL_LA_AGGREGATED,
          (5 << sh) | abi.GS_FAIL_LA_MEMORY, (9 << sh) | abi.GS_FAIL_LA_AGGREGATED,
          (2 << sh) | abi.GS_FAIL_LA_MEMORY | abi.GS_FAIL_LA_AGGREGATED]
    w += [(r << sh) | 0xF000 for r in (0, 1, 4, 5, 9, 15)] + [(5 << sh) | 0x8000 | abi.GS_FAIL_FIT_SCALAR]
    return w


CLASS_AT = 100       # the first node of the class row's designed words
ROW_KS = ("row-5-a", "row-2", "row-5-b", "row-none")      # the call that names rows 5, 2, 5, -1 in that order


@functools.lru_cache(maxsize=None)
def rows_case() -> EdgeCase:
    b = Builder(257)
    P = 2 * CPU
    pod = pod_of(b.c, P)
    words = class_words()
    sh = abi.GS_FAIL_NUMA_SHIFT
    unres, resolvable = 5 << sh, abi.GS_FAIL_FIT_CPU
    rows = np.full((NUM_ROWS, 257), resolvable, np.uint16)
    rows[ROW_CLASS, CLASS_AT:CLASS_AT + len(words)] = words
    rows[ROW_OTHER, ::3] = unres
    rows[ROW_UNRES] = [(1, 2, 3, 5, 6, 7, 9)[i % 7] << sh for i in range(257)]
    rows[0] = rows[1] = rows[4] = rows[6] = 0xFFFF      # rows no preemptor names
    q = b.quota()
    for i in range(CLASS_AT, CLASS_AT + len(words)):      # each would be a candidate
        b.full(i)
        b.put(i, 990, P, 1000 + i, q)
    nom = 30                                             # a terminating victim on the nominated node
    b.full(nom)
    b.put(nom, 990, P, 5000, q, flags=TRACKED | abi.GS_RESIDENT_TERMINATING)
    assert rows[ROW_OTHER, nom] == unres and rows[ROW_CLASS, nom] == resolvable
    b.preemptor("row-5-a", pod, q, row=ROW_CLASS)
    b.preemptor("row-2", pod, q, row=ROW_OTHER)
    b.preemptor("row-5-b", pod, q, row=ROW_CLASS, priority=pu.PRIO + 1)
    b.preemptor("row-none", pod, q)
    b.preemptor("nominated-unresolvable", pod, q, row=ROW_OTHER, nominated=nom, expect=dict(result=abi.GS_PREEMPT_NOMINATED))
    b.preemptor("nominated-resolvable", pod, q, row=ROW_CLASS, nominated=nom, expect=dict(result=abi.GS_PREEMPT_NOT_ELIGIBLE))
    b.preemptor("all-unresolvable", pod, q, row=ROW_UNRES, expect=dict(result=abi.GS_PREEMPT_NO_POTENTIAL_NODES, node=-1))
    return b.case(rows)


def alone(ec: EdgeCase, k: int):
    """Preemptor k of a rows case as a call of its own: (preemptor with row 0 or -1, its one row or None)"""
    p = ec.base.preemptors[k:k + 1].copy()
    r = int(p[0]["row"])
    if r < 0:
        return p, None
    p["row"] = 0
    return p, ec.base.rows[r:r + 1]
