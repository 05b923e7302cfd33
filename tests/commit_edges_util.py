"""The speculative commit's edge family (commit_spec_kernel, gs_commit_spec.hip): hand-built inputs, and a classifier
that proves from the CPU oracle alone which of the kernel's paths each pod's decision has to take.

The clusters are flat: every node has CAP = 100,000 milli-CPU, memory that never binds and no NodeMetric; the profile
scores NodeResourcesFit on cpu alone, so a pod of r milli-CPU scores floor((free - r) / 1000) on a node with `free`
milli-CPU left (-1: it does not fit, or the node's pod slots are used up). A uniform background (BG_FREE left: score 4
for every pod of up to 1000 milli-CPU) lies far below a few anchor nodes with designed capacities and pod-slot limits.
Pods come in two sizes: SMALL (10: a landing leaves the row's integer score where it was) and STEP (1000: a landing
lowers it by exactly one point). Where a case needs the tie-break position somewhere, the pod's `seq` is found by a
search over tiebreak_position (restated below from gs_eval_dev.h), pod by pod against the oracle's state.

classify() replays a case with two oracles: one advances pod by pod (evaluate the next pods, schedule one), one is
held at the batch-start state of the pod's batch. From the two score rows of pod q and the nodes earlier pods of its
batch landed on ("dirty", in order of first landing = the kernel's slot index) it derives what decide_core / apply_late
/ the verification see. Nothing here reads device output.

Families (each builder's docstring names the code it aims at): chains(), alternating(), ge_case(), slots_case(),
paths_case(), excl_case(), fiterror_case(), pending_only_case(), hash_case(), and on NodeNUMAResource clusters
undo_case(), hostcut_case(). launch_commit_spec runs the split pipeline on batches of 32 pods or more: every case has
at least 32 pods (fillers behind the designed ones where needed); the single selector gets them in batches under 32 and
on two ranks.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from koordinator_amd import abi, config, numa, synth
from oracle import oracle as orc
from tests import numa_edges_util as nu

FIELDS = ("node", "score", "ties", "feasible")
SEED = 0x6B6F6F7264          # config.make_config's default
CAP, BG_FREE = 100_000, 5_000
SMALL, STEP = 10, 1000
GiB = 1 << 30
# gs_commit_spec.hip / gs_kernels.h
SP_LAG, SP_KW, SP_JOBQ, SP_HASH, MAX_BATCH, LCAP, LEVALL = 12, 4, 24, 128, 128, 2048, 32
M64 = (1 << 64) - 1


# ---- selectHost's tie-break, restated (gs_eval_dev.h tiebreak_position) ----
def _mix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def tiebreak_position(seq: int, T: int, seed: int = SEED) -> int:
    """1-based position among T ties in node order"""
    key = _mix64(seed ^ _mix64(seq))
    j, i = 1, 0
    while True:
        u = float((_mix64((key + i) & M64) >> 11) + 1) * 2.0 ** -53
        x = float(j) / u
        if not x < 4.0e18:
            break
        jn = int(math.floor(x)) + 1
        if jn > T:
            break
        j, i = jn, i + 1
    return j


# ---- clusters and pods ----
def flat(n: int, anchors: dict, slots: dict | None = None, bg_free: int = BG_FREE) -> synth.Cluster:
    """n nodes of CAP milli-CPU with bg_free left; anchors: {node: free}; slots: {node: pods it still takes}"""
    c = synth.make_cluster(n, 1, 0)
    nd = c.nodes
    nd["allocatable"][:] = 0
    nd["allocatable"][:, :3] = (CAP, 1 << 40, 1 << 42)
    nd["requested"][:] = 0
    nd["nonzero_requested"][:] = 0
    nd["requested"][:, 0] = CAP - bg_free
    for node, free in anchors.items():
        nd["requested"][node, 0] = CAP - free
    nd["nonzero_requested"][:, 0] = nd["requested"][:, 0]
    nd["pod_count"], nd["allowed_pod_number"] = 10, 1000
    for node, k in (slots or {}).items():
        nd["allowed_pod_number"][node] = 10 + k
    nd["raw_allocatable_mask"] = nd["custom_flags"] = 0
    c.metrics["exists"] = 0
    c.assigned_pods = c.assigned_pods[:0]
    c.assigned_node = c.assigned_node[:0]
    c.assigned_ts = c.assigned_ts[:0]
    c.pod_metrics = c.pod_metrics[:0]
    c.pm_offsets[:] = 0
    return c


def make_cfg(n: int, **kw) -> abi.GsConfig:
    return config.make_config(n, fit=config.fit_args({"cpu": 1}), **kw)


def pods_of(c: synth.Cluster, cpus) -> np.ndarray:
    """one pod per entry: its milli-CPU, or (milli-CPU, memory); memory defaults to 1 GiB and is never scored"""
    out = np.repeat(c.pods[:1], len(cpus))
    for i, cpu in enumerate(cpus):
        cpu, mem = cpu if isinstance(cpu, tuple) else (cpu, GiB)
        p = out[i]
        p["uid"] = p["name_key"] = 1000 + i
        p["requests"][:] = 0
        p["requests"][0] = p["nonzero_requests"][0] = cpu
        p["requests"][1] = p["nonzero_requests"][1] = mem
        p["limits"][:] = p["requests"]
        p["request_mask"] = 3
        p["priority_class"], p["qos_class"], p["flags"] = abi.GS_PRIO_PROD, abi.GS_QOS_LS, 0
        p["required_cpu_bind_policy"] = p["preferred_cpu_bind_policy"] = p["preferred_cpu_exclusive_policy"] = 0
    return out


WIDE = (1, 4, 40, 1)   # 160 single-CPU cores: outside the device cpuset scope (TopoDev.ok: <= 128 cores), the host selects


def load_numa(e, nodes) -> None:
    """numa_edges_util.load with two topologies: nodes of family "wide" have 4 zones of 40 single-CPU cores (their
    cpusets are the host's to select: the commit ends the batch after such a pod), the others its 4 x 4 x 2 topology"""
    N = len(nodes)
    recs = np.zeros(N, abi.NODE_DTYPE)
    for i, nd in enumerate(nodes):
        ncpus = 160 if nd.family == "wide" else nu.NCPUS
        recs[i]["allocatable"][abi.GS_RES_CPU] = 4 * ncpus * 1000
        recs[i]["allocatable"][abi.GS_RES_MEMORY] = nu.MAX_EXACT
        recs[i]["allowed_pod_number"] = 400
        held = sum(len(a.cpus) for a in nd.allocs) * 1000
        recs[i]["requested"][abi.GS_RES_CPU] = recs[i]["nonzero_requested"][0] = held
    e.set_now(0)
    e.upsert_nodes(recs)
    e.upsert_metrics(np.zeros(N, abi.METRIC_DTYPE))
    tid = {"": e.register_topology(numa.test_topology(*nu.TOPO))}
    if any(nd.family == "wide" for nd in nodes):
        tid["wide"] = e.register_topology(numa.test_topology(*WIDE))
    nrecs, allocs, alloc_nodes = [], [], []
    for i, nd in enumerate(nodes):
        zones = [(z, c, m) for z, (c, m) in enumerate(nd.zones)]
        nrecs.append(numa.node_numa(tid.get(nd.family, tid[""]), zones=zones, numa_policy=nd.policy))
        for j, a in enumerate(nd.allocs):
            allocs.append(numa.pod_allocation(0xA110C000 + 256 * i + j, a.cpus, a.numa))
            alloc_nodes.append(i)
    e.upsert_numa(np.array(nrecs, abi.NODE_NUMA_DTYPE))
    if allocs:
        e.update_allocations(np.array(alloc_nodes, np.uint32), np.array(allocs, abi.POD_ALLOCATION_DTYPE))


@dataclasses.dataclass
class Case:
    name: str
    c: object                       # what load() pushes: a synth.Cluster (flat cases) or a node list (NUMA cases)
    pods: np.ndarray
    seq: np.ndarray
    batch: int                      # the batch size the claims are made for (every pod in one call)
    want: np.ndarray                # the oracle's placements
    claims: list                    # (pod, field of its classification ("*": the record), value or predicate)
    slowpath: int | None = None     # pods resolved from their whole row (gs_stats.slowpath_pods), where predicted
    host_pods: tuple = ()           # pods whose cpuset the host selects: each ends its batch (predicted_cuts)
    want_alloc: dict | None = None  # NUMA cases: {pod: allocation bytes or None} of the pods with a Reserve record
    numa: bool = False
    cfg_kw: dict = dataclasses.field(default_factory=dict)   # NUMA cases: plugin weights / NodeNUMAResource args

    @property
    def n(self) -> int:
        return len(self.c) if self.numa else self.c.num_nodes

    def config(self, **kw) -> abi.GsConfig:
        if self.numa:
            return config.make_config(self.n, enabled=abi.GS_ENABLE_ALL, **{**self.cfg_kw, **kw})
        return make_cfg(self.n, **kw)

    def load(self, e) -> None:
        if self.numa:
            load_numa(e, self.c)
        else:
            synth.load_into(e, self.c)

    def oracle(self) -> orc.Oracle:
        o = orc.Oracle(self.config())
        self.load(o)
        return o


class Designer:
    """Builds a case pod by pod against the oracle's state: `seq` chosen so that the tie-break lands where asked.
    c: a flat cluster with cpus = the pods' milli-CPU, or (numa) a node list with cpus = POD_DTYPE records."""

    def __init__(self, c, cpus, numa: bool = False, cfg_kw: dict | None = None):
        self.c, self.numa, self.cfg_kw = c, numa, cfg_kw or {}
        self.pods = np.asarray(cpus) if numa else pods_of(c, cpus)
        self.shell = Case("", c, self.pods, None, MAX_BATCH, None, [], numa=numa, cfg_kw=self.cfg_kw)
        self.o = self.shell.oracle()
        self.seq, self.nodes, self.q = [], [], 0
        self._next = 1

    def row(self, q=None):
        return self.o.evaluate(self.pods[self.q if q is None else q][None])[0][0].astype(np.int64)

    def ties(self, q=None):
        """the ties pod q (default: the next pod) has in the current state"""
        r = self.row(q)
        return np.nonzero(r == r.max())[0] if r.max() >= 0 else np.zeros(0, np.int64)

    def place(self, want=None, also=None) -> int:
        """Schedule the next pod. want: None (any seq), a 1-based tie rank, or a function (ties) -> rank; also: a
        further condition on the seq."""
        t = self.ties()
        T = len(t)
        jp = want(t) if callable(want) else want
        s = self._next
        while T and ((jp is not None and tiebreak_position(s, T) != jp) or (also is not None and not also(s))):
            s += 1
            assert s < self._next + 400_000, "no seq found"
        self._next = s + 1
        out = self.o.schedule(self.pods[self.q][None], np.array([s], np.uint64))[0]
        if T and jp is not None:
            assert out["node"] == t[jp - 1], (self.q, out, t, jp)
        self.seq.append(s)
        self.nodes.append(int(out["node"]))
        self.q += 1
        return int(out["node"])

    def rest(self):
        while self.q < len(self.pods):
            self.place()

    def case(self, name, batch, claims, slowpath=None, host_pods=()) -> Case:
        self.rest()
        seq = np.array(self.seq, np.uint64)
        case = Case(name, self.c, self.pods, seq, batch, None, claims, slowpath, tuple(host_pods), numa=self.numa,
                    cfg_kw=self.cfg_kw)
        o = case.oracle()
        case.want = o.schedule(self.pods, seq)
        assert case.want["node"].tolist() == self.nodes
        if self.numa:
            case.want_alloc = {}
            for j in np.nonzero(case.want["flags"] & (abi.GS_PLACED_CPUSET | abi.GS_PLACED_NUMA))[0]:
                a = o.allocation(int(case.want["node"][j]), int(self.pods["uid"][j]))
                case.want_alloc[int(j)] = None if a is None else a.tobytes()
        return case


def node_rank(want_node):
    """place(want=...): the tie that is node `want_node`"""
    def f(t):
        i = np.nonzero(t == want_node)[0]
        assert len(i) == 1, (want_node, t)
        return int(i[0]) + 1
    return f


# ---- the classifier ----
def _listing(row0, k):
    """cand_kernel's level rule for the pod at batch position k (no stale-level allowance: a call's first batch):
    levels from the top until LEVALL levels, LCAP nodes or k + 1 listed nodes. -> (listed scores, counts, next)"""
    u, cnt = np.unique(row0[row0 >= 0], return_counts=True)
    scores, counts, cum = [], [], 0
    for s, n in zip(u[::-1].tolist(), cnt[::-1].tolist()):
        if len(scores) == LEVALL or cum + n > LCAP or cum >= k + 1:
            return scores, counts, s
        scores.append(s)
        counts.append(n)
        cum += n
    return scores, counts, -1


def _rel(x, m):
    return ">" if x > m else "==" if x == m else "<"


def batches(case: Case, batch: int | None = None) -> list:
    """[b0, b1) of the batches of one call: `batch` pods each, and a batch ends right after a pod whose cpuset the host
    selects (case.host_pods); such a pod that is not its batch's last one cuts it (gs_stats.cuts)"""
    B, P, out, b0 = batch or case.batch, len(case.pods), [], 0
    while b0 < P:
        b1 = min(b0 + B, P)
        hp = [q for q in case.host_pods if b0 <= q < b1]
        if hp:
            b1 = hp[0] + 1
        out.append((b0, b1))
        b0 = b1
    return out


def predicted_cuts(case: Case, batch: int | None = None) -> int:
    B, P = batch or case.batch, len(case.pods)
    return sum(1 for b0, b1 in batches(case, batch) if b1 < min(b0 + B, P))


def classify(case: Case, batch: int | None = None, lags: int = 2) -> list[dict]:
    """Per pod, what the kernel's decision sees (see the module docstring). Fields:
      M, T, F, Mclean, nold, nnew, nd (dirty slots), jp, winner, slot (the winner's; nd: a fresh one), fresh
      listed (level M is listed), e (the winner's list index; None: its batch-start score is not M), nxt, full_row
        (listed / e / nxt / full_row: exact for a call's first batch only)
      prev: {d: (slot, relation, delta)} for d = 1..13: the row pod q-d of the batch landed on, its exact score for q
        against M_excl, the maximum with that row left out (what a decision sees while the row is pending)
      jp_excl: the tie-break position with pod q-1's row left out (None: no such row, or nothing else feasible)
      runner_up: the nodes that decision would choose among ([]: none feasible, a speculative FitError)
      late: {d: (T_s, jp_s, ranks, fresh)} for d = 1..lags: the decision over the state d pods earlier (the split
        selector's snapshot): its ties and position, the 1-based ranks of the late landings' nodes among those ties
        (0: not a tie), and whether each landing made a new slot
      gone: dirty rows feasible at batch start and infeasible now
      new_nodes: dirty rows at M now that were not at batch start; clean_ties: the clean nodes at M
    Asserts the oracle's own consistency: clean rows agree in both states, and M / T / F / winner are its placement."""
    P, N = len(case.pods), case.n
    o_seq, o_bat = case.oracle(), case.oracle()
    out = []
    for b0, b1 in batches(case, batch):
        rows0 = o_bat.evaluate(case.pods[b0:b1])[0].astype(np.int64)
        o_bat.schedule(case.pods[b0:b1], case.seq[b0:b1])
        dirty, landed = [], []       # nodes in slot order; per pod of the batch: the node it landed on (-1: none)
        hist = {}                    # q -> {d: pod q's row at the state d pods earlier}
        for q in range(b0, b1):
            ahead = min(lags + 1, b1 - q)
            rows = o_seq.evaluate(case.pods[q:q + ahead])[0].astype(np.int64)
            for d in range(1, ahead):
                hist.setdefault(q + d, {})[d] = rows[d]
            row1, row0, k = rows[0], rows0[q - b0], q - b0
            pl = o_seq.schedule(case.pods[q:q + 1], case.seq[q:q + 1])[0]
            clean = np.ones(N, bool)
            clean[dirty] = False
            assert (row1[clean] == row0[clean]).all(), (case.name, q)
            M, seq = int(row1.max()), int(case.seq[q])
            ties = np.nonzero(row1 == M)[0] if M >= 0 else np.zeros(0, np.int64)
            T, F = len(ties), int((row1 >= 0).sum())
            r = {"M": M, "T": T, "F": F, "nd": len(dirty), "Mclean": int(row1[clean].max()) if clean.any() else -1,
                 "nold": sum(1 for n in dirty if row0[n] == M and M >= 0),
                 "nnew": sum(1 for n in dirty if row1[n] == M and M >= 0),
                 "gone": [n for n in dirty if row0[n] >= 0 > row1[n]],
                 "new_nodes": sorted(n for n in dirty if row1[n] == M and row0[n] != M and M >= 0),
                 "clean_ties": np.nonzero(clean & (row1 == M))[0].tolist() if M >= 0 else []}
            w = int(pl["node"])
            if M >= 0:
                r["jp"] = tiebreak_position(seq, T)
                assert w == ties[r["jp"] - 1] and pl["score"] == M and pl["ties"] == T, (case.name, q, pl, M, T)
            else:
                r["jp"] = 0
                assert w < 0, (case.name, q, pl)
            assert pl["feasible"] == F, (case.name, q, pl, F)
            r["winner"] = w
            r["fresh"] = w >= 0 and w not in dirty
            r["slot"] = -1 if w < 0 else dirty.index(w) if w in dirty else len(dirty)
            scores, counts, nxt = _listing(row0, k)
            r["nxt"], r["listed"] = nxt, M in scores
            r["full_row"] = not (M < 0 and nxt < 0) and M <= nxt
            r["e"] = None
            if w >= 0 and r["listed"] and row0[w] == M:
                r["e"] = sum(n for s, n in zip(scores, counts) if s > M) + int((row0[:w] == M).sum())
            r["prev"] = {}
            for d in range(1, min(13, k) + 1):
                n = landed[k - d]
                if n < 0:
                    continue
                x = int(row1[n])
                rest = np.delete(row1, n)
                mx = int(rest.max()) if len(rest) else -1
                r["prev"][d] = (dirty.index(n), _rel(x, mx), x - mx)
            r["jp_excl"], r["runner_up"] = None, None
            if 1 in r["prev"]:
                rest = row1.copy()
                rest[landed[k - 1]] = -1
                r["runner_up"] = np.nonzero(rest == rest.max())[0].tolist() if rest.max() >= 0 else []
                if rest.max() >= 0:
                    r["jp_excl"] = tiebreak_position(seq, int((rest == rest.max()).sum()))
            r["late"] = {}
            for d, rs in hist.pop(q, {}).items():
                if d > k or rs.max() < 0:
                    continue
                ts = np.nonzero(rs == rs.max())[0]
                late_nodes = landed[k - d:k]
                ranks = tuple(int(np.nonzero(ts == n)[0][0]) + 1 if n in ts else 0 for n in late_nodes)
                before = {x for x in landed[:k - d] if x >= 0}
                made = tuple(n >= 0 and n not in before for n in late_nodes)
                r["late"][d] = (len(ts), tiebreak_position(seq, len(ts)), ranks, made)
            out.append(r)
            landed.append(w)
            if w >= 0 and w not in dirty:
                dirty.append(w)
    return out


def check_claims(case: Case, recs=None) -> None:
    recs = recs if recs is not None else classify(case)
    for pod, field, value in case.claims:
        got = recs[pod]
        for f in field.split(".") if field != "*" else ():   # "*": the whole record
            got = got[int(f)] if f.isdigit() else got[f]
        if callable(value):
            assert value(got), (case.name, pod, field, got)
        else:
            assert got == value, (case.name, pod, field, got, value)


# ---- 1. re-landing chains ----
CHAIN_ANCHORS = (7, 130, 131, 399, 64, 200)


@functools.lru_cache(maxsize=None)
def chains(rs: tuple, batch: int = MAX_BATCH) -> Case:
    """Anchor i (15 points below anchor i - 1, far above the background) is strictly best for rs[i] consecutive pods,
    then its pod slots are used up: every decision of a chain made while the previous landing is pending leaves the
    winner out and is rolled back (rollback, the undo log undo[q % SP_LAG], the job rings of SP_JOBQ entries: chains
    of 2, 3, SP_LAG - 1, SP_LAG, SP_LAG + 1, SP_JOBQ + 1, 64 and 127 landings on one slot). The pod after a chain finds
    the landed row infeasible; six tail pods go to the background's ties."""
    n = 400
    nodes = CHAIN_ANCHORS[:len(rs)]
    c = flat(n, {a: CAP - 15_000 * i for i, a in enumerate(nodes)}, dict(zip(nodes, rs)))
    P = sum(rs) + 6
    d = Designer(c, [100] * P)
    claims, q = [], 0
    for i, (a, r) in enumerate(zip(nodes, rs)):
        for j in range(r):
            claims += [(q, "winner", a), (q, "T", 1)]
            if j and q % batch:
                claims += [(q, "prev.1", lambda v, i=i: v[1] == ">"), (q, "fresh", False)]
            q += 1
        if q % batch:
            claims += [(q, "prev.1", lambda v: v[1] == "<"), (q, "gone", lambda v, a=a: a in v)]
    claims += [(P - 1, "T", n - len(rs)), (P - 1, "M", 4)]
    return d.case(f"chains{rs}", batch, claims)


LATE_A, LATE_D = 77, (2, 3, 6, 11, 12)


@functools.lru_cache(maxsize=None)
def late_case() -> Case:
    """The winner that comes back d pods late, d = 2, 3, 6, 11, 12 (SP_LAG - 1 and SP_LAG): anchor A has room for the
    small pods' memory only. A small pod lands on A, the next d - 1 pods ask for 8 GiB, which A does not have (the
    memory Filter applies although only cpu is scored), and land on background nodes; then a small pod's strict winner
    is A again: a row that comes back as the strict winner, new and above every listed level. prev[d] is A's row, above
    everything else; prev[1 .. d-1] are the background rows, below. (It does not force a rollback of depth d: a
    re-scoring takes about as long as one or two decisions, so A's row is ready again at the closing pod)"""
    c = flat(400, {LATE_A: CAP})
    c.nodes["requested"][LATE_A, 1] = c.nodes["allocatable"][LATE_A, 1] - (len(LATE_D) + 1) * GiB - GiB // 2
    c.nodes["nonzero_requested"][LATE_A, 1] = c.nodes["requested"][LATE_A, 1]
    cpus, closing = [100], []
    for dd in LATE_D:
        cpus += [(STEP, 8 * GiB)] * (dd - 1) + [100]
        closing.append((len(cpus) - 1, dd))
    cpus += [(STEP, 8 * GiB)] * 8
    claims = [(0, "winner", LATE_A)]
    for q, dd in closing:
        claims += [(q, "winner", LATE_A), (q, "T", 1), (q, "fresh", False), (q, f"prev.{dd}", lambda v: v[:2] == (0, ">"))]
        claims += [(q, f"prev.{j}", lambda v: v[1] == "<" and v[0] > 0) for j in range(1, dd)]
        claims += [(q - j, "*", lambda r: r["winner"] != LATE_A and r["M"] == 4) for j in range(1, dd)]
    return Designer(c, cpus).case("late", MAX_BATCH, claims)


@functools.lru_cache(maxsize=None)
def alternating(pattern: str) -> Case:
    """Two anchors take 40 pods (a batch of 32 or more: the split pipeline) in the order ABAB.. (every row's landings on one Reserve wave's parity: waves 2 and 3
    take the even and the odd pods) or AABB.. (a re-landing waits for the other wave's Reserve of the same row: 'landed-
    again wait', done_ver / prev_pend)."""
    a, b, P = 21, 300, 40
    if pattern == "ABAB":   # 2000 per pod, B 1000 behind: the one landed on falls a point behind the other
        c, cpus = flat(400, {a: CAP, b: CAP - 1000}), [2000] * P
        order = [a, b] * (P // 2)
    else:                   # 100 then 3000, B 1500 behind: the small pod leaves its row ahead, the large one does not
        c, cpus = flat(400, {a: CAP, b: CAP - 1500}), [100, 3000] * (P // 2)
        order = ([a, a, b, b] * P)[:P]
    d = Designer(c, cpus)
    claims = []
    for q, nd in enumerate(order):
        claims += [(q, "winner", nd), (q, "T", 1)]
        if q >= 2:
            same = order[q - 1] == nd
            claims.append((q, "prev.1", lambda v, same=same: v[1] == (">" if same else "<")))
    return d.case(f"alternating-{pattern}", MAX_BATCH, claims)


# ---- 2. the >= of the verification ----
GE_GROUP, GE_X = (11, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 398), 200
GE_FILL = 21   # pods behind the designed ones: 40 in all, a batch the split pipeline takes (32 pods or more)


@functools.lru_cache(maxsize=None)
def ge_case() -> Case:
    """The verification's `mis |= sc >= dM` and the late-landing test of apply_late: twelve identical anchors (score
    98) and X one point above.
      pods 0-1   SMALL onto X: pod 1 finds pod 0's row one point above everything else
      pod 2      STEP onto X: X falls to the group's level for the SMALL pods, one below it for the STEP pods
      pods 3-8   STEP: every landing leaves its row exactly one point below M: the decision made without it stands
      pods 9-18  SMALL, 7 ties (the six untouched anchors and X): every landing leaves its row exactly at M; pods 11
                 and 15 have a tie-break position that moves when the previous row is left out (position 7 of 7),
                 pods 12 and 16 one that does not (3 of 7 and of 6)"""
    c = flat(400, {**{g: CAP - 1000 for g in GE_GROUP}, GE_X: CAP})
    d = Designer(c, [SMALL, SMALL] + [STEP] * 7 + [SMALL] * 10 + [STEP] * GE_FILL)
    claims = [(0, "winner", GE_X), (1, "winner", GE_X), (1, "prev.1", (0, ">", 1)), (2, "winner", GE_X)]
    d.place()
    d.place()
    d.place(want=node_rank(GE_X))   # (for the STEP pod X already ties with the group)
    for q in range(3, 9):
        d.place()
        claims += [(q, "T", 15 - q), (q, "prev.1", lambda v: v[1:] == ("<", -1))]
    for q in range(9, 19):
        if q in (11, 15):
            d.place(want=7)
            claims += [(q, "jp", 7), (q, "jp_excl", lambda v: v < 7)]
        elif q in (12, 16):
            d.place(want=3, also=lambda s: tiebreak_position(s, 6) == 3)
            claims += [(q, "jp", 3), (q, "jp_excl", 3)]
        else:
            d.place()
        claims += [(q, "T", 7), (q, "M", 98)]
        claims.append((q, "prev.1", lambda v, q=q: v[1:] == (("==", 0) if q > 9 else ("<", -1))))
    return d.case("ge", MAX_BATCH, claims)


# ---- 3. slot words ----
SLOT_G = 100
SLOT_RELAND = (62, 63, 64, 65, 99, 63, 0, 64, 1, 62, 65, 2, 99, 64, 63)


@functools.lru_cache(maxsize=None)
def slots_case() -> Case:
    """dn0/dn1, pend0/pend1, redo0/redo1 (slot s: bit s % 64 of word s / 64): 100 STEP pods land on 100 distinct
    anchors (each landing drops its row below the others), then SMALL pods re-land on the rows in slots 62, 63, 64,
    65, 99 ...: a SMALL landing leaves its row at M, so the next decision, made while slot 63 (then 64) is pending, is
    one the verification refuses; the landings on 62 then 65 put one rollback's restored rows on both sides of bit 64."""
    n = 400
    anchors = [4 * i + 1 for i in range(SLOT_G)]
    c = flat(n, {a: CAP for a in anchors})
    d = Designer(c, [STEP] * SLOT_G + [SMALL] * len(SLOT_RELAND))
    claims = []
    for q in range(SLOT_G):
        d.place()
        claims += [(q, "fresh", True), (q, "slot", q), (q, "nold", q), (q, "T", SLOT_G - q)]
    for i, s in enumerate(SLOT_RELAND):
        q = SLOT_G + i
        d.place(want=node_rank(d.nodes[s]))
        claims += [(q, "slot", s), (q, "fresh", False), (q, "T", SLOT_G), (q, "nnew", SLOT_G), (q, "listed", False)]
        if i:
            claims.append((q, "prev.1", (SLOT_RELAND[i - 1], "==", 0)))
    return d.case("slots", MAX_BATCH, claims)


# ---- 4. winner paths ----
PATH_PLAN = {1: 1, 2: 2, 3: "T", 4: "T-1", 57: 1, 58: "T", 59: 2, 60: "T-1", 61: 1, 62: "T", 63: "T-1"}
PATH_ENTRY = {5: 31, 6: 32, 7: 63, 8: 64}
PATH_SMALL_LAND, PATH_SMALL_SEE = (20, 40), (21, 41, 70)


@functools.lru_cache(maxsize=None)
def paths_case(G: int, P: int = MAX_BATCH, small: bool = True) -> Case:
    """decide_core's winner paths over a tie group of G identical anchors (the top level, listed from entry 0): every
    landing is on a clean anchor and drops its row below M for the STEP pods, so STEP pod k of the batch sees nold = k
    dirty rows listed at M and no longer there (the old-nodes path up to 61 of them, 58 on the prep wave; the general
    path beyond) and T = G - k ties. The tie-break positions are placed at the window's clips and at the list entries
    where the reads switch from the header lanes to list memory:
      pods 1, 2        positions 1 and 2: lo clips at 0
      pods 3, 4        positions T and T - 1: hi clips at len - 1
      pods 5-8         the winner at list entry 31, 32, 63, 64 (G >= 73)
      pods 57-63       positions 1, T, 2, T - 1, 1, T, T - 1 across nold 58 -> 59 and 61 -> 62
      pods 20, 40      SMALL: their rows stay at M for the SMALL pods 21, 41, 70, which see rows both old and new
                       (nnew > 0: the general path); small = False leaves them STEP pods: nnew is 0 for every pod,
                       so that only nold > 61 can send a decision down the general path"""
    anchors = list(range(60, 60 + G))
    c = flat(G + 126, {a: CAP for a in anchors})
    cpus = [STEP] * P
    for q in PATH_SMALL_LAND + PATH_SMALL_SEE:
        if q < P and small:
            cpus[q] = SMALL
    d = Designer(c, cpus)
    claims = []

    def clean_rank(t):
        return next(i + 1 for i, n in enumerate(t.tolist()) if n not in d.nodes)

    for q in range(P):
        T = len(d.ties())
        if q in PATH_PLAN and T > 2:
            jp = {"T": T, "T-1": T - 1}.get(PATH_PLAN[q], PATH_PLAN[q])
            d.place(want=jp)
            claims.append((q, "jp", jp))
        elif q in PATH_ENTRY and G > PATH_ENTRY[q] + 8:
            d.place(want=node_rank(anchors[PATH_ENTRY[q]]))
            claims.append((q, "e", PATH_ENTRY[q]))
        elif cpus[q] == SMALL:
            d.place(want=clean_rank)
        else:
            d.place()
        claims += [(q, "listed", True), (q, "fresh", True), (q, "nold", q)]
        if cpus[q] == STEP:
            claims += [(q, "nnew", 0), (q, "T", G - q)]
        elif q in PATH_SMALL_SEE:
            claims.append((q, "nnew", sum(1 for s in PATH_SMALL_LAND + PATH_SMALL_SEE if s < q)))
    return d.case(f"paths-{G}" + ("" if small else "-step"), MAX_BATCH, claims)


# ---- 5. split-selector exclusions ----
EXCL_G = 14


@functools.lru_cache(maxsize=None)
def excl_case() -> Case:
    """apply_late (SP_KW = 4): the prep wave decides pod q over a snapshot that lacks the last landing(s); wave 0
    excludes the landed ties and re-ranks inside the recorded window. Fourteen identical anchors; a STEP landing leaves
    the level (a tie of the snapshot that is none now), a SMALL one stays at M for SMALL pods on a slot the snapshot
    holds. With late[d] = (T_s, jp_s, ranks of the d late landings' nodes among the snapshot's ties, new slot?):
      pod 2   jp_s == rank: the recorded winner is the node pod 1 landed on; the winner moves to the next tie
      pod 3   rank < jp_s (the landing below the winner in node order); pod 4: rank > jp_s
      pod 5   jp_s == T_s > rank: T - ne < jp, recorded again
      pod 6   two late landings (pods 4 and 5), both below jp_s of the snapshot two pods earlier
      pod 9   SMALL, after the SMALL pods 7 (a fresh slot) and 8 (landing on that slot again): the late landing is on
              a slot inside the snapshot and stays a tie
      pod 11  jp_s == rank == T_s: the excluded winner was the last tie"""
    anchors = [20 + 25 * i for i in range(EXCL_G)]
    c = flat(400, {a: CAP for a in anchors})
    cpus = [STEP] * 40   # (13 designed pods; 40 make a batch the split pipeline takes)
    cpus[7] = cpus[8] = cpus[9] = SMALL
    d = Designer(c, cpus)
    tp = tiebreak_position
    d.place()                                                  # pod 0: 14 ties -> 13
    d.place(want=5)                                            # pod 1: rank 5 of 13 (pod 2's snapshot)
    d.place(also=lambda s: tp(s, 13) == 5)                     # pod 2: jp_s 5 == rank; lands on 5 of 12
    d.place(also=lambda s: tp(s, 12) == 8)                     # pod 3: snapshot 12 ties, pod 2 at rank 5 < jp_s 8
    d.place(also=lambda s: tp(s, 11) == 2)                     # pod 4: snapshot 11, pod 3 at rank 8 > jp_s 2
    d.place(also=lambda s: tp(s, 10) == 10 and tp(s, 9) == 3)  # pod 5: snapshot 10, pod 4 at rank 2, jp_s == T_s
    d.place(also=lambda s: tp(s, 10) == 6)                     # pod 6: two pods earlier 10 ties; pods 4, 5 at ranks 2, 4
    d.place()                                                  # pod 7 SMALL: a fresh slot
    d.place(want=node_rank(d.nodes[7]))                        # pod 8 SMALL: the same slot again
    d.place()                                                  # pod 9 SMALL
    last = int(d.ties(11)[-1])                                 # pod 11's snapshot: its last tie
    Ts = len(d.ties(11))
    d.place(want=node_rank(last))                              # pod 10 lands there
    d.place(also=lambda s: tp(s, Ts) == Ts)                    # pod 11: jp_s == rank == T_s
    claims = [
        (2, "late.1", (13, 5, (5, ), (True, ))), (2, "jp", 5),
        (3, "late.1", (12, 8, (5, ), (True, ))), (3, "jp", 8),
        (4, "late.1", (11, 2, (8, ), (True, ))), (4, "jp", 2),
        (5, "late.1", (10, 10, (2, ), (True, ))), (5, "jp", 3),
        (6, "late.2", (10, 6, (2, 4), (True, True))),
        (9, "late.1", lambda v: v[2][0] >= 1 and v[3] == (False, )), (9, "prev.1", lambda v: v[1] == "=="),
        (11, "late.1", (Ts, Ts, (Ts, ), (True, ))),
    ]
    return d.case("excl", MAX_BATCH, claims)


# ---- 6. feasibility ----
@functools.lru_cache(maxsize=None)
def fiterror_case() -> Case:
    """Three nodes with one pod slot each and 40 pods: from pod 3 on every listed node is a dirty row that turned
    infeasible, nothing is unlisted (next < 0): FitError from the lists alone (decide_core action 1), F = 0."""
    c = flat(3, {0: CAP, 1: CAP, 2: CAP}, {0: 1, 1: 1, 2: 1})
    d = Designer(c, [STEP] * 40)
    claims = [(q, "T", 3 - q) for q in range(3)]
    for q in range(3, 40):
        claims += [(q, "winner", -1), (q, "F", 0), (q, "nxt", -1), (q, "full_row", False),
                   (q, "gone", lambda v: len(v) == 3)]
    return d.case("fiterror", MAX_BATCH, claims)


@functools.lru_cache(maxsize=None)
def pending_only_case() -> Case:
    """Two nodes, one of them full: every pod lands on node 0, the only feasible row. Decided while that row is
    pending, a pod has no feasible node at all: a speculative FitError the verification must refuse (the pending row
    is feasible) and the rollback must undo."""
    c = flat(2, {0: CAP, 1: 0})
    d = Designer(c, [SMALL, STEP] * 20)
    claims = []
    for q in range(40):
        claims += [(q, "winner", 0), (q, "F", 1), (q, "T", 1)]
        if q:
            claims.append((q, "prev.1", lambda v: v[:2] == (0, ">")))
    return d.case("pending-only", MAX_BATCH, claims)


# ---- 7. full-row resolution over a crowded hash ----
HASH_N, HASH_C, HASH_A, HASH_Z = 16_640, 5, 104, 12


def sp_hash(node: int) -> int:
    """the node -> slot hash's first probe (rebuild_hash / sp_hash_find)"""
    return ((node * 2654435761) & 0xFFFFFFFF) & (SP_HASH - 1)


@functools.lru_cache(maxsize=None)
def hash_case(A: int = HASH_A, Z: int = HASH_Z, P: int = MAX_BATCH) -> Case:
    """16,640 nodes: A one-pod anchors and Z (Z pods, 50 points lower), all at ids = 5 (mod 128): every dirty slot hashes
    to the same first probe (asserted from the hash expression), so the linear probing runs the table's length. The
    background's one level holds more than 16,500 nodes, more than LCAP: it is never listed. Pods 0 .. A-1 take the
    anchors and the next Z pods land on Z; the last P - A - Z pods find every listed node dirty and infeasible with an
    unlisted level below: full-row resolutions over a hash of A + 1 and more slots.
    The split pipeline (104 anchors, a batch of 128) resolves a pod from its whole row only over the exact state: the
    prep wave records such a pod again once everything before it has settled. The single selector (16 anchors, a batch
    of 31) resolves speculatively: each pod decided while Z's row is pending finds nothing listed and takes a
    background node from the whole row, which the verification refuses; the rollback leaves hash_ok = false and the next
    resolution rebuilds the hash."""
    ids = [HASH_C + SP_HASH * i for i in range(A + 1)]
    assert len({sp_hash(n) for n in ids}) == 1 and ids[-1] < HASH_N
    anchors, z = ids[:A], ids[A]
    c = flat(HASH_N, {**{a: CAP for a in anchors}, z: CAP // 2}, {**{a: 1 for a in anchors}, z: Z})
    d = Designer(c, [STEP] * P)
    claims = []
    for q in range(A):
        claims += [(q, "T", A - q), (q, "full_row", False)]
    first = A + Z
    for q in range(A, first):
        claims += [(q, "winner", z), (q, "full_row", False)]
        if q > A:   # decided while Z is pending, nothing listed is left
            claims += [(q, "prev.1", lambda v: v[1] == ">"), (q, "runner_up", lambda v: len(v) == HASH_N - A - 1)]
    for q in range(first, P):
        claims += [(q, "full_row", True), (q, "nd", A + 1 + q - first), (q, "Mclean", 4),
                   (q, "T", HASH_N - A - 1 - (q - first)), (q, "listed", False)]
    return d.case(f"hash-{P}", P, claims, slowpath=P - first)


# ---- 8. undo of Reserve state, host cuts (NodeNUMAResource clusters) ----
NUMA_N, NUMA_X, NUMA_Y = 8, 2, 5
UID_NUMA = 0xCE000000
NUMA_FILL = 32   # small pods behind the designed ones: every batch has 32 pods or more (the split pipeline)


def _zone_full(z):
    return nu.Alloc(nu.cpus_of_zone(z), ((z, nu.CPN * 1000, nu.SEQ_MEM[z]),))


def _numa_nodes(special: dict) -> tuple:
    """eight Restricted-policy nodes of numa_edges_util's topology; those not in `special` have 2 CPUs left (no pod of
    more fits, and every small pod scores far lower there)"""
    zones = tuple((nu.CPN * 1000, nu.SEQ_MEM[z]) for z in range(4))
    rest = (nu.Alloc(nu.cpus_of_zone(0, cores=range(3)), ((0, 6000, 20 * GiB),)), _zone_full(1), _zone_full(2), _zone_full(3))
    return tuple(special[i] if i in special else nu.Node(f"n{i}", "Restricted", zones, rest) for i in range(NUMA_N))


def _cs(cpus, k):
    return nu.Pod(cpus * 1000, GiB + k, abi.GS_QOS_LSR, nu.FULL, True, note="cpuset")


def _ls(cpus):
    return nu.Pod(cpus * 1000, GiB)


@functools.lru_cache(maxsize=None)
def undo_case(kind: str) -> Case:
    """UndoRec.row / UndoRec.cs: a pod with a Reserve record is decided while the previous landing on X, its true
    winner, is pending; the decision made without X lands it on Y, a NUMA-policy node, where the Reserve wave takes a
    cpuset ("cpuset": an LSR FullPCPUs pod) or splits the request over two zones ("split": 9 CPUs and 33 GiB, more than a
    zone holds), and the rollback restores Y's row and cpu state from the undo log. Later pods really land on Y, a
    cpuset pod among them, and must find it pristine: their allocations are compared byte for byte.
      cpuset  pods 1 and 3 (cpuset pods): winner X = pod 0's / pod 2's node, the only other feasible node is Y;
              pod 4 lands on Y, pod 5 (a cpuset pod) lands there again
      split   pod 1 (the split pod): winner X, runner-up Y alone; pod 2 lands on Y, pod 3 (a cpuset pod) again; pod 4
              (a split pod again) fits Y only, the row pod 3's landing left pending: a speculative FitError"""
    zones = tuple((nu.CPN * 1000, nu.SEQ_MEM[z]) for z in range(4))
    X, Y = NUMA_X, NUMA_Y
    if kind == "cpuset":
        nodes = _numa_nodes({X: nu.Node("X", "Restricted", zones, ()), Y: nu.Node("Y", "Restricted", zones, (_zone_full(3), ))})
        pods = [_ls(1), _cs(4, 1), _ls(7), _cs(2, 2), _ls(7), _cs(2, 3), _ls(1), _cs(2, 4), _ls(1), _cs(4, 5), _ls(1), _cs(2, 6)]
        claims = [(0, "winner", X), (2, "winner", X), (4, "winner", Y), (4, "fresh", True), (5, "winner", Y), (5, "prev.1", lambda v: v[1] == ">")]
        for q in (1, 3):
            claims += [(q, "winner", X), (q, "prev.1", lambda v: v[1] == ">"), (q, "runner_up", [Y])]
    else:
        two = (_zone_full(2), _zone_full(3))
        nodes = _numa_nodes({X: nu.Node("X", "Restricted", zones, two),
                             Y: nu.Node("Y", "Restricted", zones, two + (nu.Alloc((), ((0, 3000, GiB), )), ))})
        pods = [_ls(1), nu.Pod(9000, 33 * GiB), _ls(1), _cs(2, 1), nu.Pod(9000, 33 * GiB + 1), _ls(1), _cs(2, 2), _ls(1)]
        claims = [(0, "winner", X), (1, "winner", X), (1, "prev.1", lambda v: v[1] == ">"), (1, "runner_up", [Y]),
                  (2, "winner", Y), (2, "fresh", True), (3, "winner", Y), (3, "prev.1", lambda v: v[1] == ">"),
                  (4, "winner", Y), (4, "F", 1), (4, "runner_up", [])]
    pods += [_ls(1)] * NUMA_FILL
    d = Designer(nodes, nu.pod_records(pods, UID_NUMA), numa=True)
    d.place(want=node_rank(X))
    case = d.case(f"undo-{kind}", MAX_BATCH, claims)
    record = case.want["flags"] & (abi.GS_PLACED_CPUSET | abi.GS_PLACED_NUMA)
    assert (record[case.want["node"] >= 0] != 0).all() and (case.want["flags"] & abi.GS_PLACED_CPUSET != 0).sum() >= 2
    return case


@functools.lru_cache(maxsize=None)
def rising_case() -> Case:
    """Totals that rise with a landing: NodeNUMAResource alone (weights 0, 0, 1) with scoringStrategy and
    numaScoringStrategy MostAllocated on eight empty identical policy nodes. The node the first pod lands on scores
    higher for every later pod, above every listed level (all nodes are listed at their common batch-start score):
    decide_core's general path with len == 0 (level M is not listed, nnew = 1, nold = 0), a chain of landings on one
    slot whose row is strictly best and moves up (15, 31, 46, 62). The fourth pod fills the zone, which then scores as
    an empty one: pods 4, 8, ... see all eight nodes tied again, the landed rows among them both old and new."""
    zones = tuple((nu.CPN * 1000, nu.SEQ_MEM[z]) for z in range(4))
    nodes = tuple(nu.Node(f"n{i}", "Restricted", zones, ()) for i in range(NUMA_N))
    most = {"type": "MostAllocated", "resources": {"cpu": 1, "memory": 1}}
    cfg_kw = dict(weights=(0, 0, 1), numa=config.numa_args(scoringStrategy=most, numaScoringStrategy={"type": "MostAllocated"}))
    d = Designer(nodes, nu.pod_records([nu.Pod(2000, 2 * GiB)] * 40, UID_NUMA + 0x2000), numa=True, cfg_kw=cfg_kw)
    d.place(want=3)
    d.rest()
    claims = []
    for q in range(40):   # four pods fill a zone: three climbs, then the full zone scores as an empty one again
        if q % 4 == 0:
            claims.append((q, "T", NUMA_N))
            if q:         # the landed rows are back at their batch-start score: both old and new
                claims += [(q, "nnew", lambda v: v >= 1), (q, "*", lambda r: r["nold"] == r["nnew"] == r["nd"])]
        else:
            claims += [(q, "winner", d.nodes[q - 1]), (q, "T", 1), (q, "nnew", 1), (q, "nold", 0), (q, "listed", False),
                       (q, "prev.1", lambda v: v[1] == ">"), (q, "*", lambda r: r["M"] > r["Mclean"])]
    return d.case("rising", MAX_BATCH, claims)


RISE_TOP = (3, 5)


@functools.lru_cache(maxsize=None)
def rising_listed_case() -> Case:
    """Rows rising into a listed clean level (decide_core's general path with len > 0 and nnew > 0: `newer`, `ltn`, the
    window's ends), under rising_case's MostAllocated profile. Eight single-zone nodes of 8 CPUs; nodes 3 and 5 hold
    5 CPUs and 5 GiB already: the top level, listed first for every pod. A pod of 5 CPUs fits only an empty node and
    lifts it to exactly that level; the next pod (3 CPUs: it fills the node it lands on) finds the risen row tied with
    the listed clean ones:
      pods 0, 1   node 1 rises (an id below the listed 3 and 5); pod 1 lands on it: the winner is the new row
      pods 2, 3   node 4 rises (between); pod 3 lands on 3, a listed clean node, and fills it: an old row from here on
      pods 4, 5   node 6 rises (above) beside the risen row 4: two new rows, between and above; pod 5 lands on 6
      pods 6, 7   node 0 rises beside the risen row 4: two new rows, below and between; pod 7 lands on 5
    32 pods of 0.1 CPU follow, so that the batch is one the split pipeline takes."""
    z1 = ((nu.CPN * 1000, nu.SEQ_MEM[0]), )
    pre = nu.Alloc((), ((0, 5000, 5 * GiB), ))
    nodes = tuple(nu.Node(f"n{i}", "Restricted", z1, (pre, ) if i in RISE_TOP else ()) for i in range(NUMA_N))
    most = {"type": "MostAllocated", "resources": {"cpu": 1, "memory": 1}}
    cfg_kw = dict(weights=(0, 0, 1), numa=config.numa_args(scoringStrategy=most, numaScoringStrategy={"type": "MostAllocated"}))
    big, fill = nu.Pod(5000, 5 * GiB), nu.Pod(3000, 3 * GiB)
    d = Designer(nodes, nu.pod_records([big, fill] * 4 + [nu.Pod(100, 64 << 20)] * NUMA_FILL, UID_NUMA + 0x3000), numa=True, cfg_kw=cfg_kw)
    plan = ((1, 1), (4, 3), (6, 6), (0, 5))   # (the node that rises, the node the next pod lands on)
    for up, land in plan:
        d.place(want=node_rank(up))
        d.place(want=node_rank(land))
    claims = [(1, "new_nodes", [1]), (1, "clean_ties", [3, 5]), (3, "new_nodes", [4]), (3, "clean_ties", [3, 5]),
              (5, "new_nodes", [4, 6]), (5, "clean_ties", [5]), (7, "new_nodes", [0, 4]), (7, "clean_ties", [5])]
    for q in (1, 3, 5, 7):
        claims += [(q, "listed", True), (q, "nold", int(q >= 5)), (q, "*", lambda r: r["M"] == r["Mclean"] and r["T"] == r["nnew"] + len(r["clean_ties"]))]
    return d.case("rising-listed", MAX_BATCH, claims)


WIDE_1, WIDE_2 = 4, 6


@functools.lru_cache(maxsize=None)
def hostcut_case() -> Case:
    """`if (s_cut_at >= v) s_cut_at = -1` in the rollback: pods 2, 4 and 5 are cpuset pods of 30 CPUs, which only the two
    160-core nodes hold; that topology is outside the device cpuset scope, so the host selects their cpusets and the
    batch ends after each of them (three cuts: none of them is its batch's last pod).
      pod 2   after a mis-speculated pod: pod 1 is decided while pod 0's row, its winner, is pending
      pod 4   the mis-speculated pod itself: pod 3 lands on the wide node that pod 4 also wins, the other wide node is
              the runner-up; the decision made without the pending row asks for a cut that the rollback takes back
      pod 5   before one: the first pod of its batch, pods 6 and 7 land on X one after the other behind it"""
    zones = tuple((nu.CPN * 1000, nu.SEQ_MEM[z]) for z in range(4))
    wzones = tuple((40_000, 64 * GiB + z) for z in range(4))

    def wfull(z, n=40):
        return nu.Alloc(tuple(range(40 * z, 40 * z + n)), ((z, n * 1000, 60 * GiB), ))

    X, W1, W2 = NUMA_X, WIDE_1, WIDE_2
    nodes = _numa_nodes({X: nu.Node("X", "Restricted", zones, ()),
                         W1: nu.Node("W1", "Restricted", wzones, (wfull(3), wfull(2, 30)), family="wide"),
                         W2: nu.Node("W2", "Restricted", wzones, (wfull(3), wfull(2)), family="wide")})
    half = nu.Pod(500, GiB)
    pods = [half, half, _cs(30, 1), _ls(9), _cs(30, 2), _cs(30, 3), half, half, _ls(1), _cs(2, 4), _ls(1)]
    claims = [(0, "winner", X), (1, "winner", X), (1, "prev.1", lambda v: v[1] == ">"), (2, "winner", W1),
              (3, "winner", W2), (4, "winner", W2), (4, "prev.1", lambda v: v[1] == ">"), (4, "runner_up", [W1]),
              (5, "winner", W1), (5, "nd", 0), (6, "winner", X), (7, "winner", X), (7, "prev.1", lambda v: v[1] == ">")]
    pods += [nu.Pod(500, GiB)] * NUMA_FILL
    d = Designer(nodes, nu.pod_records(pods, UID_NUMA + 0x1000), numa=True)
    case = d.case("hostcut", MAX_BATCH, claims, host_pods=(2, 4, 5))
    assert all(case.want["flags"][q] & abi.GS_PLACED_CPUSET and nodes[case.want["node"][q]].family == "wide" for q in (2, 4, 5))
    assert predicted_cuts(case) == 3
    return case


def all_cases() -> list:
    """every case, by name (built on first use)"""
    return [("chains-short", lambda: chains((2, 3, 11, 12, 13, 25))), ("chains-long", lambda: chains((64, 127))),
            ("chains-low-shard", lambda: chains((5, 9))),   # anchors 7 and 130: both in the first half of the nodes
            ("alternating-ABAB", lambda: alternating("ABAB")), ("alternating-AABB", lambda: alternating("AABB")),
            ("ge", ge_case), ("slots", slots_case), ("paths-130", lambda: paths_case(130)),
            ("paths-130-step", lambda: paths_case(130, small=False)), ("paths-300", lambda: paths_case(300)), ("paths-2048", lambda: paths_case(2048, 72)), ("excl", excl_case),
            ("fiterror", fiterror_case), ("pending-only", pending_only_case), ("hash", hash_case), ("hash-31", lambda: hash_case(16, 8, 31)),
            ("undo-cpuset", lambda: undo_case("cpuset")), ("undo-split", lambda: undo_case("split")),
            ("hostcut", hostcut_case), ("rising", rising_case), ("rising-listed", rising_listed_case),
            ("late", late_case)]


