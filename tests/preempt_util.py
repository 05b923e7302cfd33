"""ElasticQuota's PostFilter dry run: the truth, restated in Python over the CPU oracle's Filter.

Steps 1-4 of the dry run (elasticquota/preempt.go:61-215, plugin.go:257-321 and [upstream] preemption.Evaluator's
DryRunPreemption / pickOneNodeForPreemption) are restated here; every Filter verdict is the oracle's (or_evaluate
through fit_diag_util.codes_of). One Oracle is kept in the engine's state: it holds the assign cache and the NUMA
allocations, which or_nodes_upsert leaves alone (it replaces only the gs_node). For reprieve step s every potential
node's gs_node is upserted with that node's own current requested / pod_count and the preemptor is evaluated once: the
nodes are independent, so one evaluation serves all of them. The rows are restored afterwards."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from koordinator_amd import abi, synth
from oracle import oracle as orc
from tests import fit_diag_util as fd

NOT_POTENTIAL, CANDIDATE, NO_VICTIMS, UNFIT, FITS, ERROR = range(6)
PRIO = 1000          # the preemptors' priority; residents lie in a band around it
QUOTA = 1            # the preemptors' quota id
FIT_BITS = (abi.GS_FAIL_FIT_PODS, abi.GS_FAIL_FIT_CPU, abi.GS_FAIL_FIT_MEMORY, abi.GS_FAIL_FIT_EPHEMERAL,
            abi.GS_FAIL_FIT_SCALAR)


# ---- the pick (pickOneNodeForPreemption with no PDB violations), criterion by criterion ----
def pick(cands) -> tuple[int, int]:
    """cands: [(node, first_priority, sum_priorities, num_victims, earliest_start_ns)] -> (index of the pick, the
    criterion 2..6 that decided it; 0 for a single candidate); (-1, 0) for none."""
    if not cands:
        return -1, 0
    alive = list(range(len(cands)))
    if len(alive) == 1:
        return alive[0], 0
    steps = [(2, lambda c: c[1], min), (3, lambda c: c[2], min), (4, lambda c: c[3], min), (5, lambda c: c[4], max),
             (6, lambda c: c[0], min)]
    for crit, key, best in steps:
        b = best(key(cands[i]) for i in alive)
        alive = [i for i in alive if key(cands[i]) == b]
        if len(alive) == 1:
            return alive[0], crit
    return alive[0], 6


def key_of(node: int, victims) -> tuple:
    """The pick key of a candidate: victims in victim order (the first has the highest priority).
    GetEarliestPodStartTime: the earliest start among the victims of the highest priority."""
    top = max(int(v["priority"]) for v in victims)
    assert top == int(victims[0]["priority"])
    return (node, top, sum(int(v["priority"]) + (1 << 31) for v in victims), len(victims),
            min(int(v["start_time_ns"]) for v in victims if int(v["priority"]) == top))


def candidate_array(cands) -> np.ndarray:
    a = np.zeros(len(cands), abi.PREEMPT_CANDIDATE_DTYPE)
    for i, (node, first, total, n, earliest) in enumerate(cands):
        a[i] = (node, first, total, n, 0, earliest)
    return a


# ---- residents ----
def order_key(r):
    """MoreImportantPod: higher priority first, then the earlier start; the remaining tie by ascending uid."""
    return (-int(r["priority"]), int(r["start_time_ns"]), int(r["uid"]))


def make_residents(c: synth.Cluster, counts, seed: int, quota_pct: int = 55):
    """Seeded residents on a cluster: node i gets counts[i] pods (RESIDENT_POD_DTYPE) whose requests sum per slot to at
    most 0.9 x the node's requested; priorities in PRIO-6 .. PRIO+3; 4 quota ids (quota_pct % in QUOTA); ~10%
    non-preemptible, ~10% not tracked by their quota, ~2% terminating; start times distinct per node.
    -> (node_idx[M], pods[M])."""
    s = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    assert (counts <= c.nodes["pod_count"]).all(), "k <= pod_count"
    M = int(counts.sum())
    node_idx = np.repeat(np.arange(c.num_nodes, dtype=np.uint32), counts)
    pods = np.zeros(M, abi.RESIDENT_POD_DTYPE)
    pods["uid"] = (np.arange(M, dtype=np.uint64) + 1) * 7919 + seed * 1_000_003
    w = s.randint(1, 9, M).astype(np.float64)
    wsum = np.bincount(node_idx, w, c.num_nodes)[node_idx]
    for slot, step in ((0, 100), (1, 1 << 20), (2, 1 << 20)):
        tot = c.nodes["requested"][node_idx, slot].astype(np.float64) * 0.9
        pods["requests"][:, slot] = (tot * w / wsum).astype(np.int64) // step * step
    pods["quota_request"][:, 0] = pods["requests"][:, 0]
    pods["quota_request"][:, 1] = pods["requests"][:, 1]
    pods["quota_request_mask"] = 3
    pods["priority"] = PRIO + s.randint(-6, 4, M)
    q = s.randint(0, 100, M)
    pods["quota"] = np.where(q < quota_pct, QUOTA, np.where(q < quota_pct + 15, 0, np.where(q < quota_pct + 30, 2, 3)))
    f = s.randint(0, 100, M)
    g = s.randint(0, 100, M)
    pods["flags"] = (np.where(f < 10, abi.GS_RESIDENT_NON_PREEMPTIBLE, 0) |
                     np.where(g < 90, abi.GS_RESIDENT_QUOTA_TRACKED, 0) |
                     np.where(s.randint(0, 100, M) < 2, abi.GS_RESIDENT_TERMINATING, 0)).astype(np.uint32)
    base = c.now_ns - 3600 * 10**9
    rank = np.concatenate([s.permutation(int(k)) for k in counts]) if M else np.zeros(0, np.int64)
    pods["start_time_ns"] = base + rank * 10**9
    return node_idx, pods


class Table:
    """The resident-pod table on the truth's side: per node the pods in MoreImportantPod order."""

    def __init__(self, n: int):
        self.nodes: list[list] = [[] for _ in range(n)]

    def add(self, node_idx, pods):
        for i, p in zip(np.asarray(node_idx).tolist(), pods):
            assert all(int(r["uid"]) != int(p["uid"]) for r in self.nodes[i])
            self.nodes[i].append(p.copy())
            self.nodes[i].sort(key=order_key)

    def remove(self, node_idx, uids):
        for i, u in zip(np.asarray(node_idx).tolist(), np.asarray(uids).tolist()):
            self.nodes[i] = [r for r in self.nodes[i] if int(r["uid"]) != u]


def make_preemptor(pod, row: int, used, limit, quota: int = QUOTA, priority: int = PRIO, flags: int = 0,
                   nominated: int = -1, limit_mask: int = 3):
    """A PREEMPTOR_DTYPE record: quota request = the pod's cpu / memory requests (dims 0, 1)."""
    p = np.zeros(1, abi.PREEMPTOR_DTYPE)[0]
    p["pod"] = pod
    p["priority"], p["quota"] = priority, quota
    p["quota_request"][:2] = pod["requests"][:2]
    p["quota_request_mask"] = 3
    p["limit_mask"] = limit_mask
    p["used"][:2] = used
    p["used_limit"][:2] = limit
    p["flags"], p["nominated_node"], p["row"] = flags, nominated, row
    return p


@functools.lru_cache(maxsize=None)
def fw_code(word: int) -> int:
    return abi.status_framework_code(word)


# ---- the dry run ----
@dataclasses.dataclass
class Answer:
    status: int                      # gs_preempt_status
    node: int
    victims: list                    # uids, in victim order
    num_potential: int
    num_candidates: int
    num_errors: int
    node_status: np.ndarray          # uint8[N]
    victim_bits: np.ndarray          # uint64[N][2]
    cands: list                      # the candidates' pick keys, ascending node
    decided_at: int                  # the criterion that decided the pick
    non_prefix: int                  # candidates with a victim more important than a reprieved potential victim
    quota_victims_on_fitting: int    # victims on nodes the pod fits with nobody evicted
    amp_flips: int = 0               # nodes whose Filter fails at some step on the amplified-CPU check alone
    only_bits: int = 0               # the Fit bits that were the only failing bit of some reprieve step's Filter code


def exceeds(pre, used) -> bool:
    if int(pre["quota"]) < 0:
        return False
    m = int(pre["quota_request_mask"]) & int(pre["limit_mask"])
    return any((m >> d & 1) and used[d] + int(pre["quota_request"][d]) > int(pre["used_limit"][d])
               for d in range(abi.GS_QUOTA_DIMS))


def move_used(r, sign: int, used, skip: bool) -> None:
    """The plugin's AddPod (+1) / RemovePod (-1) on `used`: the request of a tracked resident over its own keys
    (quota_request_mask; a value outside the mask is no key of the request and moves nothing), floored at zero per
    dimension when it leaves."""
    if skip or not int(r["flags"]) & abi.GS_RESIDENT_QUOTA_TRACKED:
        return
    for d in range(abi.GS_QUOTA_DIMS):
        if not int(r["quota_request_mask"]) >> d & 1:
            continue
        q = int(r["quota_request"][d])
        used[d] = max(0, used[d] - q) if sign < 0 else used[d] + q


def dry_run(o: orc.Oracle, nodes: np.ndarray, table: Table, pre, rows=None) -> Answer:
    """One preemptor on the oracle's state; nodes: the oracle's current gs_node rows (left unchanged)."""
    N = len(nodes)
    zero = Answer(abi.GS_PREEMPT_NOT_ELIGIBLE, -1, [], 0, 0, 0, np.zeros(N, np.uint8), np.zeros((N, 2), np.uint64), [], 0,
                  0, 0)
    prio, quota, row = int(pre["priority"]), int(pre["quota"]), int(pre["row"])
    skip = quota < 0
    # 1. PodEligibleToPreemptOthers
    if int(pre["flags"]) & abi.GS_PREEMPT_NEVER:
        return zero
    nom = int(pre["nominated_node"])
    if nom >= 0 and not (row >= 0 and fw_code(int(rows[row][nom])) == 2):
        if any(int(r["flags"]) & abi.GS_RESIDENT_TERMINATING and int(r["quota"]) == quota and int(r["priority"]) < prio
               for r in table.nodes[nom]):
            return zero
    # 2. the potential nodes
    if row < 0:
        potential = list(range(N))
    else:
        potential = [i for i in range(N) if fw_code(int(rows[row][i])) != 2]
    status = np.zeros(N, np.uint8)
    bits = np.zeros((N, 2), np.uint64)
    pod = np.array([pre["pod"]], abi.POD_DTYPE)
    fits_now = fd.codes_of(o, pod)[0] == 0
    work = nodes.copy()

    def evaluate(changed):
        if changed:
            idx = np.array(changed, np.uint32)
            o.upsert_nodes(work[idx], idx)
        return fd.codes_of(o, pod)[0]

    def move(i, r, sign, used):
        """NodeInfo.AddPodInfo (+1) / RemovePod (-1) of resident r on node i, and the plugin's AddPod / RemovePod"""
        work["requested"][i] += sign * r["requests"]
        work["pod_count"][i] += sign
        move_used(r, sign, used, skip)

    # 3a. the potential victims leave
    state = {}
    for i in potential:
        res = table.nodes[i]
        pv = [j for j, r in enumerate(res) if not int(r["flags"]) & abi.GS_RESIDENT_NON_PREEMPTIBLE and
              int(r["priority"]) < prio and int(r["quota"]) == quota]
        if not pv:
            status[i] = NO_VICTIMS
            continue
        used = [int(x) for x in pre["used"]]
        for j in pv:
            move(i, res[j], -1, used)
        state[i] = dict(pv=pv, used=used, victims=[], err=False)
    # 3b. the Filter with all of them gone
    codes = evaluate(list(state))
    for i in list(state):
        if codes[i]:
            status[i] = UNFIT
            del state[i]
    # 3d. reprieve, one potential victim per node and step
    amp_nodes = set()
    only_bits = 0
    step = 0
    while True:
        cur = [i for i, s in state.items() if not s["err"] and step < len(s["pv"])]
        if not cur:
            break
        for i in cur:
            s = state[i]
            move(i, table.nodes[i][s["pv"][step]], +1, s["used"])
        codes = evaluate(cur)   # (a node removed from below is upserted again by its next step)
        for i in cur:
            s = state[i]
            j = s["pv"][step]
            r = table.nodes[i][j]
            removed = False
            if codes[i]:
                if (int(codes[i]) & abi.GS_FAIL_NUMA_MASK) >> abi.GS_FAIL_NUMA_SHIFT == abi.GS_NUMA_INSUFFICIENT_AMP_CPU \
                        and not int(codes[i]) & 0x3F:
                    amp_nodes.add(i)
                if int(codes[i]) in FIT_BITS:
                    only_bits |= int(codes[i])
                move(i, r, -1, s["used"])
                removed = True
                s["victims"].append(j)
            if exceeds(pre, s["used"]):
                if removed:
                    s["err"] = True          # the second nodeInfo.RemovePod fails
                    continue
                move(i, r, -1, s["used"])
                s["victims"].append(j)
        step += 1
    # restore the oracle's rows
    o.upsert_nodes(nodes)
    # 3e. the candidates
    cands, non_prefix, qv = [], 0, 0
    nerr = 0
    for i, s in sorted(state.items()):
        if s["err"]:
            status[i] = ERROR
            nerr += 1
            continue
        if not s["victims"]:
            status[i] = FITS
            continue
        status[i] = CANDIDATE
        for j in s["victims"]:
            bits[i][j >> 6] |= np.uint64(1) << np.uint64(j & 63)
        v = [table.nodes[i][j] for j in s["victims"]]
        cands.append(key_of(i, v))
        vs = set(s["victims"])
        if any(j not in vs and j > s["victims"][0] for j in s["pv"]):
            non_prefix += 1
        if fits_now[i]:
            qv += len(v)
    k, crit = pick(cands)
    ans = Answer(abi.GS_PREEMPT_NO_CANDIDATES, -1, [], len(potential), len(cands), nerr, status, bits, cands, crit,
                 non_prefix, qv, len(amp_nodes), only_bits)
    if not potential:
        ans.status = abi.GS_PREEMPT_NO_POTENTIAL_NODES
    elif k >= 0:
        ans.status = abi.GS_PREEMPT_NOMINATED
        ans.node = cands[k][0]
        ans.victims = [int(table.nodes[ans.node][j]["uid"]) for j in state[ans.node]["victims"]]
    elif nerr:
        ans.status = abi.GS_PREEMPT_ERROR
    return ans


# ---- the oracle in the engine's end state ----
def end_state(c: synth.Cluster, numa: bool, npods: int | None = None):
    """(oracle, gs_node rows, placements) after the first npods pods of c were scheduled: the rows are the loaded rows
    plus the placements' AddPod deltas; upserting them leaves every Filter code unchanged (asserted on a pod sample)."""
    o = orc.Oracle(fd.make_cfg(c, numa))
    synth.load_into(o, c)
    pods = c.pods if npods is None else c.pods[:npods]
    got = o.schedule(pods, np.arange(len(pods), dtype=np.uint64)) if len(pods) else np.zeros(0, abi.PLACEMENT_DTYPE)
    nodes = c.nodes.copy()
    for p, g in zip(pods, got):
        n = int(g["node"])
        if n >= 0:
            nodes["requested"][n] += p["requests"]
            nodes["nonzero_requested"][n] += p["nonzero_requests"]
            nodes["pod_count"][n] += 1
    sample = c.pods[:: max(1, len(c.pods) // 8)][:8]
    before = fd.codes_of(o, sample)
    o.upsert_nodes(nodes)
    assert np.array_equal(before, fd.codes_of(o, sample)), "the reconstructed rows change a Filter code"
    return o, nodes, got


def quota_used(pods, quota: int = QUOTA):
    """The quota's used: the tracked residents' quota requests (dims 0, 1)."""
    m = (pods["quota"] == quota) & ((pods["flags"] & abi.GS_RESIDENT_QUOTA_TRACKED) != 0)
    return pods["quota_request"][m][:, :2].sum(axis=0)


def check(res, status, bits, k: int, ans: Answer, table: Table):
    """Preemptor k of one gs_preempt_dry_run call against the truth: node_status, victim_bits, the result struct, and
    gs_preempt_pick_node over the detail arrays."""
    bad = np.nonzero(status[k] != ans.node_status)[0]
    assert bad.size == 0, (f"preemptor {k}: {bad.size} node statuses differ, first at node {bad[0]}: "
                           f"gpu {status[k][bad[0]]} truth {ans.node_status[bad[0]]}")
    bad = np.nonzero((bits[k] != ans.victim_bits).any(axis=1))[0]
    assert bad.size == 0, (f"preemptor {k}: victim bits differ at node {bad[0]}: gpu {bits[k][bad[0]]} "
                           f"truth {ans.victim_bits[bad[0]]}")
    r = res[k]
    assert (int(r["status"]), int(r["node"])) == (ans.status, ans.node), (k, r["status"], r["node"], ans.status, ans.node)
    assert int(r["num_victims"]) == len(ans.victims) and r["victims"][:len(ans.victims)].tolist() == ans.victims, k
    assert (r["victims"][len(ans.victims):] == 0).all()
    assert (int(r["num_potential"]), int(r["num_candidates"]), int(r["num_errors"])) == \
        (ans.num_potential, ans.num_candidates, ans.num_errors), k
    # the device reduction agrees with the host pick over the detail arrays
    cands = []
    for i in np.nonzero(status[k] == CANDIDATE)[0].tolist():
        cands.append(key_of(i, [table.nodes[i][j] for j in range(len(table.nodes[i]))
                                if int(bits[k][i][j >> 6]) >> (j & 63) & 1]))
    j = abi.preempt_pick_node(candidate_array(cands)) if cands else -1
    assert (cands[j][0] if j >= 0 else -1) == int(r["node"]), k


# ---- the cases the GPU tests run (tests/test_preempt.py asserts their input conditions on the truth alone) ----
@dataclasses.dataclass
class Case:
    c: synth.Cluster
    numa: bool
    npods: int | None            # pods scheduled first (None: all of c.pods)
    node_idx: np.ndarray         # the residents
    residents: np.ndarray
    rows: np.ndarray | None      # status rows [R][N]
    preemptors: np.ndarray       # PREEMPTOR_DTYPE
    pod_of: list | None = None   # row cases: the index in c.pods of each preemptor's pod
    _answers: dict = dataclasses.field(default_factory=dict)
    _state: tuple | None = None

    def table(self) -> Table:
        t = Table(self.c.num_nodes)
        t.add(self.node_idx, self.residents)
        return t

    def answers(self, ks) -> list[Answer]:
        """The truth of preemptors ks, each computed once."""
        if self._state is None:
            o, nodes, _ = end_state(self.c, self.numa, self.npods)
            self._state = (o, nodes, self.table())
        o, nodes, table = self._state
        for k in ks:
            if k not in self._answers:
                self._answers[k] = dry_run(o, nodes, table, self.preemptors[k], self.rows)
        return [self._answers[k] for k in ks]


def resident_counts(c: synth.Cluster, choices, seed: int) -> np.ndarray:
    s = np.random.RandomState(seed)
    return np.minimum(np.array(choices)[s.randint(0, len(choices), c.num_nodes)], c.nodes["pod_count"])


@functools.lru_cache(maxsize=None)
def row_case(numa: bool) -> Case:
    """700 nodes, rows from the tight cluster's FitError pods (fit_status_util.status_case), the dry run at the end
    state of the whole queue. The quota never binds: used_limit = used + the pod's request."""
    from tests import fit_status_util as fs
    c, _, st = fs.status_case(700, 512, 3 if numa else 0, numa)
    node_idx, res = make_residents(c, resident_counts(c, (0, 2, 5, 8, 12, 16), 11), 12)
    used = quota_used(res)
    ks = st.order
    if numa:   # first the FitError pods some node could hold whose row has an UnschedulableAndUnresolvable node
        unres = [k for k in ks if c.pods[k]["requests"][0] < 100_000 and
                 any(fw_code(int(w)) == 2 for w in np.unique(st.rows[k]).tolist())]
        ks = unres + [k for k in ks if k not in set(unres)]
    rows = np.stack([st.rows[k] for k in ks])
    pre = np.stack([make_preemptor(c.pods[k], r, used, used + c.pods[k]["requests"][:2]) for r, k in enumerate(ks)])
    return Case(c, numa, None, node_idx, res, rows, pre, ks)


@functools.lru_cache(maxsize=None)
def last_pod_case() -> Case:
    """row_case(False) cut after its second FitError pod: that pod is the last of the queue, so the state of the dry
    run is the state of the pod's own turn."""
    rc = row_case(False)
    k = rc.pod_of[1]
    pre = rc.preemptors[1:2].copy()
    pre["row"] = 0
    return Case(rc.c, False, k + 1, rc.node_idx, rc.residents, rc.rows[1:2], pre, [k])


@functools.lru_cache(maxsize=None)
def quota_case() -> Case:
    """700 nodes, preemptors the quota gate rejected (row = -1: every node is potential): used + request exceeds
    used_limit by a few CPUs, so a node is a candidate only if its tracked victims free that much; then a skip
    preemptor (no quota) and a PreemptNever one."""
    c = fd.tight_cluster(700, 16, 0, False)
    node_idx, res = make_residents(c, resident_counts(c, (0, 2, 5, 8, 12, 16), 21), 22)
    used = quota_used(res)
    pre = []
    for k, over in enumerate((2000, 5000, 9000)):
        p = c.pods[k].copy()
        p["requests"][0] = p["nonzero_requests"][0] = (2000, 4000, 1000)[k]
        p["request_mask"] |= 3
        pre.append(make_preemptor(p, -1, used, used + p["requests"][:2] - np.array([over, 0])))
    pre.append(make_preemptor(c.pods[3], -1, used, used, quota=-1))
    pre.append(make_preemptor(c.pods[4], -1, used, used, flags=abi.GS_PREEMPT_NEVER))
    # a quota with room (another PreFilter rejected the pod): where the pod fits, everybody is reprieved
    pre.append(make_preemptor(pre[1]["pod"], -1, used, used + pre[1]["pod"]["requests"][:2]))
    # nominated to a node that holds a terminating lower-priority pod of its quota: not eligible
    t = np.nonzero(((res["flags"] & abi.GS_RESIDENT_TERMINATING) != 0) & (res["quota"] == QUOTA) & (res["priority"] < PRIO))[0]
    pre.append(make_preemptor(pre[1]["pod"], -1, used, used + pre[1]["pod"]["requests"][:2], nominated=int(node_idx[t[0]])))
    return Case(c, False, 0, node_idx, res, None, np.stack(pre))


NUMA_PREEMPTORS = (0, 2, 13)   # row_case(True): two with UnschedulableAndUnresolvable nodes, one on amplified nodes


@functools.lru_cache(maxsize=None)
def boundary_case() -> Case:
    """257 nodes (one past the kernel's first workgroup), 1 preemptor, residents per node from {0, 1, 2, 63, 64, 65,
    128}: both victim words and the full list. The row is the pod's Filter status on the loaded cluster."""
    from tests import fit_status_util as fs
    c = fd.tight_cluster(257, 8, 0, False)
    counts = np.array((0, 1, 2, 63, 64, 65, 128))[np.arange(257) % 7]
    c.nodes["allowed_pod_number"] = 200
    c.nodes["pod_count"] = np.maximum(c.nodes["pod_count"], counts)
    node_idx, res = make_residents(c, counts, 31)
    pod = c.pods[0].copy()
    pod["requests"][0] = pod["nonzero_requests"][0] = 6000
    pod["request_mask"] |= 3
    o = orc.Oracle(fd.make_cfg(c, False))
    synth.load_into(o, c)
    rows = fs.project(fd.codes_of(o, np.array([pod]))[0], fd.scalar_mask_of(pod))[None, :]
    o.close()
    used = quota_used(res)
    pre = np.stack([make_preemptor(pod, 0, used, used + pod["requests"][:2])])
    return Case(c, False, 0, node_idx, res, rows, pre)
