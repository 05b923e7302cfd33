"""The preemption dry run with PodDisruptionBudgets: the truth, restated over the pieces of tests/preempt_util.py.

filterPodsWithPDBViolation (preempt.go:222-267) is restated literally: one private counter per PDB, decremented for
every potential victim in MoreImportantPod order, the pod violating iff one of its counters is then below zero. The
reprieve runs the violating group first, then the non-violating one, with the step of preempt_util.dry_run (add back,
the oracle's Filter, the quota check, the double removal); numViolatingVictim counts the violating pods whose Filter
failed; the victims stay in reprieve order; pickOneNodeForPreemption has its six criteria. Matching (namespace,
selector, DisruptedPods) is the caller's: a case hands over, per resident, the ids that would be decremented."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from koordinator_amd import abi
from tests import fit_diag_util as fd
from tests import preempt_util as pu
from tests.preempt_util import CANDIDATE, ERROR, FITS, NO_VICTIMS, UNFIT, Table, exceeds, fw_code, make_residents  # noqa: F401

NONE, UNLIMITED = abi.GS_PDB_NONE, abi.GS_PDB_UNLIMITED


# ---- filterPodsWithPDBViolation ----
def partition_literal(lists, budgets) -> list[bool]:
    """lists: per potential victim, in order, the ids of the PDBs decremented for it; budgets: {id: DisruptionsAllowed}
    (an id that is not there: no such PDB). -> violating flag per pod, by the reference's running counters."""
    left = dict(budgets)
    out = []
    for ids in lists:
        violating = False
        for p in ids:
            if p not in left:
                continue
            left[p] -= 1
            if left[p] < 0:
                violating = True
        out.append(violating)
    return out


def partition_counting(lists, budgets) -> list[bool]:
    """The rule the kernel uses: pod j is violating iff for some PDB p it lists, the pods at positions <= j that list p
    outnumber budgets[p]."""
    out = []
    for j, ids in enumerate(lists):
        out.append(any(sum(p in lists[q] for q in range(j + 1)) > budgets.get(p, UNLIMITED) for p in ids))
    return out


# ---- pickOneNodeForPreemption, in full ----
def pick(cands):
    """cands: [(node, num_pdb_violations, first_priority, sum_priorities, num_victims, earliest_start_ns)] ->
    (index of the pick, the criterion 1..6 that decided it (0: a single candidate), the indices still alive when that
    criterion was applied); (-1, 0, []) for none."""
    if not cands:
        return -1, 0, []
    alive = list(range(len(cands)))
    if len(alive) == 1:
        return alive[0], 0, alive
    steps = [(1, lambda c: c[1], min), (2, lambda c: c[2], min), (3, lambda c: c[3], min), (4, lambda c: c[4], min),
             (5, lambda c: c[5], max), (6, lambda c: c[0], min)]
    for crit, key, best in steps:
        before = alive
        b = best(key(cands[i]) for i in alive)
        alive = [i for i in alive if key(cands[i]) == b]
        if len(alive) == 1:
            return alive[0], crit, before
    return alive[0], 6, before


def earliest_start(victims) -> int:
    """[upstream] GetEarliestPodStartTime: walks all victims, the maximum priority met so far and the earliest start
    among the victims of that priority."""
    top, earliest = int(victims[0]["priority"]), int(victims[0]["start_time_ns"])
    for v in victims:
        p, s = int(v["priority"]), int(v["start_time_ns"])
        if p == top:
            earliest = min(earliest, s)
        elif p > top:
            top, earliest = p, s
    return earliest


def key_of(node: int, nviol: int, victims) -> tuple:
    """victims in slice order (violating group first)"""
    return (node, nviol, int(victims[0]["priority"]), sum(int(v["priority"]) + (1 << 31) for v in victims),
            len(victims), earliest_start(victims))


def candidate_array(cands) -> np.ndarray:
    a = np.zeros(len(cands), abi.PREEMPT_CANDIDATE_PDB_DTYPE)
    for i, (node, nviol, first, total, n, earliest) in enumerate(cands):
        a[i] = (node, first, total, n, nviol, earliest)
    return a


# ---- the dry run ----
@dataclasses.dataclass
class Answer:
    status: int
    node: int
    victims: list                    # uids in slice order: violating victims, then non-violating ones
    num_pdb_violations: int
    num_potential: int
    num_candidates: int
    num_errors: int
    node_status: np.ndarray          # uint8[N]
    victim_bits: np.ndarray          # uint64[N][2]
    violating_bits: np.ndarray       # uint64[N][2], zero unless the node is a candidate
    pdb_violations: np.ndarray       # uint8[N]
    cands: list                      # the candidates' pick keys, ascending node
    decided_at: int
    alive_at_decision: list          # nodes still alive when the deciding criterion was applied
    partitions: dict                 # node -> (potential positions, violating positions), every node with victims to try
    error_in_violating_sweep: int    # Error nodes whose double removal happened in the violating sweep
    first_below_top: list            # candidate nodes whose first victim's priority is below their highest


def bits_of(positions) -> np.ndarray:
    w = np.zeros(2, np.uint64)
    for j in positions:
        w[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return w


def dry_run(o, nodes: np.ndarray, table: Table, pre, rows, lists: dict, budgets: dict) -> Answer:
    """One preemptor on the oracle's state, as preempt_util.dry_run; lists: {uid: ids}, budgets: {id: allowed}."""
    N = len(nodes)
    z2 = lambda: np.zeros((N, 2), np.uint64)   # noqa: E731
    zero = Answer(abi.GS_PREEMPT_NOT_ELIGIBLE, -1, [], 0, 0, 0, 0, np.zeros(N, np.uint8), z2(), z2(),
                  np.zeros(N, np.uint8), [], 0, [], {}, 0, [])
    prio, quota, row = int(pre["priority"]), int(pre["quota"]), int(pre["row"])
    skip = quota < 0
    if int(pre["flags"]) & abi.GS_PREEMPT_NEVER:
        return zero
    nom = int(pre["nominated_node"])
    if nom >= 0 and not (row >= 0 and fw_code(int(rows[row][nom])) == 2):
        if any(int(r["flags"]) & abi.GS_RESIDENT_TERMINATING and int(r["quota"]) == quota and int(r["priority"]) < prio
               for r in table.nodes[nom]):
            return zero
    potential = list(range(N)) if row < 0 else [i for i in range(N) if fw_code(int(rows[row][i])) != 2]
    status = np.zeros(N, np.uint8)
    bits, viol, nviol = z2(), z2(), np.zeros(N, np.uint8)
    pod = np.array([pre["pod"]], abi.POD_DTYPE)
    work = nodes.copy()

    def evaluate(changed):
        if changed:
            idx = np.array(changed, np.uint32)
            o.upsert_nodes(work[idx], idx)
        return fd.codes_of(o, pod)[0]

    def move(i, r, sign, used):
        work["requested"][i] += sign * r["requests"]
        work["pod_count"][i] += sign
        pu.move_used(r, sign, used, skip)

    # the potential victims leave; filterPodsWithPDBViolation over them, before any reprieve
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
        flags = partition_literal([lists.get(int(res[j]["uid"]), ()) for j in pv], budgets)
        vio = [j for j, f in zip(pv, flags) if f]
        seq = vio + [j for j, f in zip(pv, flags) if not f]     # the two sweeps
        state[i] = dict(pv=pv, vio=set(vio), seq=seq, used=used, victims=[], nviol=0, err=False, err_vio=False)
    codes = evaluate(list(state))
    for i in list(state):
        if codes[i]:
            status[i] = UNFIT
            del state[i]
    step = 0
    while True:
        cur = [i for i, s in state.items() if not s["err"] and step < len(s["seq"])]
        if not cur:
            break
        for i in cur:
            s = state[i]
            move(i, table.nodes[i][s["seq"][step]], +1, s["used"])
        codes = evaluate(cur)
        for i in cur:
            s = state[i]
            j = s["seq"][step]
            r = table.nodes[i][j]
            removed = False
            if codes[i]:                       # !fits: a victim, and counted when it is of the violating group
                move(i, r, -1, s["used"])
                removed = True
                s["victims"].append(j)
                if j in s["vio"]:
                    s["nviol"] += 1
            if exceeds(pre, s["used"]):
                if removed:
                    s["err"] = True
                    s["err_vio"] = j in s["vio"]
                    continue
                move(i, r, -1, s["used"])
                s["victims"].append(j)          # through the quota check alone: not counted
        step += 1
    o.upsert_nodes(nodes)
    cands, nerr, err_vio, below = [], 0, 0, []
    for i, s in sorted(state.items()):
        if s["err"]:
            status[i] = ERROR
            nerr += 1
            err_vio += s["err_vio"]
            continue
        if not s["victims"]:
            status[i] = FITS
            continue
        status[i] = CANDIDATE
        bits[i] = bits_of(s["victims"])
        viol[i] = bits_of(s["vio"])
        nviol[i] = s["nviol"]
        v = [table.nodes[i][j] for j in s["victims"]]
        cands.append(key_of(i, s["nviol"], v))
        if int(v[0]["priority"]) < max(int(x["priority"]) for x in v):
            below.append(i)
    k, crit, alive = pick(cands)
    ans = Answer(abi.GS_PREEMPT_NO_CANDIDATES, -1, [], 0, len(potential), len(cands), nerr, status, bits, viol, nviol,
                 cands, crit, [cands[i][0] for i in alive], {i: (s["pv"], sorted(s["vio"])) for i, s in state.items()},
                 err_vio, below)
    if not potential:
        ans.status = abi.GS_PREEMPT_NO_POTENTIAL_NODES
    elif k >= 0:
        ans.status = abi.GS_PREEMPT_NOMINATED
        ans.node = cands[k][0]
        ans.num_pdb_violations = cands[k][1]
        ans.victims = [int(table.nodes[ans.node][j]["uid"]) for j in state[ans.node]["victims"]]
    elif nerr:
        ans.status = abi.GS_PREEMPT_ERROR
    return ans


def victims_in_order(table: Table, i: int, bits, viol) -> list:
    """The victims' records of node i in slice order from the two mask pairs."""
    has = lambda w, j: int(w[j >> 6]) >> (j & 63) & 1   # noqa: E731
    n = len(table.nodes[i])
    return [table.nodes[i][j] for j in range(n) if has(bits, j) and has(viol, j)] + \
        [table.nodes[i][j] for j in range(n) if has(bits, j) and not has(viol, j)]


def check(res, status, bits, viol, nviol, k: int, ans: Answer, table: Table):
    """Preemptor k of one gs_preempt_dry_run_pdb call against the truth: the four detail arrays, the result struct with
    the victims' order, and gs_preempt_pick_node_pdb over the detail arrays."""
    for name, got, want in (("node_status", status[k], ans.node_status), ("pdb_violations", nviol[k], ans.pdb_violations)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"preemptor {k}: {name} differs at {bad.size} nodes, first {bad[0]}: gpu {got[bad[0]]} truth {want[bad[0]]}"
    for name, got, want in (("victim_bits", bits[k], ans.victim_bits), ("violating_bits", viol[k], ans.violating_bits)):
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"preemptor {k}: {name} differs at node {bad[0]}: gpu {got[bad[0]]} truth {want[bad[0]]}"
    r = res[k]
    assert (int(r["status"]), int(r["node"])) == (ans.status, ans.node), (k, r["status"], r["node"], ans.status, ans.node)
    assert int(r["num_victims"]) == len(ans.victims) and r["victims"][:len(ans.victims)].tolist() == ans.victims, k
    assert (r["victims"][len(ans.victims):] == 0).all()
    assert (int(r["num_potential"]), int(r["num_candidates"]), int(r["num_errors"]), int(r["num_pdb_violations"])) == \
        (ans.num_potential, ans.num_candidates, ans.num_errors, ans.num_pdb_violations), k
    cands = [key_of(i, int(nviol[k][i]), victims_in_order(table, i, bits[k][i], viol[k][i]))
             for i in np.nonzero(status[k] == CANDIDATE)[0].tolist()]
    j = abi.preempt_pick_node_pdb(candidate_array(cands)) if cands else -1
    assert (cands[j][0] if j >= 0 else -1) == int(r["node"]), k


# ---- the cases: preempt_util's, with memberships and budgets ----
@dataclasses.dataclass
class PdbCase:
    base: pu.Case
    preemptors: np.ndarray           # PREEMPTOR_DTYPE (the base's, some with another priority)
    pdb_ids: np.ndarray              # uint16[M][4], aligned with base.residents
    budget_ids: np.ndarray           # uint32[B]
    budget_allowed: np.ndarray       # int32[B]
    _answers: dict = dataclasses.field(default_factory=dict)
    _plain: dict = dataclasses.field(default_factory=dict)

    @property
    def lists(self) -> dict:
        return {int(u): tuple(int(x) for x in row if x != NONE) for u, row in zip(self.base.residents["uid"], self.pdb_ids)}

    @property
    def budgets(self) -> dict:
        return {int(i): int(a) for i, a in zip(self.budget_ids, self.budget_allowed) if a != UNLIMITED}

    def _state(self):
        self.base.answers([])           # builds the oracle's end state
        return self.base._state

    def answers(self, ks, lists=None, budgets=None) -> list[Answer]:
        """The truth of preemptors ks with the case's lists and budgets (cached), or with the ones given."""
        o, nodes, table = self._state()
        if lists is not None or budgets is not None:
            return [dry_run(o, nodes, table, self.preemptors[k], self.base.rows, self.lists if lists is None else lists,
                            self.budgets if budgets is None else budgets) for k in ks]
        ls, bs = self.lists, self.budgets
        for k in ks:
            if k not in self._answers:
                self._answers[k] = dry_run(o, nodes, table, self.preemptors[k], self.base.rows, ls, bs)
        return [self._answers[k] for k in ks]

    def plain(self, ks) -> list[pu.Answer]:
        """The non-PDB truth (preempt_util.dry_run) of the same preemptors."""
        o, nodes, table = self._state()
        for k in ks:
            if k not in self._plain:
                self._plain[k] = pu.dry_run(o, nodes, table, self.preemptors[k], self.base.rows)
        return [self._plain[k] for k in ks]


def random_lists(residents, seed: int, ids, weights=(35, 35, 20, 0, 10)) -> np.ndarray:
    """uint16[M][4]: per resident 0..4 distinct ids out of `ids` (weights: percent with 0, 1, 2, 3, 4 memberships)."""
    s = np.random.RandomState(seed)
    M = len(residents)
    out = np.full((M, abi.GS_MAX_POD_PDBS), NONE, np.uint16)
    n = np.searchsorted(np.cumsum(weights), s.randint(0, 100, M), side="right")
    for m in range(M):
        out[m, :n[m]] = s.permutation(ids)[:n[m]]
    return out


ALL_Y = 65534     # the highest id: budget -1, so every pod that lists it is violating


def all_violating(case: pu.Case, pdb_ids: np.ndarray, nodes) -> None:
    """Every resident of `nodes` lists ALL_Y alone: all its potential victims are violating, so the reprieve order and
    the victim set are the non-PDB ones and every Filter-failed victim counts."""
    m = np.isin(case.node_idx, np.asarray(list(nodes), np.uint32))
    pdb_ids[m] = NONE
    pdb_ids[m, 0] = ALL_Y


ROW_IDS = np.array([0, 1, 2, 3, 4, 5, 7, 100], np.uint32)
ROW_ALLOWED = np.array([-1, 0, 1, 1, 0, 2, 1, 0], np.int32)
ROW_C = 2           # the preemptor whose pick the violation count decides
ROW_FIRST = 5       # the preemptor whose pick criterion 2 decides, on the priority of the first victim in slice order
ROW_EARLIEST = 6    # the preemptor whose pick criterion 5 decides, on GetEarliestPodStartTime's general rule
ROW_KS = (1, ROW_C, ROW_FIRST)     # the three-preemptor call; 1: priority PRIO - 2. ROW_EARLIEST: in the 128-call
# Shaped nodes of ROW_FIRST (quota 8) and ROW_EARLIEST (quota 9): node -> (quota, priority of the first victim b,
# priority of the other victim a, start of b, start of a; priorities relative to PRIO, starts in seconds).
# Each node holds two potential victims of row_case's preemptor ROW_C, a more important than b. They move to a quota
# of their own, so they are the only potential victims of the shaped preemptor; b alone lists ALL_Y, so b is violating
# and is reprieved first, fails the Filter and stands first in the slice, below a.
#   quota 8: node 50's first victim (-900) lies below node 114's (-850): criterion 2 picks 50. Read as "the highest
#            victim priority" (-700 against -750) it would pick 114.
#   quota 9: the same priorities on both nodes; the highest-priority victim a started later on 122 (100 s against 50 s):
#            criterion 5 picks 122. With the start of the first victim's priority class (10 s against 20 s) it would
#            pick 424.
SHAPED = {50: (8, -900, -700, 30, 40), 114: (8, -850, -750, 30, 40),
          122: (9, -900, -700, 10, 100), 424: (9, -900, -700, 20, 50)}


def shaped_row_base():
    """preempt_util.row_case(False) with the shaped nodes' residents, and the two shaped preemptors (the pod and row of
    preemptor ROW_C, quotas 8 and 9, a quota that never binds). -> (Case, the uids of the first victims b)."""
    b0 = pu.row_case(False)
    res = b0.residents.copy()
    at = {int(u): m for m, u in enumerate(res["uid"])}
    table = b0.table()
    t0 = int(b0.c.now_ns) - 7200 * 10**9
    firsts = []
    for node, (quota, pb, pa, sb, sa) in SHAPED.items():
        pv = [at[int(r["uid"])] for r in table.nodes[node] if not int(r["flags"]) & abi.GS_RESIDENT_NON_PREEMPTIBLE and
              int(r["priority"]) < pu.PRIO and int(r["quota"]) == pu.QUOTA]
        assert len(pv) == 2, node
        ma, mb = pv
        res["quota"][[ma, mb]] = quota
        res["priority"][ma], res["priority"][mb] = pu.PRIO + pa, pu.PRIO + pb
        res["start_time_ns"][ma], res["start_time_ns"][mb] = t0 + sa * 10**9, t0 + sb * 10**9
        firsts.append(int(res["uid"][mb]))
    pre = b0.preemptors.copy()
    pod = b0.c.pods[b0.pod_of[ROW_C]]
    for k, quota in ((ROW_FIRST, 8), (ROW_EARLIEST, 9)):
        used = pu.quota_used(res, quota)
        pre[k] = pu.make_preemptor(pod, int(pre[ROW_C]["row"]), used, used + pod["requests"][:2], quota=quota)
    return pu.Case(b0.c, False, None, b0.node_idx, res, b0.rows, pre, b0.pod_of), firsts


@functools.lru_cache(maxsize=None)
def row_case(numa: bool) -> PdbCase:
    """preempt_util.row_case with 0..4 memberships per resident out of eight PDBs with budgets -1..2, plus id 9 that
    is listed and never upserted. Fit + LoadAware: preemptor 1 has priority PRIO - 2 (another potential set on the
    same nodes); the candidates of preemptor ROW_C that tie at the fewest violations, but one, list ALL_Y alone, so
    that its pick is decided by the violation count; and the SHAPED nodes with their two preemptors."""
    firsts = []
    base = pu.row_case(numa)
    if not numa:
        base, firsts = shaped_row_base()
    ids = random_lists(base.residents, 5 if numa else 41, np.concatenate([ROW_IDS, [9]]).astype(np.uint16))
    pre = base.preemptors.copy()
    bid = np.concatenate([ROW_IDS, [ALL_Y]]).astype(np.uint32)
    ball = np.concatenate([ROW_ALLOWED, [-1]]).astype(np.int32)
    case = PdbCase(base, pre, ids, bid, ball)
    if not numa:
        pre[1]["priority"] = pu.PRIO - 2
        a, = case.answers([ROW_C])
        old, = case.plain([ROW_C])
        low = min(c[1] for c in a.cands)
        tie = [c[0] for c in a.cands if c[1] == low]
        keep = [i for i in tie if i != old.node][0]
        all_violating(base, ids, [i for i in tie if i != keep])
        shaped = np.isin(base.residents["quota"], (8, 9))       # (no potential victims of the other preemptors)
        ids[shaped] = NONE
        ids[np.isin(base.residents["uid"], firsts), 0] = ALL_Y
        case = PdbCase(base, pre, ids, bid, ball)
    return case


def mutated_picks(case: PdbCase, k: int):
    """The node preemptor k would nominate with two wrong key rules, from the truth's victims in slice order:
    (`first` = the highest victim priority, `earliest` = the earliest start among the victims of the FIRST victim's
    priority): what gs_preempt_dry_run's kernel computes for its MoreImportantPod-ordered victims."""
    a, = case.answers([k])
    table = case.base.table()
    by_first, by_earliest = [], []
    for c in a.cands:
        v = victims_in_order(table, c[0], a.victim_bits[c[0]], a.violating_bits[c[0]])
        by_first.append(c[:2] + (max(int(x["priority"]) for x in v),) + c[3:])
        by_earliest.append(c[:5] + (min(int(x["start_time_ns"]) for x in v if int(x["priority"]) == int(v[0]["priority"])),))
    return by_first[pick(by_first)[0]][0], by_earliest[pick(by_earliest)[0]][0]


@functools.lru_cache(maxsize=None)
def quota_case() -> PdbCase:
    base = pu.quota_case()
    ids = random_lists(base.residents, 43, ROW_IDS.astype(np.uint16), weights=(30, 40, 20, 0, 10))
    return PdbCase(base, base.preemptors.copy(), ids, ROW_IDS, ROW_ALLOWED)


BOUNDARY_PDB = 0           # the PDB whose budget runs out between list positions 63 and 64


@functools.lru_cache(maxsize=None)
def boundary_case() -> PdbCase:
    """preempt_util.boundary_case. On the nodes with 65 and 128 residents every resident is made a potential victim
    (preemptible, the preemptor's quota, priority below its) and BOUNDARY_PDB, budget 33, is listed by the pods at the
    even positions 0..62 and by positions 63, 64, ..: its 33 allowed disruptions end with position 63, the last
    non-violating match, and position 64 is the first violating one. The other nodes: 0, 1 or 4 memberships out of ids
    {1, 2, 3, 65534, 9} with budgets 1, 0, -1, 1 and never upserted."""
    b0 = pu.boundary_case()
    res = b0.residents.copy()
    counts = np.bincount(b0.node_idx, minlength=257)
    big = np.isin(b0.node_idx, np.nonzero(counts >= 65)[0])
    res["flags"][big] &= ~np.uint32(abi.GS_RESIDENT_NON_PREEMPTIBLE)
    res["quota"][big] = pu.QUOTA
    res["priority"][big] = np.minimum(res["priority"][big], pu.PRIO - 1)
    used = pu.quota_used(res)
    pod = b0.preemptors[0]["pod"]
    pre = np.stack([pu.make_preemptor(pod, 0, used, used + pod["requests"][:2])])
    base = pu.Case(b0.c, False, 0, b0.node_idx, res, b0.rows, pre)
    ids = random_lists(res, 47, np.array([1, 2, 3, ALL_Y, 9], np.uint16), weights=(40, 40, 0, 0, 20))
    table = base.table()
    pos = {int(r["uid"]): j for i in np.nonzero(counts >= 65)[0].tolist() for j, r in enumerate(table.nodes[i])}
    for m in np.nonzero(big)[0].tolist():
        j = pos[int(res["uid"][m])]
        ids[m] = NONE
        if j >= 63 or j % 2 == 0:
            ids[m, 0] = BOUNDARY_PDB
    return PdbCase(base, pre, ids, np.array([BOUNDARY_PDB, 1, 2, 3, ALL_Y], np.uint32),
                   np.array([33, 1, 0, -1, 1], np.int32))
