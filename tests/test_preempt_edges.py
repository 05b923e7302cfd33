"""The preemption edge family without a GPU: the input conditions of tests/test_gpu_preempt_edges.py, asserted on the
truth alone (tests/preempt_edges_util.py over the CPU oracle), so that no GPU test passes vacuously; the host pick
(gs_preempt_pick_node / gs_preempt_pick_node_pdb, the order the kernels share) on every designed candidate set; and
the truth's correction (a resident's quota request counts over its own keys only) against the existing cases."""
import numpy as np
import pytest

from koordinator_amd import abi, build
from tests import preempt_edges_util as pe
from tests import preempt_pdb_util as pp
from tests import preempt_util as pu


@pytest.fixture(scope="module")
def lib():
    build.build()
    return abi.load()


def both(ec: pe.EdgeCase):
    ks = list(range(len(ec.names)))
    return ec.base.answers(ks), ec.pdb.answers(ks)


def host_picks(a, b):
    """the nodes the two host picks nominate over the truth's candidate keys"""
    j = abi.preempt_pick_node(pu.candidate_array(a.cands)) if a.cands else -1
    k = abi.preempt_pick_node_pdb(pp.candidate_array(b.cands)) if b.cands else -1
    return (a.cands[j][0] if j >= 0 else -1), (b.cands[k][0] if k >= 0 else -1)


def expectations_hold(ec: pe.EdgeCase):
    A, B = both(ec)
    for k in range(len(ec.names)):
        pe.check_expect(ec, k, A[k], B[k])
        assert host_picks(A[k], B[k]) == (A[k].node, B[k].node), ec.names[k]
    return A, B


# ---- 1. pick positions x criteria ----
def test_pick_section_shape():
    """258 parts: the pick kernel's second stride holds parts 256 and 257, and the last workgroup owns one node. The
    anchors stand in lane 0 and 63 of a wave, the first and last lane of a workgroup, the first lane of the pick
    kernel's wave 1 (part 64), its last thread (part 255) and both parts of the second stride."""
    N = pe.PICK_N
    assert (N + 255) // 256 == 258 and N - 257 * 256 == 1
    assert [a // 256 for a in pe.ANCHORS] == [0, 0, 0, 0, 1, 63, 64, 255, 256, 257]
    assert [a % 256 for a in pe.ANCHORS] == [0, 63, 64, 255, 0, 255, 0, 255, 0, 0]
    ps = pe.pick_section()
    assert len(ps.batches) == pe.PICK_BATCHES and all(len(b.names) <= pe.BATCH for b in ps.batches)
    assert len({cf.quota for cf in ps.configs}) == len(ps.configs)
    counts = np.bincount(np.concatenate([b.base.node_idx for b in ps.batches]), minlength=N)
    assert set(np.nonzero(counts)[0].tolist()) == set(pe.ANCHORS)       # residents on the anchors alone


@pytest.mark.parametrize("b", range(pe.PICK_BATCHES))
def test_pick_batch_conditions(lib, b):
    """Every configuration of batch b nominates the anchor it was built for, on the criterion it was built for, and
    the host pick agrees; the order without the deciding criterion nominates another node, and so does the order with
    that criterion inverted. (Anchor 0 cannot be worse in the node index: where it wins on criterion 5 nothing later
    is against it, so there only the inverted criterion nominates another node.)"""
    ps = pe.pick_section()
    A, B = ps.answers(b)
    for k, (a, p) in enumerate(zip(A, B)):
        cf = ps.config_of(b, k)
        assert a.num_potential == p.num_potential == pe.PICK_N
        assert host_picks(a, p) == (a.node, p.node), cf.name
        if not cf.crit:
            continue
        single = len(cf.present) == 1
        assert p.node == cf.winner and p.decided_at == (0 if single else cf.crit), cf.name
        assert p.num_candidates == a.num_candidates == len(cf.present)
        assert [c[0] for c in p.cands] == list(cf.present)          # every anchor present is a candidate
        if cf.crit == 1:      # the old call does not see the violations: the others tie, the lowest of them wins
            assert a.node == min(x for x in cf.present if x != cf.winner) and a.decided_at == 6
            assert p.num_pdb_violations == 0 and sorted(c[1] for c in p.cands) == [0] + [1] * 9
        else:                 # the anchors tie at one violation each
            assert a.node == cf.winner and a.decided_at == p.decided_at
            assert {c[1] for c in p.cands} == {1}
        if single:
            continue
        for cands, node, crit in ((p.cands, p.node, p.decided_at), (pe.pdb_form(a.cands), a.node, a.decided_at)):
            dropped = pe.pick_order(cands, drop=crit)
            assert pe.pick_order(cands) == node
            assert dropped != node or (node == cands[0][0] and crit == 5), (cf.name, crit)
            assert pe.pick_order(cands, invert=crit) != node, (cf.name, crit)
            # the winner is strictly worse in every later criterion it can be worse in
            w = next(c for c in cands if c[0] == node)
            for later in range(crit + 1, 7):
                f, best = pe.STEPS[later]
                others = [c[f] for c in cands if c[0] != node]
                if later == 6:      # worse in the node index: not the lowest candidate, unless it is anchor 0
                    assert node > min(others) or node == pe.ANCHORS[0], (cf.name, crit)
                    continue
                assert all((w[f] > o) if best is min else (w[f] < o) for o in others), (cf.name, crit, later)


def test_pick_every_anchor_wins_on_every_criterion():
    """decided_at takes every value 2..6 (1..6 with PDBs), and under each every anchor wins at least once"""
    ps = pe.pick_section()
    won = {c: set() for c in range(1, 7)}
    won_plain = {c: set() for c in range(2, 7)}
    for b in range(len(ps.batches)):
        for a, p in zip(*ps.answers(b)):
            if p.decided_at:
                won[p.decided_at].add(p.node)
            if a.decided_at:
                won_plain[a.decided_at].add(a.node)
    anchors = set(pe.ANCHORS)
    for c in range(1, 6):
        assert won[c] == anchors, c
    for c in range(2, 6):
        assert won_plain[c] == anchors, c
    # criterion 6 needs a second candidate above the winner: every anchor but the last
    assert won[6] == anchors - {pe.ANCHORS[-1]} and won_plain[6] >= won[6]


def test_pick_section_error_and_no_candidate():
    ps = pe.pick_section()
    b = len(ps.batches) - 1
    A, B = ps.answers(b)
    names = ps.batches[b].names
    for ans in (A, B):
        e, n = ans[names.index("error")], ans[names.index("nocand")]
        assert (e.status, e.num_errors, e.num_candidates, e.num_potential) == (abi.GS_PREEMPT_ERROR, len(pe.ANCHORS), 0, pe.PICK_N)
        assert (e.node_status[list(pe.ANCHORS)] == pu.ERROR).all() and (e.node_status == pu.ERROR).sum() == len(pe.ANCHORS)
        assert (n.status, n.num_errors, n.num_candidates, n.num_potential) == (abi.GS_PREEMPT_NO_CANDIDATES, 0, 0, pe.PICK_N)
        assert (n.node_status[list(pe.ANCHORS[::2])] == pu.UNFIT).all()
        assert set(np.unique(n.node_status).tolist()) == {pu.UNFIT, pu.NO_VICTIMS}


# ---- 2. the two launches ----
def test_numa_case_conditions(lib):
    ec = pe.numa_case()
    A, B = expectations_hold(ec)
    policy = ec.base.c.numa["node_numa"]["numa_topology_policy"] != abi.GS_NUMA_POLICY_NONE
    seen = []
    for a in A:
        (n0, *k0), (n1, *k1) = a.cands
        assert k0 == k1 and n0 < n1 and a.decided_at == 6 and a.node == n0       # tied through criterion 5
        assert policy[n0] != policy[n1]
        assert a.node_status[n0] == a.node_status[n1] == pu.CANDIDATE
        seen.append(bool(policy[n0]))
    assert seen == [True, False]          # the policy node at the lower index, then at the higher


# ---- 3. key values ----
LOW, HIGH = (lambda x: x & 0xFFFFFFFF), (lambda x: x >> 32)
# scenario -> (field of preempt_util's key, what a wrong compare reads of it)
WRONG_READS = {"sum-high": (2, LOW), "sum-low": (2, HIGH), "earliest-above-32": (4, LOW), "earliest-below-32": (4, HIGH),
               "earliest-halves-disagree": (4, LOW), "earliest-2^62": (4, lambda x: x & ((1 << 62) - 1)),
               "first-minus-1": (1, LOW)}


def test_key_case_conditions(lib):
    ec = pe.key_case()
    A, _ = expectations_hold(ec)
    for name, (f, read) in WRONG_READS.items():
        a = A[ec.k(name)]
        wrong = [c[:f] + (read(c[f]),) + c[f + 1:] for c in a.cands]
        assert wrong[pu.pick(wrong)[0]][0] != a.node, name
    x, y = A[ec.k("sum-high")].cands
    assert abs(x[2] - y[2]) == 1 << 32 and x[1] == y[1] and x[3] == y[3]
    x, y = A[ec.k("sum-low")].cands
    assert abs(x[2] - y[2]) == 1 and x[2] >> 32 == y[2] >> 32
    assert sorted(c[4] for c in A[ec.k("earliest-0-1")].cands) == [0, 1]
    assert sorted(c[1] for c in A[ec.k("first-int32-min")].cands) == [pe.INT32_MIN, pe.INT32_MIN + 1]
    assert A[ec.k("preemptor-int32-max")].cands[0][1] == pe.INT32_MAX - 1
    a = A[ec.k("preemptor-int32-min")]
    assert (a.node_status == pu.NO_VICTIMS).all()
    a = A[ec.k("128-victims")]
    table = ec.base.table()
    assert len(a.victims) == 128 == abi.GS_MAX_NODE_PODS and a.victims == [int(r["uid"]) for r in table.nodes[a.node]]
    assert a.victims != sorted(a.victims)            # the table's order is not the uids'
    for pos in (63, 64, 127):
        for kind in ("alone", "reprieved"):
            a = A[ec.k(f"lone-{pos}-{kind}")]
            assert len(table.nodes[a.node]) == 128 and a.victims == [int(table.nodes[a.node][pos]["uid"])]
            assert a.non_prefix == (1 if kind == "reprieved" and pos < 127 else 0)


# ---- 4. resource slots and the pod count ----
def test_slot_case_conditions(lib):
    ec = pe.slot_case()
    A, _ = expectations_hold(ec)
    seen = 0
    for a in A:
        seen |= a.only_bits
    assert seen == sum(pu.FIT_BITS)       # each Fit bit is the only failing bit of some reprieve step
    for s in pe.SLOT_Q:
        p = ec.base.preemptors[ec.k(f"slot-{s}")]["pod"]
        assert [d for d in range(7) if p["requests"][d]] == [s]
    m = np.isin(ec.base.node_idx, [n for k in ec.ks("slot-") for n in ec.expect[k]["status"]])
    assert (ec.base.residents["requests"][m][:, :2] == 0).all()      # the residents hold the slot and nothing else


# ---- 5. quota dimensions and masks ----
def test_quota_case_conditions(lib, monkeypatch):
    ec = pe.quota_case()
    A, _ = expectations_hold(ec)
    assert all(int(p["row"]) == -1 for p in ec.base.preemptors)
    for d in range(2, 8):
        a = A[ec.k(f"dim-{d}")]
        assert a.quota_victims_on_fitting == 1         # the quota's doing alone
    assert A[ec.k("error-dim-4")].num_errors == 1
    # moved regardless of the resident's own mask, dimension 3 would make the pod a victim
    k = ec.k("outside-own-mask")
    o, nodes, table = ec.base._state

    def move_all(r, sign, used, skip):
        if skip or not int(r["flags"]) & abi.GS_RESIDENT_QUOTA_TRACKED:
            return
        for d in range(abi.GS_QUOTA_DIMS):
            q = int(r["quota_request"][d])
            used[d] = max(0, used[d] - q) if sign < 0 else used[d] + q
    monkeypatch.setattr(pu, "move_used", move_all)
    assert pu.dry_run(o, nodes, table, ec.base.preemptors[k]).num_candidates == 1 and A[k].num_candidates == 0


def test_existing_cases_hold_nothing_outside_their_masks():
    """preempt_util.move_used honours quota_request_mask; every resident of the existing cases has zeros outside its
    mask, so no existing answer changes. (The cases are the cached ones of tests/test_preempt.py and
    tests/test_preempt_pdb.py: built once per session.)"""
    for res in (pu.row_case(False).residents, pu.row_case(True).residents, pu.quota_case().residents,
                pu.boundary_case().residents, pp.shaped_row_base()[0].residents, pp.boundary_case().base.residents):
        inside = (res["quota_request_mask"][:, None] >> np.arange(abi.GS_QUOTA_DIMS)) & 1
        assert (res["quota_request"][inside == 0] == 0).all()


# ---- 6. rows ----
def test_rows_case_conditions(lib):
    ec = pe.rows_case()
    A, _ = expectations_hold(ec)
    words = pe.class_words()
    codes = [abi.status_framework_code(w) for w in words]
    sh = abi.GS_FAIL_NUMA_SHIFT
    assert {w >> sh & 15 for w in words[:16]} == set(range(16)) and all(w & 0x3F == 0 for w in words[:16])
    assert all(w & 0x1F and not w & pe.LA for w in words[16:32]) and all(w & pe.LA for w in words[32:48])
    # (the malformed words have no framework code at all, -1: nothing says UnschedulableAndUnresolvable, so potential)
    assert {0, 1, 2} <= set(codes) <= {-1, 0, 1, 2} and codes.count(2) >= 10 and set(codes[48:54]) == {-1}
    assert [codes[r] for r in (1, 2, 3, 5, 6, 7, 9)] == [2] * 7 and 2 not in codes[16:48]
    a = A[ec.k("row-5-a")]
    at = np.arange(pe.CLASS_AT, pe.CLASS_AT + len(words))
    want = np.where(np.array(codes) == 2, pu.NOT_POTENTIAL, pu.CANDIDATE)     # every class node would be a candidate
    assert np.array_equal(a.node_status[at], want)
    assert a.num_potential == 257 - codes.count(2) and (a.node_status == pu.NOT_POTENTIAL).sum() == codes.count(2)
    assert (A[ec.k("row-none")].node_status[at] == pu.CANDIDATE).all()
    assert [int(ec.base.preemptors[ec.k(n)]["row"]) for n in pe.ROW_KS] == [5, 2, 5, -1] and len(ec.base.rows) == 7
    assert not A[ec.k("nominated-resolvable")].node_status.any()
    assert A[ec.k("all-unresolvable")].num_potential == 0
