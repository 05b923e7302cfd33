"""gs_preempt_dry_run on the GPU against the restatement over the CPU oracle (tests/preempt_util.py; the cases' input
conditions are asserted in tests/test_preempt.py). Every case compares node_status, victim_bits, the result struct and
gs_preempt_pick_node over the detail arrays with the truth, then checks that the dry run modified nothing: the mirror
still matches the host state and gs_evaluate's codes of the preemptors are unchanged."""
import ctypes as C

import numpy as np
import pytest

from koordinator_amd import abi, synth
from tests import fit_diag_util as fd
from tests import preempt_util as pu

pytestmark = pytest.mark.gpu


def engine(case: pu.Case, residents: bool = True, **kw):
    """An Engine in the case's state: the cluster loaded, the case's pods scheduled first (-> the status rows the
    engine itself reports, in the case's preemptor order), the residents registered."""
    from koordinator_amd.engine import Engine
    c = case.c
    e = Engine(fd.make_cfg(c, case.numa, **kw))
    synth.load_into(e, c)
    rows = None
    pods = c.pods if case.npods is None else c.pods[:case.npods]
    if len(pods):
        _, _, words, row_of = e.schedule_diag_nodes(pods)
        rows = words[[int(row_of[k]) for k in case.pod_of]]
        assert np.array_equal(rows, case.rows)          # the truth's potential nodes come from the same rows
    elif case.rows is not None:
        rows = case.rows
    if residents:
        e.node_pods_add(case.node_idx, case.residents)
    return e, rows


def run_and_check(e, case, ks, rows, table=None):
    pre = case.preemptors[list(ks)]
    pods = np.ascontiguousarray(pre["pod"][:4])
    before = e.evaluate(pods)[1]
    res, status, bits = e.preempt_dry_run(pre, rows)
    table = table or case.table()
    for j, a in enumerate(case.answers(list(ks))):
        pu.check(res, status, bits, j, a, table)
    assert e.mirror_check() == 0
    assert np.array_equal(before, e.evaluate(pods)[1])
    return res, status, bits


def test_grid_boundary_both_mask_words_and_guard_rows():
    """257 nodes: one past the first workgroup; residents per node from {0, 1, 2, 63, 64, 65, 128}. Nothing is written
    outside the n handed-out detail rows."""
    from koordinator_amd.engine import lib
    case = pu.boundary_case()
    e, rows = engine(case)
    for i in (1, 2, 3, 4, 5, 6):     # the table returns each list in MoreImportantPod order
        got = e.node_pods(i)
        want = case.table().nodes[i]
        assert [int(r["uid"]) for r in got] == [int(r["uid"]) for r in want]
    run_and_check(e, case, [0], rows)
    N = 257
    pre = np.ascontiguousarray(case.preemptors[:1])
    out = np.zeros(1, abi.PREEMPT_RESULT_DTYPE)
    status = np.full((3, N), 0xFF, np.uint8)
    bits = np.full((3, N, 2), 0xFFFFFFFFFFFFFFFF, np.uint64)
    d = abi.GsPreemptDetail(node_status=abi.ptr(status), victim_bits=abi.ptr(bits))
    rows = np.ascontiguousarray(rows)
    assert lib().gs_preempt_dry_run(e._h, abi.ptr(pre), 1, abi.ptr(rows), 1, abi.ptr(out), C.byref(d)) == 0
    a, = case.answers([0])
    assert np.array_equal(status[0], a.node_status) and np.array_equal(bits[0], a.victim_bits)
    assert (status[1:] == 0xFF).all() and (bits[1:] == 0xFFFFFFFFFFFFFFFF).all()
    # no detail: the same result
    out2 = np.zeros(1, abi.PREEMPT_RESULT_DTYPE)
    assert lib().gs_preempt_dry_run(e._h, abi.ptr(pre), 1, abi.ptr(rows), 1, abi.ptr(out2), None) == 0
    assert out.tobytes() == out2.tobytes()
    e.close()


def test_rows_of_the_first_fit_errors():
    """700 nodes, Fit + LoadAware: the rows of the engine's own gs_schedule_diag_nodes, the dry run at the end state;
    the first 3 FitError pods, then 128 preemptors in one call."""
    case = pu.row_case(False)
    e, rows = engine(case)
    res, _, _ = run_and_check(e, case, [0, 1, 2], rows)
    assert sorted(res["status"].tolist()) == [abi.GS_PREEMPT_NOMINATED, abi.GS_PREEMPT_NOMINATED,
                                              abi.GS_PREEMPT_NO_CANDIDATES]
    ks = [k % 16 for k in range(128)]
    res, status, bits = run_and_check(e, case, ks, rows)
    for j in range(16, 128):       # the same preemptor gives the same answer wherever it stands in the call
        assert res[j].tobytes() == res[j % 16].tobytes()
        assert np.array_equal(status[j], status[j % 16]) and np.array_equal(bits[j], bits[j % 16])
    e.close()


def test_state_of_the_pods_own_turn():
    """The FitError pod is the last pod of its call: the dry run sees the state of the pod's own turn."""
    case = pu.last_pod_case()
    e, rows = engine(case)
    run_and_check(e, case, [0], rows)
    e.close()


def test_numa_profile():
    """Policy nodes through the index list, potential nodes != all nodes (the UnschedulableAndUnresolvable ones have
    status 0), and reprieves that fail on the amplified-CPU check alone."""
    case = pu.row_case(True)
    e, rows = engine(case)
    ks = list(pu.NUMA_PREEMPTORS)
    _, status, _ = run_and_check(e, case, ks, rows)
    for j, k in enumerate(ks):
        unres = np.array([pu.fw_code(int(w)) == 2 for w in rows[int(case.preemptors[k]["row"])].tolist()])
        assert (status[j][unres] == pu.NOT_POTENTIAL).all() and (status[j][~unres] != pu.NOT_POTENTIAL).all()
    policy = case.c.numa["node_numa"]["numa_topology_policy"] != abi.GS_NUMA_POLICY_NONE
    assert (status[:, policy] == pu.CANDIDATE).any() and (status[:, ~policy] == pu.CANDIDATE).any()
    e.close()


def test_quota_rejected_skip_and_never():
    """row = -1: every node is potential; Error nodes and quota-driven victims; a preemptor without a quota, one with
    PreemptNever, one nominated to a node with a terminating victim."""
    case = pu.quota_case()
    e, rows = engine(case)
    res, status, _ = run_and_check(e, case, range(len(case.preemptors)), rows)
    assert (status[0] == pu.ERROR).sum() >= 5
    assert res["status"].tolist()[3:5] == [abi.GS_PREEMPT_NO_CANDIDATES, abi.GS_PREEMPT_NOT_ELIGIBLE]
    assert res["status"][6] == abi.GS_PREEMPT_NOT_ELIGIBLE and not status[6].any()
    e.close()


def same_answer(x, y):
    for a, b in zip(x, y):
        assert a.tobytes() == b.tobytes()


def test_table_maintenance():
    """Add / remove between dry runs, a node emptied and refilled, the 129th pod refused, gs_reset: each time the
    answer of a context built with the final table in one go."""
    from koordinator_amd.engine import lib
    case = pu.boundary_case()
    pre = case.preemptors[:1]
    ref, rows = engine(case)
    want = ref.preempt_dry_run(pre, rows)
    ref.close()
    e, _ = engine(case, residents=False)
    half = np.arange(len(case.residents)) % 2 == 0
    e.node_pods_add(case.node_idx[half], case.residents[half])
    first = e.preempt_dry_run(pre, rows)
    assert first[0].tobytes() != want[0].tobytes() or not np.array_equal(first[1], want[1])
    extra = case.residents[:3].copy()
    extra["uid"] += 1 << 40
    e.node_pods_add(case.node_idx[:3], extra)                      # three that leave again
    e.node_pods_add(case.node_idx[~half], case.residents[~half])
    e.node_pods_remove(case.node_idx[:3], extra["uid"])
    same_answer(e.preempt_dry_run(pre, rows), want)
    # a node with 128 residents emptied and refilled in another order
    full = int(np.nonzero(np.bincount(case.node_idx, minlength=257) == 128)[0][0])
    m = np.nonzero(case.node_idx == full)[0]
    e.node_pods_remove(case.node_idx[m], case.residents["uid"][m])
    assert len(e.node_pods(full)) == 0
    emptied = e.preempt_dry_run(pre, rows)
    assert emptied[1][0][full] == pu.NO_VICTIMS
    e.node_pods_add(case.node_idx[m[::-1]], case.residents[m[::-1]])
    same_answer(e.preempt_dry_run(pre, rows), want)
    # the 129th pod and a duplicate uid are refused, and nothing of such a call is applied
    one = case.residents[m[:1]].copy()
    idx = np.array([full], np.uint32)
    assert lib().gs_node_pods_add(e._h, abi.ptr(idx), abi.ptr(one), 1) == abi.GS_EINVAL
    one["uid"] += 1 << 41
    assert lib().gs_node_pods_add(e._h, abi.ptr(idx), abi.ptr(one), 1) == abi.GS_EUNSUPPORTED
    two = np.concatenate([one, one])
    two["uid"][1] += 1
    idx2 = np.array([0, full], np.uint32)
    assert lib().gs_node_pods_add(e._h, abi.ptr(idx2), abi.ptr(two), 2) == abi.GS_EUNSUPPORTED
    assert len(e.node_pods(full)) == 128 and len(e.node_pods(0)) == 0
    same_answer(e.preempt_dry_run(pre, rows), want)
    e.reset()
    same_answer(e.preempt_dry_run(pre, rows), want)
    assert e.mirror_check() == 0
    e.close()


def test_refused_on_several_ranks_and_with_extensions():
    """GS_EUNSUPPORTED before any work: no row flushed, no kernel counted, no table created."""
    from koordinator_amd.engine import Engine, GpuScoreError, LocalGroup
    from oracle import oracle as orc
    case = pu.quota_case()
    cfg = fd.make_cfg(case.c, False)
    g = LocalGroup(2)
    ranks = [Engine(cfg) for _ in range(2)]
    for r, x in enumerate(ranks):
        synth.load_into(x, case.c)
        x.comm_init_local(g, r)
    ext = Engine(cfg)
    synth.load_into(ext, case.c)
    ext.ext_configure(orc.ext_args_default())
    for x in ranks + [ext]:
        before = x.stats()
        with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EUNSUPPORTED}"):
            x.preempt_dry_run(case.preemptors[:2], None)
        assert x.stats() == before
        assert len(x.node_pods(0)) == 0
        x.close()
    del g
