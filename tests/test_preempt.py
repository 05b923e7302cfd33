"""ElasticQuota's PostFilter dry run without a GPU: gs_preempt_pick_node against the restated pick, the new structs'
sizes, the restatement (tests/preempt_util.py) on hand cases over a one-node oracle cluster, and the input conditions
of the GPU cases (tests/test_gpu_preempt.py), asserted on the truth alone so that no GPU test passes vacuously."""
import ctypes as C

import numpy as np
import pytest

from koordinator_amd import abi, build
from tests import fit_diag_util as fd
from tests import preempt_util as pu
from tests.preempt_edges_util import CPU, one_node, pod_of, resident


@pytest.fixture(scope="module")
def lib():
    build.build()
    return abi.load()


# ---- gs_preempt_pick_node ----
BASE = (7, 990, 3 * ((1 << 31) + 990), 3, 1_000)   # node, first priority, priority sum, victims, earliest start


def vary(field: int, value):
    c = list(BASE)
    c[0] = 9
    c[field] = value
    return tuple(c)


@pytest.mark.parametrize("crit,other,better", [
    (2, vary(1, 989), True),                         # a lower first priority wins
    (3, vary(2, BASE[2] - 1), True),                 # then the smaller priority sum
    (4, vary(3, 2), True),                           # then fewer victims
    (5, vary(4, 2_000), True),                       # then the LATEST earliest start
    (6, vary(0, 3), True),                           # then the lower node index
    (2, vary(1, 991), False), (3, vary(2, BASE[2] + 1), False), (4, vary(3, 4), False), (5, vary(4, 500), False),
    (6, vary(0, 9), False),
])
def test_pick_each_criterion_alone(lib, crit, other, better):
    """Two candidates that differ in one criterion, in both directions and both list orders."""
    for cands in ([BASE, other], [other, BASE]):
        want = cands.index(other if better else BASE)
        k, decided = pu.pick(cands)
        assert (k, decided) == (want, crit)
        assert abi.preempt_pick_node(pu.candidate_array(cands)) == want


def test_pick_earlier_criteria_dominate(lib):
    a = (1, 990, 100, 9, 0)          # worse in every later criterion
    b = (0, 991, 1, 1, 10**12)
    assert pu.pick([b, a])[0] == 1 and abi.preempt_pick_node(pu.candidate_array([b, a])) == 1
    assert abi.preempt_pick_node(pu.candidate_array([])) == -1 and pu.pick([]) == (-1, 0)


def test_pick_earliest_start_of_two_top_victims(lib):
    """Criterion 5 reads the earliest start among the victims of the HIGHEST priority, not among all victims."""
    def victims(*ps):
        v = np.zeros(len(ps), abi.RESIDENT_POD_DTYPE)
        for r, (prio, start) in zip(v, ps):
            r["priority"], r["start_time_ns"] = prio, start
        return v
    a = pu.key_of(0, victims((990, 500), (990, 300), (980, 1)))     # earliest of the two top victims: 300
    b = pu.key_of(1, victims((990, 400), (990, 350), (980, 900)))   # 350: later, so b wins
    assert (a[4], b[4]) == (300, 350) and a[1:4] == b[1:4]
    assert pu.pick([a, b]) == (1, 5)
    assert abi.preempt_pick_node(pu.candidate_array([a, b])) == 1


def test_pick_random_sets_with_heavy_ties(lib):
    s = np.random.RandomState(3)
    decided = set()
    for _ in range(1000):
        n = int(s.randint(1, 40))
        nodes = s.permutation(200)[:n]
        cands = [(int(nodes[i]), 990 + int(s.randint(0, 2)), 5 * (1 << 31) + int(s.randint(0, 3)), 2 + int(s.randint(0, 2)),
                  int(s.randint(0, 3))) for i in range(n)]
        k, crit = pu.pick(cands)
        decided.add(crit)
        assert abi.preempt_pick_node(pu.candidate_array(cands)) == k
    assert decided >= {2, 3, 4, 5, 6}


def test_struct_sizes(lib):
    names = ["gs_pod", "gs_node", "gs_node_metric", "gs_pod_metric", "gs_config", "gs_placement", "gs_stats",
             "gs_loadaware_args", "gs_cpu_topology", "gs_node_numa", "gs_pod_allocation", "gs_numa_args",
             "gs_quota_group", "gs_quota_status", "gs_node_devices", "gs_reservation", "gs_pod_ext", "gs_ext_args",
             "gs_ext_placement", "gs_status_map", "gs_resident_pod", "gs_preemptor", "gs_preempt_result",
             "gs_preempt_detail", "gs_preempt_candidate"]
    arr = (C.c_uint64 * len(names))()
    lib.gs_abi_sizes(arr, len(names))
    for name, size in zip(names, arr):
        assert abi.STRUCT_SIZES[name] == size, name
    assert abi.STRUCT_SIZES["gs_preempt_candidate"] == 32 and abi.GS_ABI_VERSION == 6


# ---- the restatement on a one-node cluster (the builders: tests/preempt_edges_util.py) ----
def run(free_cpu, residents, cpu, used, limit, **kw):
    c, o = one_node(free_cpu)
    t = pu.Table(1)
    t.add([0] * len(residents), residents)
    rows = kw.pop("rows", None)
    pre = pu.make_preemptor(pod_of(c, cpu), -1 if rows is None else 0, (used, 0), (limit, 1 << 50), **kw)
    before = fd.codes_of(o, c.pods[:1])
    a = pu.dry_run(o, c.nodes, t, pre, rows)
    assert np.array_equal(before, fd.codes_of(o, c.pods[:1]))   # the oracle's rows were restored
    o.close()
    return a, t


def test_non_prefix_victim_set():
    """A large important pod is evicted, a small less important one reprieved."""
    a, _ = run(0, [resident(1, 8 * CPU, 990), resident(2, 2 * CPU, 980)], 8 * CPU, 0, 1 << 40)
    assert (a.status, a.node, a.victims) == (abi.GS_PREEMPT_NOMINATED, 0, [1])
    assert a.node_status[0] == pu.CANDIDATE and a.victim_bits[0].tolist() == [1, 0] and a.non_prefix == 1


def test_quota_driven_victim_on_a_node_that_fits():
    a, _ = run(8 * CPU, [resident(1, 4 * CPU, 990)], 2 * CPU, 10 * CPU, 11 * CPU)
    assert (a.status, a.victims, a.quota_victims_on_fitting) == (abi.GS_PREEMPT_NOMINATED, [1], 1)


def test_double_removal_is_an_error():
    """The reprieved pod fits neither the node nor the quota: removed twice, the node ends with an Error."""
    a, _ = run(0, [resident(1, 4 * CPU, 990)], 2 * CPU, 10 * CPU, 7 * CPU)
    assert (a.status, a.node, a.num_errors, a.num_candidates) == (abi.GS_PREEMPT_ERROR, -1, 1, 0)
    assert a.node_status[0] == pu.ERROR and not a.victim_bits.any()


def test_no_victims_found():
    a, _ = run(0, [resident(1, 4 * CPU, 1000), resident(2, 4 * CPU, 990, quota=2),
                   resident(3, 4 * CPU, 990, flags=abi.GS_RESIDENT_NON_PREEMPTIBLE)], 2 * CPU, 0, 1 << 40)
    assert (a.status, a.num_potential, a.node_status[0]) == (abi.GS_PREEMPT_NO_CANDIDATES, 1, pu.NO_VICTIMS)


def test_fits_with_none_evicted():
    a, _ = run(8 * CPU, [resident(1, 4 * CPU, 990)], 2 * CPU, 0, 1 << 40)
    assert (a.status, a.node_status[0]) == (abi.GS_PREEMPT_NO_CANDIDATES, pu.FITS)
    a, _ = run(0, [resident(1, 4 * CPU, 990)], 8 * CPU, 0, 1 << 40)     # 4 CPUs freed do not hold 8
    assert (a.status, a.node_status[0]) == (abi.GS_PREEMPT_NO_CANDIDATES, pu.UNFIT)


def test_used_is_floored_at_zero():
    """used 1 CPU, the victim's 4 leave: 0, not -3; back again: 4, and 4 + 2 exceeds 5 (1 + 2 would not)."""
    a, _ = run(8 * CPU, [resident(1, 4 * CPU, 990)], 2 * CPU, 1 * CPU, 5 * CPU)
    assert (a.status, a.victims) == (abi.GS_PREEMPT_NOMINATED, [1])
    a, _ = run(8 * CPU, [resident(1, 4 * CPU, 990, flags=0)], 2 * CPU, 1 * CPU, 5 * CPU)   # untracked: used stays 1
    assert a.node_status[0] == pu.FITS
    a, _ = run(8 * CPU, [resident(1, 4 * CPU, 990, quota=-1)], 2 * CPU, 99 * CPU, 0, quota=-1)   # skip: no quota check
    assert a.node_status[0] == pu.FITS


def test_uid_breaks_the_remaining_tie():
    a, t = run(0, [resident(5, 4 * CPU, 990, start=7), resident(3, 4 * CPU, 990, start=7)], 4 * CPU, 0, 1 << 40)
    assert [int(r["uid"]) for r in t.nodes[0]] == [3, 5]
    assert a.victims == [5] and a.victim_bits[0].tolist() == [2, 0]


def test_eligibility():
    term = resident(1, 4 * CPU, 990, flags=abi.GS_RESIDENT_QUOTA_TRACKED | abi.GS_RESIDENT_TERMINATING)
    a, _ = run(0, [term], 2 * CPU, 0, 1 << 40, flags=abi.GS_PREEMPT_NEVER)
    assert (a.status, a.num_potential) == (abi.GS_PREEMPT_NOT_ELIGIBLE, 0) and not a.node_status.any()
    a, _ = run(0, [term], 2 * CPU, 0, 1 << 40, nominated=0)
    assert a.status == abi.GS_PREEMPT_NOT_ELIGIBLE
    # the nominated node is UnschedulableAndUnresolvable in the pod's row: eligible again, and no potential node
    unres = np.array([[abi.GS_NUMA_INVALID_TOPOLOGY << abi.GS_FAIL_NUMA_SHIFT]], np.uint16)
    a, _ = run(0, [term], 2 * CPU, 0, 1 << 40, nominated=0, rows=unres)
    assert a.status == abi.GS_PREEMPT_NO_POTENTIAL_NODES
    # a terminating pod of another quota, or of no lower priority, does not count
    for other in (resident(1, 4 * CPU, 990, quota=2, flags=abi.GS_RESIDENT_TERMINATING),
                  resident(1, 4 * CPU, 1000, flags=abi.GS_RESIDENT_TERMINATING)):
        a, _ = run(0, [other, resident(2, 4 * CPU, 990)], 2 * CPU, 0, 1 << 40, nominated=0)
        assert a.status == abi.GS_PREEMPT_NOMINATED


# ---- the GPU cases' input conditions ----
def test_row_case_conditions():
    """700 nodes, Fit + LoadAware, rows of the first 3 FitError pods. Status 0 needs an UnschedulableAndUnresolvable
    row entry, which only NodeNUMAResource produces (the NUMA case below); status 4 cannot follow from a truthful row:
    a node that failed the Filter at the pod's turn holds no less afterwards, so with everybody reprieved it fails
    again (the quota case has it)."""
    case = pu.row_case(False)
    ans = case.answers([0, 1, 2])
    seen = set()
    for a in ans:
        seen |= set(np.unique(a.node_status).tolist())
    assert seen == {pu.CANDIDATE, pu.NO_VICTIMS, pu.UNFIT}
    assert max(a.num_candidates for a in ans) >= 20 and max(a.non_prefix for a in ans) >= 5
    assert any(a.decided_at >= 3 for a in ans)
    assert any(a.status == abi.GS_PREEMPT_NO_CANDIDATES for a in ans)   # the 400-CPU pod: no node is enough


def test_numa_case_conditions():
    case = pu.row_case(True)
    ans = case.answers(list(pu.NUMA_PREEMPTORS))
    seen = set()
    for a in ans:
        seen |= set(np.unique(a.node_status).tolist())
    assert seen == {pu.NOT_POTENTIAL, pu.CANDIDATE, pu.NO_VICTIMS, pu.UNFIT}
    assert any(0 < a.num_potential < 700 for a in ans)            # potential nodes != all nodes
    assert max(a.num_candidates for a in ans) >= 20 and max(a.non_prefix for a in ans) >= 5
    assert any(a.amp_flips >= 1 for a in ans)    # a reprieve fails on the amplified-CPU check alone somewhere
    assert (case.c.numa["node_numa"]["cpu_amplification_ratio"] > 1).any()
    assert any(a.decided_at >= 3 for a in ans)


def test_quota_case_conditions():
    case = pu.quota_case()
    ans = case.answers(list(range(len(case.preemptors))))
    rejected = ans[:3]
    assert all(int(p["row"]) == -1 for p in case.preemptors)
    assert max(a.num_errors for a in rejected) >= 5
    assert max(a.quota_victims_on_fitting for a in rejected) >= 20
    assert any(a.decided_at >= 3 for a in rejected)
    assert ans[3].num_candidates == 0 and (ans[3].node_status == pu.NO_VICTIMS).all()      # skip: nobody shares "no quota"
    assert ans[4].status == abi.GS_PREEMPT_NOT_ELIGIBLE
    seen = set(np.unique(ans[5].node_status).tolist())
    assert seen >= {pu.CANDIDATE, pu.NO_VICTIMS, pu.UNFIT, pu.FITS}
    assert int(case.preemptors[6]["nominated_node"]) >= 0 and ans[6].status == abi.GS_PREEMPT_NOT_ELIGIBLE


def test_boundary_case_conditions():
    case = pu.boundary_case()
    a, = case.answers([0])
    counts = np.bincount(case.node_idx, minlength=257)
    assert set(counts.tolist()) == {0, 1, 2, 63, 64, 65, 128}
    assert a.num_candidates >= 20 and (a.victim_bits[:, 1] != 0).any() and (a.victim_bits[:, 0] != 0).any()
    assert a.node_status[256] != pu.NOT_POTENTIAL
