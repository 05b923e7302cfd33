"""PodDisruptionBudgets in the preemption dry run, without a GPU: the counting rule the kernel uses against the literal
counter decrement, gs_preempt_pick_node_pdb against the restated six-criterion pick, the new structs' sizes, and the
input conditions (a)-(j) of the GPU cases (tests/test_gpu_preempt_pdb.py), asserted on the truth alone
(tests/preempt_pdb_util.py) so that no GPU test passes vacuously."""
import ctypes as C

import numpy as np
import pytest

from koordinator_amd import abi, build
from tests import preempt_pdb_util as pp
from tests import preempt_util as pu


@pytest.fixture(scope="module")
def lib():
    build.build()
    return abi.load()


def popcount(words) -> int:
    return sum(bin(int(w)).count("1") for w in words)


# ---- the partition ----
def test_counting_rule_equals_the_literal_decrement():
    """1,000 random lists of <= 128 pods, 0-4 memberships each, budgets in -1..5 (and PDBs that do not exist)."""
    s = np.random.RandomState(7)
    violating = 0
    for _ in range(1000):
        n = int(s.randint(0, 129))
        npdb = int(s.randint(1, 9))
        budgets = {p: int(s.randint(-1, 6)) for p in range(npdb) if s.randint(0, 8)}
        lists = [tuple(s.permutation(npdb)[:min(npdb, int(s.randint(0, 5)))].tolist()) for _ in range(n)]
        want = pp.partition_literal(lists, budgets)
        assert pp.partition_counting(lists, budgets) == want
        violating += sum(want)
    assert violating > 10_000


# ---- gs_preempt_pick_node_pdb ----
BASE = (7, 1, 990, 3 * ((1 << 31) + 990), 3, 1_000)   # node, violations, first priority, priority sum, victims, earliest


def vary(field: int, value):
    c = list(BASE)
    c[0] = 9
    c[field] = value
    return tuple(c)


@pytest.mark.parametrize("crit,other,better", [
    (1, vary(1, 0), True),                           # fewer PDB violations win
    (2, vary(2, 989), True),                         # then a lower first priority
    (3, vary(3, BASE[3] - 1), True),                 # then the smaller priority sum
    (4, vary(4, 2), True),                           # then fewer victims
    (5, vary(5, 2_000), True),                       # then the LATEST earliest start
    (6, vary(0, 3), True),                           # then the lower node index
    (1, vary(1, 2), False), (2, vary(2, 991), False), (3, vary(3, BASE[3] + 1), False), (4, vary(4, 4), False),
    (5, vary(5, 500), False), (6, vary(0, 9), False),
])
def test_pick_each_criterion_alone(lib, crit, other, better):
    for cands in ([BASE, other], [other, BASE]):
        want = cands.index(other if better else BASE)
        k, decided, _ = pp.pick(cands)
        assert (k, decided) == (want, crit)
        assert abi.preempt_pick_node_pdb(pp.candidate_array(cands)) == want


def test_pick_violations_dominate(lib):
    a = (1, 0, 999, 10**12, 9, 0)          # no violation, worse in every later criterion
    b = (0, 1, 900, 1, 1, 10**12)
    assert pp.pick([b, a])[:2] == (1, 1) and abi.preempt_pick_node_pdb(pp.candidate_array([b, a])) == 1
    assert abi.preempt_pick_node_pdb(pp.candidate_array([])) == -1 and pp.pick([]) == (-1, 0, [])


def test_pick_random_sets_with_heavy_ties(lib):
    s = np.random.RandomState(5)
    decided = set()
    for _ in range(1000):
        n = int(s.randint(1, 40))
        nodes = s.permutation(200)[:n]
        cands = [(int(nodes[i]), int(s.randint(0, 2)), 990 + int(s.randint(0, 2)), 5 * (1 << 31) + int(s.randint(0, 3)),
                  2 + int(s.randint(0, 2)), int(s.randint(0, 3))) for i in range(n)]
        k, crit, _ = pp.pick(cands)
        decided.add(crit)
        assert abi.preempt_pick_node_pdb(pp.candidate_array(cands)) == k
    assert decided >= {1, 2, 3, 4, 5, 6}


def test_degenerate_keys_agree_with_the_old_pick(lib):
    """No violations and `first` = the highest priority: the order of gs_preempt_pick_node."""
    s = np.random.RandomState(9)
    for _ in range(300):
        n = int(s.randint(1, 30))
        nodes = s.permutation(100)[:n]
        old = [(int(nodes[i]), 990 + int(s.randint(0, 2)), 5 * (1 << 31) + int(s.randint(0, 3)), 2 + int(s.randint(0, 2)),
                int(s.randint(0, 3))) for i in range(n)]
        new = [(c[0], 0) + c[1:] for c in old]
        assert abi.preempt_pick_node_pdb(pp.candidate_array(new)) == abi.preempt_pick_node(pu.candidate_array(old))


def test_first_is_the_first_victim_and_earliest_walks_all(lib):
    """A violating low-priority victim stands first: criterion 2 reads it, criterion 5 the top-priority victims."""
    def victims(*ps):
        v = np.zeros(len(ps), abi.RESIDENT_POD_DTYPE)
        for r, (prio, start) in zip(v, ps):
            r["priority"], r["start_time_ns"] = prio, start
        return v
    a = pp.key_of(0, 1, victims((980, 5), (990, 500), (990, 300)))
    b = pp.key_of(1, 1, victims((980, 9), (990, 400), (990, 350)))
    assert (a[2], a[5], b[5]) == (980, 300, 350)
    assert pp.pick([a, b])[:2] == (1, 5) and abi.preempt_pick_node_pdb(pp.candidate_array([a, b])) == 1
    c = pp.key_of(2, 1, victims((979, 1), (995, 2)))
    assert pp.pick([a, c])[:2] == (1, 2) and abi.preempt_pick_node_pdb(pp.candidate_array([a, c])) == 1


def test_struct_sizes(lib):
    names = ["gs_pod", "gs_node", "gs_node_metric", "gs_pod_metric", "gs_config", "gs_placement", "gs_stats",
             "gs_loadaware_args", "gs_cpu_topology", "gs_node_numa", "gs_pod_allocation", "gs_numa_args",
             "gs_quota_group", "gs_quota_status", "gs_node_devices", "gs_reservation", "gs_pod_ext", "gs_ext_args",
             "gs_ext_placement", "gs_status_map", "gs_resident_pod", "gs_preemptor", "gs_preempt_result",
             "gs_preempt_detail", "gs_preempt_candidate", "gs_preempt_result_pdb", "gs_preempt_detail_pdb",
             "gs_preempt_candidate_pdb"]
    arr = (C.c_uint64 * len(names))()
    lib.gs_abi_sizes(arr, len(names))
    for name, size in zip(names, arr):
        assert abi.STRUCT_SIZES[name] == size, name
    assert (abi.STRUCT_SIZES["gs_preempt_result_pdb"], abi.STRUCT_SIZES["gs_preempt_detail_pdb"],
            abi.STRUCT_SIZES["gs_preempt_candidate_pdb"]) == (32 + 8 * 128, 32, 32)
    assert abi.GS_ABI_VERSION == 6 and (abi.GS_MAX_PDBS, abi.GS_MAX_POD_PDBS, abi.GS_PDB_NONE) == (65535, 4, 0xFFFF)


# ---- the GPU cases' input conditions ----
def candidates(a):
    return np.nonzero(a.node_status == pp.CANDIDATE)[0].tolist()


def both_groups(a):
    return [i for i in candidates(a) if 0 < len(a.partitions[i][1]) < len(a.partitions[i][0])]


def memberships_and_budgets(case):
    n = (case.pdb_ids != pp.NONE).sum(axis=1)
    listed = set(case.pdb_ids[case.pdb_ids != pp.NONE].tolist())
    return set(n.tolist()), listed, set(case.budget_allowed.tolist()), listed - set(case.budget_ids.tolist())


def test_row_case_conditions():
    """(a)-(d), (i) on row_case(False) with the preemptors of the three-preemptor call and ROW_EARLIEST, which the
    128-preemptor call reaches. (d): ROW_FIRST's pick is decided by criterion 2 and ROW_EARLIEST's by criterion 5, each
    with first-below-top candidates alive at the deciding step, and each nominated node changes if the kernel's key
    took the non-PDB rule for that field: the GPU comparison of the nominated node sees both rules."""
    case = pp.row_case(False)
    ks = list(pp.ROW_KS) + [pp.ROW_EARLIEST]
    ans, plain = case.answers(ks), case.plain(ks)
    assert max(len(both_groups(a)) for a in ans) >= 5                                           # (a)
    assert max(sum(1 for i in candidates(a) if (a.victim_bits[i] != p.victim_bits[i]).any())
               for a, p in zip(ans, plain)) >= 3                                                # (b), per preemptor
    a, p = ans[ks.index(pp.ROW_C)], plain[ks.index(pp.ROW_C)]
    assert a.decided_at == 1 and a.node != p.node and a.node >= 0 and p.node >= 0               # (c)
    for k, crit, field in ((pp.ROW_FIRST, 2, 0), (pp.ROW_EARLIEST, 5, 1)):                      # (d)
        a = ans[ks.index(k)]
        assert a.first_below_top and a.decided_at == crit
        assert set(a.alive_at_decision) & set(a.first_below_top)
        assert a.node in a.first_below_top
        wrong = pp.mutated_picks(case, k)[field]
        assert wrong >= 0 and wrong != a.node, (k, wrong, a.node)
        assert sorted(c[0] for c in a.cands) == sorted(n for n, v in pp.SHAPED.items() if v[0] == int(case.preemptors[k]["quota"]))
    x, y = ans[0], ans[1]                                                                       # (i)
    assert int(case.preemptors[ks[0]]["priority"]) != int(case.preemptors[ks[1]]["priority"])
    assert any(x.partitions[i][1] != y.partitions[i][1] for i in x.partitions if i in y.partitions and
               x.node_status[i] == y.node_status[i] == pp.CANDIDATE)
    n, listed, allowed, never = memberships_and_budgets(case)
    assert n >= {0, 1, 4} and allowed >= {-1, 0, 1} and never == {9}
    assert max(ks) < 16 <= len(case.preemptors)      # the 128-preemptor call of the GPU test runs preemptors 0..15


def test_numa_case_conditions():
    case = pp.row_case(True)
    ans = case.answers(list(pu.NUMA_PREEMPTORS))
    policy = case.base.c.numa["node_numa"]["numa_topology_policy"] != abi.GS_NUMA_POLICY_NONE
    with_violating = {i for a in ans for i in candidates(a) if a.partitions[i][1]}
    assert any(policy[i] for i in with_violating) and any(not policy[i] for i in with_violating)
    assert any(a.pdb_violations.any() for a in ans)


def test_quota_case_conditions():
    """(e) a violating victim made by the quota check alone; (j) a double removal inside the violating sweep; the skip
    and the not-eligible preemptors."""
    case = pp.quota_case()
    ks = list(range(len(case.preemptors)))
    ans = case.answers(ks)
    assert any(int(a.pdb_violations[i]) < popcount(a.victim_bits[i] & a.violating_bits[i])
               for a in ans[:3] for i in candidates(a))                                         # (e)
    assert max(a.error_in_violating_sweep for a in ans[:3]) >= 1                                # (j)
    assert ans[3].num_candidates == 0 and int(case.preemptors[3]["quota"]) < 0
    assert ans[4].status == ans[6].status == abi.GS_PREEMPT_NOT_ELIGIBLE
    assert any(a.node != p.node for a, p in zip(ans, case.plain(ks)))


def test_boundary_case_conditions():
    """(f) the budget runs out exactly between bits 63 and 64 on candidates with 65 and 128 residents; (g), (h)."""
    case = pp.boundary_case()
    a, = case.answers([0])
    counts = np.bincount(case.base.node_idx, minlength=257)
    table = case.base.table()
    lists = case.lists
    for size in (65, 128):
        hit = [i for i in candidates(a) if counts[i] == size and len(a.partitions[i][0]) == size and
               int(a.violating_bits[i][0]) == 0 and int(a.violating_bits[i][1]) & 1]
        assert hit, size
        i = hit[0]
        assert pp.BOUNDARY_PDB in lists[int(table.nodes[i][63]["uid"])] and pp.BOUNDARY_PDB in lists[int(table.nodes[i][64]["uid"])]
    assert any(counts[i] == 128 and int(a.violating_bits[i][1]) == 2**64 - 1 for i in candidates(a))
    n, listed, allowed, never = memberships_and_budgets(case)
    assert n >= {0, 1, 4} and listed >= {0, 65534} and allowed >= {-1, 0, 1} and never == {9}   # (g), (h)
    assert a.node_status[256] != pu.NOT_POTENTIAL


def test_unreached_budgets_give_the_old_truth():
    """No list, or every budget unlimited: the restatement equals preempt_util.dry_run, victims in the same order."""
    case = pp.quota_case()
    for lists, budgets in (({}, case.budgets), (None, {})):
        for a, p in zip(case.answers([0, 2], lists=lists, budgets=budgets), case.plain([0, 2])):
            assert np.array_equal(a.node_status, p.node_status) and np.array_equal(a.victim_bits, p.victim_bits)
            assert (a.status, a.node, a.victims) == (p.status, p.node, p.victims)
            assert not a.violating_bits.any() and not a.pdb_violations.any() and a.num_pdb_violations == 0
            assert [c[:1] + c[2:] for c in a.cands] == p.cands
