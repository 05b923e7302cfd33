"""gs_preempt_dry_run and gs_preempt_dry_run_pdb on the GPU at the edges of tests/preempt_edges_util.py (the inputs'
conditions are asserted on the truth alone in tests/test_preempt_edges.py). Every case goes through both calls and
through preempt_util.check / preempt_pdb_util.check (node status, victim bits, the result struct, the host pick over
the detail arrays), and through the "modified nothing" checks of tests/test_gpu_preempt.py: mirror_check() == 0 and
the preemptors' evaluate codes unchanged."""
import numpy as np
import pytest

from koordinator_amd import abi, synth
from tests import fit_diag_util as fd
from tests import preempt_edges_util as pe
from tests import preempt_util as pu
from tests import test_gpu_preempt as old
from tests import test_gpu_preempt_pdb as oldp

pytestmark = pytest.mark.gpu


def engine_of(ec: pe.EdgeCase):
    """The engine in the case's state, the residents' PDB lists and the budget registered"""
    e, rows = old.engine(ec.base)
    oldp.set_lists(e, ec.pdb)
    oldp.set_budgets(e, ec.pdb)
    return e, rows


def run_both(e, ec: pe.EdgeCase, ks, rows):
    """Preemptors ks through both calls against both truths -> (the old call's outputs, the PDB call's)"""
    ks = list(ks)
    plain = old.run_and_check(e, ec.base, ks, rows, ec.base.table())
    pdb = oldp.run_and_check(e, ec.pdb, ks, rows)
    for j, k in enumerate(ks):      # what the scenario was built for, on the device's answer
        x = ec.expect[k]
        if "node" in x:
            assert int(plain[0][j]["node"]) == x["node"] and int(pdb[0][j]["node"]) == x.get("pdb_node", x["node"])
        for node, st in x.get("status", {}).items():
            assert plain[1][j][node] == st and pdb[1][j][node] == st, (ec.names[k], node)
    return plain, pdb


# ---- 1. pick positions x criteria at N = 65,793: one engine, the configurations switched in and out ----
@pytest.fixture(scope="module")
def pick_engine():
    from koordinator_amd.engine import Engine
    ps = pe.pick_section()
    e = Engine(fd.make_cfg(ps.c, False))
    synth.load_into(e, ps.c)
    oldp.set_budgets(e, ps.batches[0].pdb)
    yield e
    e.close()


@pytest.mark.parametrize("b", range(pe.PICK_BATCHES))
def test_pick_positions_and_criteria(pick_engine, b):
    """258 parts per preemptor, the second stride of the pick kernel; the winner and the runner-up in different lanes,
    waves, workgroups and strides; each criterion deciding alone against all later ones; then Error everywhere and no
    candidate at all (the last batch)."""
    e, ps = pick_engine, pe.pick_section()
    ec = ps.batches[b]
    base = ec.base
    e.node_pods_add(base.node_idx, base.residents)
    try:
        oldp.set_lists(e, ec.pdb)
        ks = range(len(ec.names))
        (res, status, _), (res_pdb, _, _, _, nviol) = run_both(e, ec, ks, None)
        for k in ks:
            cf = ps.config_of(b, k)
            assert int(res[k]["num_potential"]) == int(res_pdb[k]["num_potential"]) == pe.PICK_N
            if cf.crit:
                assert int(res_pdb[k]["node"]) == cf.winner and (status[k] == pu.CANDIDATE).sum() == len(cf.present)
                if cf.crit > 1:
                    assert int(res[k]["node"]) == cf.winner and int(res_pdb[k]["num_pdb_violations"]) == 1
            elif cf.name == "error":
                assert (int(res[k]["status"]), int(res[k]["num_errors"])) == (abi.GS_PREEMPT_ERROR, len(pe.ANCHORS))
                assert (int(res_pdb[k]["status"]), int(res_pdb[k]["num_errors"])) == (abi.GS_PREEMPT_ERROR, len(pe.ANCHORS))
            else:
                assert int(res[k]["status"]) == int(res_pdb[k]["status"]) == abi.GS_PREEMPT_NO_CANDIDATES
    finally:
        e.node_pods_remove(base.node_idx, base.residents["uid"])


# ---- 2. the pick across the two launches ----
def test_pick_across_the_two_launches():
    """A policy node (second launch, its part behind every non-policy part) and a non-policy node tied through
    criterion 5, the policy node at the lower index and at the higher: the lower index wins both times."""
    ec = pe.numa_case()
    e, rows = engine_of(ec)
    (res, status, _), _ = run_both(e, ec, range(2), rows)
    policy = ec.base.c.numa["node_numa"]["numa_topology_policy"] != abi.GS_NUMA_POLICY_NONE
    assert [bool(policy[int(r["node"])]) for r in res] == [True, False]
    for k in range(2):
        assert (status[k][policy] == pu.CANDIDATE).sum() == 1 and (status[k][~policy] == pu.CANDIDATE).sum() == 1
    e.close()


# ---- 3..5. key values, resource slots, quota dimensions at N = 257: one engine per case, one preemptor per test ----
@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(name):
        if name not in made:
            ec = getattr(pe, name)()
            made[name] = (ec,) + engine_of(ec)
        return made[name]
    yield get
    for _, e, _ in made.values():
        e.close()


@pytest.mark.parametrize("name", pe.key_case().names)
def test_key_values(engines, name):
    """64-bit key fields that differ in one half, priorities at the ends of int32, 128 victims, a lone victim at
    position 63, 64, 127 (in the PDB call once as the lone violating victim)."""
    ec, e, rows = engines("key_case")
    k = ec.k(name)
    (res, _, bits), (res_pdb, _, _, viol, nviol) = run_both(e, ec, [k], rows)
    x = ec.expect[k]
    for node, w in x.get("bits", {}).items():
        assert bits[0][node].tolist() == w
    for node, n in x.get("nviol", {}).items():
        assert int(nviol[0][node]) == n and (viol[0][node].tolist() == x["bits"][node] if n else not viol[0][node].any())
    if name == "128-victims":
        assert int(res[0]["num_victims"]) == int(res_pdb[0]["num_victims"]) == 128 and (res[0]["victims"] != 0).all()


@pytest.mark.parametrize("name", pe.slot_case().names)
def test_resource_slots_and_pod_count(engines, name):
    """Slots 2..6 and the pod count as the only binding quantity: candidate, one unit too little, FITS, a reprieve
    that fails by one unit and one that leaves exactly nothing."""
    ec, e, rows = engines("slot_case")
    k = ec.k(name)
    (_, _, bits), _ = run_both(e, ec, [k], rows)
    for node, w in ec.expect[k].get("bits", {}).items():
        assert bits[0][node].tolist() == w


@pytest.mark.parametrize("name", pe.quota_case().names)
def test_quota_dimensions_and_masks(engines, name):
    """Dimensions 2..7 binding, a dimension left out of either mask, a resident's value outside its own mask, the
    floor at zero in dimension 5, a preemptor without a quota, Error through dimension 4."""
    ec, e, rows = engines("quota_case")
    run_both(e, ec, [ec.k(name)], rows)


def test_all_of_a_case_in_one_call(engines):
    """Every preemptor of a case in one call: the same answers wherever a preemptor stands"""
    for case in ("key_case", "slot_case", "quota_case"):
        ec, e, rows = engines(case)
        run_both(e, ec, range(len(ec.names)), rows)


# ---- 6. rows ----
@pytest.fixture(scope="module")
def rows_engine():
    ec = pe.rows_case()
    e, rows = engine_of(ec)
    yield ec, e, rows
    e.close()


def test_row_word_classes(rows_engine):
    """Status 0 exactly where gs_status_framework_code says UnschedulableAndUnresolvable; every other class node is a
    candidate."""
    ec, e, rows = rows_engine
    k = ec.k("row-5-a")
    (res, status, _), _ = run_both(e, ec, [k], rows)
    words = pe.class_words()
    unres = np.array([abi.status_framework_code(w) == 2 for w in words])
    at = np.arange(pe.CLASS_AT, pe.CLASS_AT + len(words))
    assert (status[0][at[unres]] == pu.NOT_POTENTIAL).all() and (status[0][at[~unres]] == pu.CANDIDATE).all()
    assert int(res[0]["num_potential"]) == 257 - int(unres.sum())


@pytest.mark.parametrize("name,want", [("nominated-unresolvable", abi.GS_PREEMPT_NOMINATED),
                                       ("nominated-resolvable", abi.GS_PREEMPT_NOT_ELIGIBLE),
                                       ("all-unresolvable", abi.GS_PREEMPT_NO_POTENTIAL_NODES)])
def test_row_eligibility_and_no_potential_node(rows_engine, name, want):
    ec, e, rows = rows_engine
    (res, status, _), (res_pdb, _, _, _, _) = run_both(e, ec, [ec.k(name)], rows)
    assert int(res[0]["status"]) == int(res_pdb[0]["status"]) == want
    if want != abi.GS_PREEMPT_NOMINATED:
        assert not status[0].any()


def test_rows_named_out_of_order(rows_engine):
    """Seven rows handed in, four preemptors naming rows 5, 2, 5 and -1: each answer is the preemptor's answer when
    called alone with its row."""
    ec, e, rows = rows_engine
    ks = [ec.k(n) for n in pe.ROW_KS]
    plain, pdb = run_both(e, ec, ks, rows)
    for j, k in enumerate(ks):
        p, r = pe.alone(ec, k)
        for got, one in ((plain, e.preempt_dry_run(p, r)), (pdb, e.preempt_dry_run_pdb(p, r))):
            for x, y in zip(got, one):
                assert x[j].tobytes() == y[0].tobytes(), (pe.ROW_KS[j],)
