"""The speculative commit (commit_spec_kernel, gs_commit_spec.hip) at its rollback, tie-window and slot edges, against
the oracle's sequential scheduleOne. Needs an MI355X: -m gpu.

The inputs come from tests/commit_edges_util.py (each builder's docstring names the code it is aimed at);
tests/test_commit_edges.py shows from the oracle alone that every named pod reaches its edge. Here every case must equal
the oracle on node, score, ties and feasible (and, where pods have a Reserve record, on the Reserve flags and the
allocation bytes, under verify_cpusets), leave the HBM mirror equal to the host's, cut the batches the classifier predicts
and resolve from the whole row the pods it predicts. Everything is bit-exact.

* blocking, one call, at the batch size the claims are made for;
* the chain, slot and path cases at batch sizes 31, 32, 33, 64 and 128 (31 / 32: launch_commit_spec's switch between the
  single-selector and the split pipeline), blocking and with three submissions in flight;
* on two ranks over the callback transport, under both exchanges (GS_XCHG=levels: the non-split kernel, winners on the
  other rank's shard enter as SO_UNKNOWN / SO_UNLISTED rows);
* per family once more in the GS_COMMIT_STAMPS=1 build, whose counters (Engine.commit_counters) show that the paths ran:
  same placements, and lower bounds of "at least once" on the counters the family is aimed at. How often a row is still
  pending when the next pod is decided is a matter of timing; the observed counts are in DESIGN.md §6.
"""
import threading
import time

import numpy as np
import pytest

from koordinator_amd import abi
from tests import commit_edges_util as ce

pytestmark = pytest.mark.gpu
CASES = dict(ce.all_cases())
RESERVE_MASK = abi.GS_PLACED_NUMA | abi.GS_PLACED_CPUSET | (0xF << abi.GS_PLACED_AFFINITY_SHIFT)
T_FILE = [0.0]


@pytest.fixture(autouse=True)
def _test_time():
    t0 = time.perf_counter()
    yield
    T_FILE[0] += time.perf_counter() - t0


@pytest.fixture(autouse=True, scope="module")
def _file_time():
    yield
    print(f"\ntest_gpu_commit_edges.py: {T_FILE[0]:.1f} s in its tests")


def _same(case, got, allocation=None, who=""):
    want = case.want[:len(got)]
    for f in ce.FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{who}{case.name}: {f} differs first at pod {bad[0]}: gpu {got[bad[0]]} oracle {want[bad[0]]}"
    if case.want_alloc is None:
        return
    assert np.array_equal(got["flags"] & RESERVE_MASK, want["flags"] & RESERVE_MASK), \
        f"{who}{case.name}: Reserve flags differ at pods {np.nonzero((got['flags'] ^ want['flags']) & RESERVE_MASK)[0][:8]}"
    for j, wa in case.want_alloc.items():
        if j >= len(got):
            continue
        a = allocation(int(got["node"][j]), int(case.pods["uid"][j]))
        assert (a is None) == (wa is None) and (a is None or a.tobytes() == wa), \
            f"{who}{case.name}: pod {j} on node {got['node'][j]}: allocation differs from the oracle's"


def _engine(case, batch=None):
    from koordinator_amd.engine import Engine
    e = Engine(case.config(device=0, batch_size=batch or case.batch))
    case.load(e)
    if case.numa:
        e.verify_cpusets(True)
    e.reset_stats()
    return e


def _submit_three(e, pods, seq, chunk):
    hs, outs = [], []
    for lo in range(0, len(pods), chunk):
        hs.append(e.schedule_submit(pods[lo:lo + chunk], seq[lo:lo + chunk]))
        if len(hs) == 3:
            outs.append(e.schedule_wait(hs.pop(0)))
    outs += [e.schedule_wait(h) for h in hs]
    return np.concatenate(outs)


def _run(case, batch=None, chunk=None):
    """one engine, the case's pods blocking in one call (or in submissions of `chunk`, three in flight) -> stats"""
    e = _engine(case, batch)
    try:
        got = e.schedule(case.pods, case.seq) if chunk is None else _submit_three(e, case.pods, case.seq, chunk)
        _same(case, got, e.allocation)
        assert e.mirror_check() == 0, f"{case.name}: HBM mirror diverged from the host mirror"
        st = e.stats()
        cc = e.commit_counters() if _stamps_on() else None
    finally:
        e.close()
    print(f"{case.name} batch {batch or case.batch}: cuts {st['cuts']}, slowpath_pods {st['slowpath_pods']}, batches {st['batches']}")
    return st, cc


def _stamps_on():
    import os
    return os.environ.get("GS_COMMIT_STAMPS") == "1"


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(name):
    case = CASES[name]()
    st, _ = _run(case)
    assert st["cuts"] == ce.predicted_cuts(case), st
    if len(case.pods) <= case.batch:   # (the classifier's level rule is a call's first batch's)
        assert st["slowpath_pods"] == (case.slowpath or 0), st


@pytest.mark.parametrize("batch", [3, 5, 32])
@pytest.mark.parametrize("name", ["hostcut", "undo-cpuset", "undo-split", "rising-listed", "late"])
def test_reserve_records_at_other_batch_sizes(name, batch):
    """the cpuset / zone-split cases on the single selector with its verify wave (batches under 32 pods: a host cut
    ends the batch through s_vcut) and at the split pipeline's smallest batch; batches of 3 make host pod 2 its batch's
    last pod (no cut for it)"""
    case = CASES[name]()
    st, _ = _run(case, batch)
    assert st["cuts"] == ce.predicted_cuts(case, batch), st


BOUNDARY_CASES = ("chains-long", "chains-short", "slots", "paths-130", "ge")


@pytest.mark.parametrize("batch", [31, 32, 33, 64, 128])
@pytest.mark.parametrize("name", BOUNDARY_CASES)
def test_batch_boundaries_blocking(name, batch):
    """chains that span a boundary: one slab row for several landings, the next batch's fix-up of its stale levels"""
    case = CASES[name]()
    st, _ = _run(case, batch)
    assert st["cuts"] == 0 and st["batches"] >= -(-len(case.pods) // batch), st


@pytest.mark.parametrize("batch", [31, 32, 33, 64, 128])
@pytest.mark.parametrize("name", BOUNDARY_CASES)
def test_batch_boundaries_three_submissions_in_flight(name, batch):
    case = CASES[name]()
    st, _ = _run(case, batch, chunk=batch + 7)
    assert st["cuts"] == 0, st


# ---------------------------------------------------------------------------------------------------------------------
# two ranks on one GPU

def _two_ranks(case):
    from koordinator_amd.engine import Engine
    engines, th, out = [], [], []
    barrier = threading.Barrier(2)
    try:
        for _ in range(2):
            engines.append(Engine(case.config(device=0)))
        for x in engines:
            case.load(x)
        slots = [None, None]

        def make_ag(r):
            def ag(data):
                slots[r] = data
                barrier.wait()
                out = list(slots)
                barrier.wait()
                return out
            return ag

        for r, x in enumerate(engines):
            x.comm_init_callback(2, r, make_ag(r))
            x.reset_stats()
        res = [None, None]

        def run(r):
            res[r] = engines[r].schedule(case.pods, case.seq)

        th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th), f"{case.name}: a rank did not finish"
        for r in range(2):
            assert res[r] is not None, f"{case.name}: rank {r} failed"
            _same(case, res[r], engines[r].allocation, f"rank {r} ")
            assert engines[r].mirror_check() == 0, f"{case.name} rank {r}: HBM mirror diverged"
            st = engines[r].stats()
            print(f"{case.name} rank {r}: cuts {st['cuts']}, slowpath_pods {st['slowpath_pods']}, batches {st['batches']}")
            # no case here has a pod the classifier resolves from its whole row (which the level exchange leaves to the
            # host: a rank has no score rows of the other shard)
            assert st["cuts"] == 0 and st["slowpath_pods"] == 0, f"{case.name} rank {r}: {st}"
            out.append(engines[r].commit_counters() if _stamps_on() else None)
    finally:
        # a rank still inside gs_schedule (its peer failed): release it from the all-gather before its engine goes
        if any(t.is_alive() for t in th):
            barrier.abort()
            for t in th:
                t.join(timeout=30)
        for r, x in enumerate(engines):
            if r >= len(th) or not th[r].is_alive():
                x.close()
    return out


@pytest.mark.parametrize("name", ["chains-short", "chains-long", "chains-low-shard", "alternating-AABB", "ge", "slots",
                                  "paths-130", "excl"])
@pytest.mark.parametrize("xchg", ["rows", "levels"])
def test_two_ranks_on_one_gpu_callback_transport(name, xchg, monkeypatch):
    """Each rank owns half of the nodes. Under the score-row exchange (the default) every rank holds whole rows and its
    commit runs as on one shard; under GS_XCHG=levels the ranks exchange candidate levels and the commit is the
    non-split kernel at every batch size, with winners on the other rank's shard as SO_UNKNOWN / SO_UNLISTED rows. For
    the second rank every anchor of chains-low-shard lies on the other rank's shard, the other cases' anchors lie on
    both; paths-130 crosses nold 61 -> 62 on the single selector."""
    monkeypatch.setenv("GS_XCHG", xchg)
    _two_ranks(CASES[name]())


# ---------------------------------------------------------------------------------------------------------------------
# proof that the paths ran: the GS_COMMIT_STAMPS=1 build's counters

# family -> (cases, batch (None: the case's), counters that must be >= 1)
FAMILIES = {
    "chains": (("chains-short", "chains-long", "alternating-ABAB", "alternating-AABB"), None,
               ("rollbacks", "rollback_depth", "split_late_landings")),
    "ge": (("ge", ), None, ("rollbacks", "split_late_landings", "split_excluded_ties")),
    "ge-single-selector": (("ge", ), 20, ("rollbacks", "pending_ge", "pending_ge_rollbacks", "est_prev_eq")),
    "slots": (("slots", ), None, ("rollbacks", "prep_general_path")),
    "paths": (("paths-130", "paths-300", "paths-2048"), None,
              ("prep_old_path", "prep_general_path", "prep_list_beyond_32", "prep_list_beyond_64", "split_late_landings")),
    # (batches of 31 never see nold > 30: the old-nodes path only; 61 -> 62 on the single selector is the two-rank test below)
    "paths-single-selector": (("paths-130", "paths-300"), 31, ("old_path", "list_beyond_32", "list_beyond_64")),
    "excl": (("excl", ), None, ("split_late_landings", "split_excluded_ties", "split_rerecords")),
    "feasibility": (("fiterror", "pending-only"), None, ("rollbacks", )),
    # (the split pipeline resolves from the whole row over the exact state only: no rollback comes of it)
    "hash": (("hash", ), None, ("full_row", "split_rerecords")),
    "hash-single-selector": (("hash-31", ), None, ("full_row", "rollbacks")),
    # (the fillers chain on one node and roll back on their own: these bounds do not show that the mis-speculated
    # cpuset / split Reserve or the cut was the one undone; that is held by the placements and the allocation bytes)
    "undo": (("undo-cpuset", "undo-split"), None, ("rollbacks", "restored_rows")),
    # (the closing pods find A's row ready again, a new row above every listed level: the general path; a row that is
    # still pending after d >= 2 decisions is caught by apply_late's settled-early check, not by a rollback)
    "late": (("late", ), None, ("prep_general_path", "split_settled_early")),
    # (the single selector has no settled-early check: the in-between pods are decided with background rows pending at M)
    "late-single-selector": (("late", ), 31, ("general_path", "pending_ge")),
    "rising-listed": (("rising-listed", ), None, ("prep_general_path", )),
    "hostcut": (("hostcut", ), None, ("rollbacks", )),
    "rising": (("rising", ), None, ("rollbacks", "prep_general_path")),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_counters_show_the_paths_ran(family, monkeypatch):
    """the stamps build (a second instantiation of the same kernel template): the same placements, and the counters"""
    monkeypatch.setenv("GS_COMMIT_STAMPS", "1")
    names, batch, need = FAMILIES[family]
    total = dict.fromkeys(abi.COMMIT_COUNTER_KEYS, 0)
    for name in names:
        _, cc = _run(CASES[name](), batch)
        print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in cc.items() if v))
        for k, v in cc.items():
            total[k] += v
    print(f"family {family}: " + ", ".join(f"{k} {v}" for k, v in total.items() if v))
    assert total["decisions"] >= sum(len(CASES[n]().pods) for n in names)
    for k in need:
        assert total[k] >= 1, f"{family}: counter {k} stayed 0: the inputs did not reach the path ({total})"


def test_single_selector_general_path_beyond_61_old_rows(monkeypatch):
    """nold 61 -> 62 on the single selector: two ranks under the level exchange (every batch runs the non-split
    kernel), paths-130-step, in
    which no row is ever new (nnew = 0 for every pod), so a general-path decision can only come from nold > 61"""
    monkeypatch.setenv("GS_COMMIT_STAMPS", "1")
    monkeypatch.setenv("GS_XCHG", "levels")
    for r, cc in enumerate(_two_ranks(CASES["paths-130-step"]())):
        print(f"rank {r}: " + ", ".join(f"{k} {v}" for k, v in cc.items() if v))
        assert cc["split_batches"] == 0 and cc["single_batches"] >= 1
        assert cc["old_path"] >= 1 and cc["general_path"] >= 1, cc


def test_counters_refused_without_the_stamps_build(monkeypatch):
    from koordinator_amd.engine import GpuScoreError
    monkeypatch.delenv("GS_COMMIT_STAMPS", raising=False)
    e = _engine(CASES["fiterror"]())
    try:
        with pytest.raises(GpuScoreError):
            e.commit_counters()
    finally:
        e.close()
