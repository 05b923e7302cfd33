"""gs_schedule_top_scores on the GPU against the CPU oracle: the --debug-scores table of every scored pod is the first
topn of its feasible nodes by (total descending, node ascending) at that pod's turn, with the plugin scores
(tests/top_scores_util.py has the truth). Most tables differ both from the one at their batch's start and from the
one at its end, so an implementation that evaluates before or after the batch, or after the call, fails."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from koordinator_amd import abi, synth
from tests import fit_diag_util as fd
from tests import fit_status_util as fs
from tests import top_scores_util as tu

pytestmark = pytest.mark.gpu


def engine(c, numa=False, cfg=None, **kw):
    from koordinator_amd.engine import Engine
    e = Engine(cfg if cfg is not None else fd.make_cfg(c, numa, **kw))
    synth.load_into(e, c)
    return e


@functools.lru_cache(maxsize=None)
def plain_run(n, p, cid, numa):
    """Plain gs_schedule of a tight case, and the context's stats() after it."""
    c, _ = tu.case(n, p, cid, numa)
    e = engine(c, numa)
    out = e.schedule(c.pods)
    st = e.stats()
    e.close()
    return out, st


def run_case(c, t, topn, numa=False, **kw):
    e = engine(c, numa, **kw)
    got, rows, count = e.schedule_top_scores(c.pods, topn=topn)
    tu.check(got, rows, count, t, topn)
    assert e.mirror_check() == 0
    st = e.stats()
    e.close()
    return got, rows, count, st


@pytest.mark.parametrize("topn", [1, 8, 64])
@pytest.mark.parametrize("batch", [1, 7, 128])
def test_batch_sizes(batch, topn):
    c, t = tu.case(700, 512, 0, False)
    got, _, count, _ = run_case(c, t, topn, batch_size=batch)
    assert (count > 0).sum() >= 350 and (got["node"] < 0).sum() >= 100   # (the oracle alone: 391 and 121)
    if batch == 128:
        tu.same_placements(got, plain_run(700, 512, 0, False)[0])


@pytest.mark.parametrize("topn", [8, 64])
def test_numa(topn):
    c, t = tu.case(700, 256, 3, True)
    policy = c.numa["node_numa"]["numa_topology_policy"] != 0
    assert sum(int(policy[t.table(i, topn)["node"]].sum()) for i in range(256)) >= 100   # rows on policy nodes
    got, rows, _, _ = run_case(c, t, topn, numa=True)
    assert (rows["plugin"][:, :, abi.GS_PLUGIN_NUMA] > 0).any()
    tu.same_placements(got, plain_run(700, 256, 3, True)[0])


def test_padding_tail():
    c, t = tu.case(1500, 640, 0, False)
    run_case(c, t, 8)


@functools.lru_cache(maxsize=None)
def small_case():
    c = fd.tight_cluster(257, 96, 0, False)
    return c, tu.Truth(c, fd.make_cfg(c, False), windows=False)


def test_guard_bytes():
    """257 nodes, topn 64, through the C-ABI with guard records around rows and count: nothing outside is written."""
    from koordinator_amd.engine import lib
    c, t = small_case()
    P, topn, G = len(c.pods), 64, 128
    assert (t.count(topn) > 0).sum() >= 50 and t.short(topn).sum() >= 1
    e = engine(c)
    rows = np.zeros(P * topn + 2 * G, abi.TOP_SCORE_DTYPE)
    rows.view(np.uint8)[:] = 0xA5
    rows[G:G + P * topn].view(np.uint8)[:] = 0
    count = np.full(P + 2 * G, 0xA5A5A5A5, np.uint32)
    out = np.zeros(P, abi.PLACEMENT_DTYPE)
    seq = np.arange(P, dtype=np.uint64)
    ts = abi.GsTopScores(rows=abi.ptr(rows[G:]), count=abi.ptr(count[G:]), topn=topn)
    assert lib().gs_schedule_top_scores(e._h, abi.ptr(c.pods), P, abi.ptr(seq), abi.ptr(out), C.byref(ts)) == 0
    tu.check(out, rows[G:G + P * topn].reshape(P, topn), count[G:G + P], t, topn)
    for guard in (rows[:G], rows[G + P * topn:]):
        assert (guard.view(np.uint8) == 0xA5).all()
    assert (count[:G] == 0xA5A5A5A5).all() and (count[G + P:] == 0xA5A5A5A5).all()
    assert e.mirror_check() == 0
    e.close()


def test_chunked_and_submitted():
    c, t = tu.case(700, 512, 0, False)
    e = engine(c)
    parts = []
    for i in range(0, 512, 128):
        got, rows, count = e.schedule_top_scores(c.pods[i:i + 128], np.arange(i, i + 128, dtype=np.uint64), topn=8)
        tu.check(got, rows, count, t, 8, i, i + 128)
        parts.append((got, rows, count))
    assert e.mirror_check() == 0
    e.close()
    e = engine(c)
    h = [e.schedule_submit_top_scores(c.pods[i:i + 256], np.arange(i, i + 256, dtype=np.uint64), topn=8) for i in (0, 256)]
    sub = [e.schedule_wait(x) for x in h]
    for (got, rows, count), i in zip(sub, (0, 256)):
        tu.check(got, rows, count, t, 8, i, i + 256)
    assert e.mirror_check() == 0
    e.close()
    for f in range(3):
        assert np.array_equal(np.concatenate([p[f] for p in parts]), np.concatenate([s[f] for s in sub]))


@pytest.mark.parametrize("order,topn", [(("top", "nodes", "plain", "diag"), 8), (("diag", "plain", "nodes", "top"), 64)])
def test_report_kinds_back_to_back(order, topn):
    """Four submissions of 128 pods, each with another kind of report, waited for only after the last is submitted: the
    first batch of a run is launched speculatively with that run's reports behind the batch of the run before it, whose
    placements are applied (deferred) to its own run's destinations. Over the two orders every kind is the batch behind
    each other kind and the batch in front of one."""
    c, tt = tu.case(700, 512, 0, False)
    _, td, st = fs.status_case(700, 512, 0, False)
    windows = list(range(0, 512, 128))
    for lo in windows:   # every batch has pods for both landed passes (the oracle alone: 29 / 41 / 27 / 24 pods with no
        w = slice(lo, lo + 128)   # node, 99 / 87 / 101 / 104 scored pods)
        assert (tt.placements["node"][w] < 0).sum() >= 1 and (tt.placements["feasible"][w] >= 2).sum() >= 1
    e = engine(c)
    # a context's first run of a kind allocates its buffers with the worker idle: empty runs do so before the first
    # submission, so that none of the four waits for the one before it
    e.schedule_diag_nodes(c.pods[:0])
    e.schedule_top_scores(c.pods[:0])
    submit = {"top": lambda p, s: e.schedule_submit_top_scores(p, s, topn=topn), "nodes": e.schedule_submit_diag_nodes,
              "plain": e.schedule_submit, "diag": e.schedule_submit_diag}
    h = [submit[k](c.pods[lo:lo + 128], np.arange(lo, lo + 128, dtype=np.uint64)) for k, lo in zip(order, windows)]
    res = [e.schedule_wait(x) for x in h]
    placed = []
    for k, lo, r in zip(order, windows, res):
        hi = lo + 128
        if k == "top":
            got, rows, count = r
            tu.check(got, rows, count, tt, topn, lo, hi)
        elif k == "nodes":
            got, diag, words, row_of = r
            fd.check(got, diag, td, c.num_nodes, lo, hi)
            fs.check_rows(words, row_of, st, lo, hi)
        elif k == "diag":
            got, diag = r
            fd.check(got, diag, td, c.num_nodes, lo, hi)
        else:
            got = r
            for f in ("node", "score", "ties", "feasible"):
                assert np.array_equal(got[f], tt.placements[f][lo:hi]), f
        placed.append(got)
    assert e.mirror_check() == 0
    e.close()
    tu.same_placements(np.concatenate(placed), plain_run(700, 512, 0, False)[0])


@pytest.mark.parametrize("n,p", [(300, 200), (2100, 200)])
def test_homogeneous(n, p):
    """Every node ties: the cut at a tie level and the removal of the landed nodes, across the 64-lane and 256-thread
    boundaries of the compaction (2,100 nodes: past LCAP)."""
    c, t = tu.homogeneous_case(n, p)
    assert t.cut_tie(64).sum() >= p // 2 and (t.placements["ties"] > 64).sum() >= p // 2
    last = max(int(t.table(i, 64)["node"][t.table(i, 64)["total"] == t.table(i, 64)["total"][-1]].max()) for i in range(p))
    assert last >= (64 if n < 1024 else 256)   # a table's cut level reaches past the first wave / first 256 nodes
    for topn in (8, 64):
        run_case(c, t, topn)


def test_one_feasible_node():
    c, t = tu.one_feasible_case()
    k = tu.ONE_FEASIBLE_POD
    assert t.placements["feasible"][k] == 1 and t.placements["node"][k] >= 0
    got, _, count, _ = run_case(c, t, 8)
    assert count[k] == 0 and got["node"][k] >= 0 and count[k - 1] > 0 and count[k + 1] > 0


def test_special_pods_cut_the_batch():
    """Pods the host applies itself (a terminated pod, a uid already in an assign cache, a name a PodMetric carries)
    end the batch before and after them: the tables come from the passes that stand."""
    c0, _ = tu.case(700, 512, 0, False)
    pods = c0.pods[:200].copy()
    pods["flags"][50] |= abi.GS_POD_TERMINATED
    pods["uid"][51] = c0.assigned_pods["uid"][0]
    pods["name_key"][120] = c0.pod_metrics["name_key"][0]
    for k in (50, 51, 120):   # small enough to find nodes on the tight cluster
        pods["requests"][k, 0] = pods["nonzero_requests"][k, 0] = 100
    c = dataclasses.replace(c0, pods=pods)
    t = tu.Truth(c, fd.make_cfg(c, False), windows=False)
    assert all(t.count(8)[k] > 0 for k in (49, 50, 51, 52, 120, 121))
    _, _, _, st = run_case(c, t, 8)
    assert st["batches"] >= 6


def test_weights_and_score_only_profile():
    c, _ = tu.case(700, 512, 0, False)
    c = dataclasses.replace(c, pods=c.pods[:200])
    cfg = fd.make_cfg(c, False, weights=(7, 13, 0))
    t = tu.Truth(c, cfg, windows=False)
    e = engine(c, cfg=cfg)
    got, rows, count = e.schedule_top_scores(c.pods, topn=8)
    tu.check(got, rows, count, t, 8)
    assert e.mirror_check() == 0
    e.close()
    assert (rows["total"][count > 0, 0] > 200).any()   # (beyond what weights of 1 can give two plugins)
    cn = dataclasses.replace(c, pods=c.pods[:128])
    cfg = fd.make_cfg(cn, False)
    cfg.enabled = abi.GS_ENABLE_FIT_SCORE | abi.GS_ENABLE_LA_SCORE
    t = tu.Truth(cn, cfg, windows=False)
    assert (t.count(64) == 64).all()   # no Filter: every node is feasible for every pod
    e = engine(cn, cfg=cfg)
    got, rows, count = e.schedule_top_scores(cn.pods, topn=64)
    tu.check(got, rows, count, t, 64)
    assert e.mirror_check() == 0
    e.close()


def test_refusals():
    from koordinator_amd.engine import Engine, GpuScoreError, LocalGroup, lib
    c, _ = tu.case(700, 512, 0, False)
    cfg = fd.make_cfg(c, False)
    g = LocalGroup(2)
    ranks = [Engine(cfg) for _ in range(2)]
    for r, x in enumerate(ranks):
        synth.load_into(x, c)
        x.comm_init_local(g, r)
    sampled = engine(c, percentage_of_nodes_to_score=50)
    for x in ranks + [sampled]:
        before = x.stats()
        with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EUNSUPPORTED}"):
            x.schedule_top_scores(c.pods[:64])
        with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EUNSUPPORTED}"):
            x.schedule_submit_top_scores(c.pods[:64])
        assert x.stats() == before
        x.close()
    del g
    e = engine(c)
    before = e.stats()
    for topn in (0, 65):
        with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EINVAL}"):
            e.schedule_top_scores(c.pods[:64], topn=topn)
        with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EINVAL}"):
            e.schedule_submit_top_scores(c.pods[:64], topn=topn)
    out = np.zeros(64, abi.PLACEMENT_DTYPE)
    rows, count = np.zeros((64, 8), abi.TOP_SCORE_DTYPE), np.zeros(64, np.uint32)
    for ts in (None, abi.GsTopScores(rows=None, count=abi.ptr(count), topn=8),
               abi.GsTopScores(rows=abi.ptr(rows), count=None, topn=8)):
        arg = C.byref(ts) if ts is not None else None
        assert lib().gs_schedule_top_scores(e._h, abi.ptr(c.pods), 64, None, abi.ptr(out), arg) == abi.GS_EINVAL
    assert e.stats() == before
    e.close()


INT_STATS = ("pods", "batches", "eval_launches", "eval_pairs")


def test_off_means_off():
    """A context that ran only the new call and one that ran only gs_schedule agree on the placements and on the
    batch structure; the plain context holds none of the feature's buffers (its counters are those of the plain path:
    the same batches, eval launches and pairs)."""
    c, t = tu.case(700, 512, 0, False)
    plain, pst = plain_run(700, 512, 0, False)
    got, _, _, tst = run_case(c, t, 8)
    tu.same_placements(plain, got)
    for k in INT_STATS:
        if k in pst:
            assert pst[k] == tst[k], k
    # the parent commit's plain run on this input (three runs alike): the plain path launches what it launched
    assert {k: pst[k] for k in INT_STATS} == {"pods": 512, "batches": 4, "eval_launches": 4, "eval_pairs": 358400}
