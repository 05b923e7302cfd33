"""The candidate-level stage (cand_kernel, the cs_hist / cs_pick / cs_list slice kernels, fix_levels_kernel,
merge_levels_kernel) at its row-length, list-capacity and score-range edges, against the oracle's sequential
scheduleOne on node, score, ties and feasible. Needs an MI355X: -m gpu.

The inputs come from tests/level_edges_util.py; tests/test_level_edges.py shows from the oracle alone that each of them
puts its deciding nodes where it claims."""
import threading
import time

import numpy as np
import pytest

from koordinator_amd import config
from koordinator_amd.engine import Engine, GpuScoreError, LocalGroup
from koordinator_amd import synth
from tests import level_edges_util as lu
from tests.test_gpu_parity import run_ranks_local
from tests.test_gpu_sampling import check as sampling_check, sampling_pair

pytestmark = pytest.mark.gpu


def _engine(c, **kw):
    e = Engine(config.make_config(c.num_nodes, device=0, **kw))
    synth.load_into(e, c)
    return e


def _calls(e, pods, chunk, lo=0):
    """blocking gs_schedule calls of `chunk` pods, sequence numbers lo.."""
    seq = np.arange(lo, lo + len(pods), dtype=np.uint64)
    return np.concatenate([e.schedule(pods[i:i + chunk], seq[i:i + chunk]) for i in range(0, len(pods), chunk)])


def _ranks_same(c, cfg, n, want):
    res, engines, _ = run_ranks_local(c, cfg, n)
    for r in range(n):
        assert not isinstance(res[r], Exception) and res[r] is not None, (r, res[r])
        lu.same(res[r], want)
        assert engines[r].mirror_check() == 0
    return engines


# ---------------------------------------------------------------------------------------------------------------------
# 1. deciding nodes at the ends of rows, steps, wave shares and slices

SHAPES = {"one-call": dict(), "batch8": dict(batch_size=8), "calls-of-31": dict()}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", lu.EDGE_SIZES)
def test_edge_positions_one_rank(n, shape):
    """one-call: one batch through cand_kernel at every size (from 3,585 nodes it has 39 pods or more, beyond the 32 the
    slice kernels take). batch8: every later batch's levels are built beside the previous commit and fixed up after it, the landed
    rows being the edge nodes. calls-of-31: each call's first batch is a short one, built by cand_kernel below 3,585
    nodes and by the slice kernels from there."""
    c, want, _ = lu.edge_cluster(n)
    e = _engine(c, **SHAPES[shape])
    got = _calls(e, c.pods, 31) if shape == "calls-of-31" else e.schedule(c.pods, np.arange(len(c.pods), dtype=np.uint64))
    lu.same(got, want)
    assert e.mirror_check() == 0


@pytest.mark.parametrize("xchg", ["levels", "scores"])
@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("n", lu.SHARDED_EDGE_SIZES)
def test_edge_positions_sharded(n, ranks, xchg, monkeypatch):
    """shards of ceil(n / ranks) rows: their ends fall before, on and after 512-entry steps, and every shard but the
    first lists node ids from a non-zero base"""
    monkeypatch.setenv("GS_XCHG", xchg)
    c, want, _ = lu.edge_cluster(n)
    engines = _ranks_same(c, config.make_config(n), ranks, want)
    for r in range(ranks - 1):
        assert engines[r].stats()["shard_end"] == engines[r + 1].stats()["shard_begin"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. large rows

def test_sliced_rows_second_halves():
    """135,169 nodes in three calls of 6 pods: slices of 4096 entries, so cs_hist_kernel's second load and
    cs_list_kernel's second 2048 entries run, the deciding nodes at their ends; the last slice holds 512 entries and
    the last node. Measured: the oracle's 18 placements 1.4 s on the CPU; loading the engine and the three calls 0.13 s
    on an MI355X (0.5 s for the whole test there)."""
    c, want, _ = lu.sliced_case()
    t0 = time.perf_counter()
    e = _engine(c)
    got = _calls(e, c.pods, 6)
    print(f"sliced rows: engine load + 3 calls {time.perf_counter() - t0:.2f} s")
    lu.same(got, want)
    assert e.mirror_check() == 0


def test_stepcap_rows_steps_without_a_recorded_maximum():
    """262,657 nodes, one call of 34 pods at batch_size 64 (more than 32 pods: cand_kernel): each of the first three
    waves takes 129 steps, the last one past the 128 recorded per-step maxima (pass 2 reads it unconditionally), with
    deciding nodes at both ends of it. Measured: the oracle's 34 placements 3.7 s on the CPU; loading the engine and the
    call 0.20 s on an MI355X (1.1 s for the whole test there)."""
    c, want, _ = lu.stepcap_case()
    t0 = time.perf_counter()
    e = _engine(c, batch_size=64)
    got = e.schedule(c.pods, np.arange(len(c.pods), dtype=np.uint64))
    print(f"stepcap rows: engine load + 1 call {time.perf_counter() - t0:.2f} s")
    lu.same(got, want)
    assert e.mirror_check() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. a top level at the list capacity

@pytest.mark.parametrize("n", lu.CAPACITY_SIZES)
def test_top_level_at_list_capacity_one_rank(n):
    """One level of 2047 / 2048 / 2049 identical nodes against LCAP = 2048 (listed iff cb + c <= lcap). At 2049 no level
    is listed and the pods are resolved from their whole rows. Below, the slow path is not excluded by the code (a pod
    whose listed nodes are all dirtied takes it), so its count is printed, not asserted: observed 0 at 2047 and 2048, and
    40 (every pod) at 2049."""
    c, want = lu.capacity_case(n)
    e = _engine(c)
    lu.same(e.schedule(c.pods, np.arange(len(c.pods), dtype=np.uint64)), want)
    assert e.mirror_check() == 0
    st = e.stats()
    print(f"capacity {n}: slowpath_pods {st['slowpath_pods']} cuts {st['cuts']}")
    if n > 2048:
        assert st["slowpath_pods"] > 0


@pytest.mark.parametrize("n", lu.SHARD_CAPACITY_SIZES)
def test_top_level_at_exchange_capacity_two_ranks(n, monkeypatch):
    """256 and 257 identical nodes per shard against XCAP = 256 under GS_XCHG=levels; at 257 the host resolves the pods
    (as in test_homogeneous_cluster_two_ranks_host_slow_path: the batch is cut and the pod resolved from the rows).
    Observed per rank: slowpath_pods 0, cuts 0 at 256 per shard; 2 and 2 at 257 (a shard's top level passes 256 only until
    a pod has landed on one of its nodes)."""
    monkeypatch.setenv("GS_XCHG", "levels")
    c, want = lu.capacity_case(n)
    engines = _ranks_same(c, config.make_config(n), 2, want)
    for r, x in enumerate(engines):
        st = x.stats()
        print(f"shard capacity {n} rank {r}: slowpath_pods {st['slowpath_pods']} cuts {st['cuts']}")
        if n > 512:
            assert st["slowpath_pods"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. score range: one bin to the admitted maximum

@pytest.mark.parametrize("weights", lu.WEIGHTS + lu.NUMA_WEIGHTS, ids=str)
def test_score_range_three_batches(weights):
    """300 pods in one call: batches of 128, 128 and 44, the later ones' levels built beside the previous commit and
    fixed up (histograms of max_score + 1 bins, the level pick's 64-bin strides over mostly empty bins)"""
    c, want = lu.range_case(weights)
    e = _engine(c, weights=weights, enabled=lu.enabled_of(weights))
    lu.same(e.schedule(c.pods, np.arange(len(c.pods), dtype=np.uint64)), want)
    assert e.mirror_check() == 0
    assert e.stats()["batches"] >= 3


@pytest.mark.parametrize("weights", lu.WEIGHTS + lu.NUMA_WEIGHTS[:1], ids=str)
def test_score_range_sliced_rows(weights):
    """calls of 31 pods over 4,500 nodes: the slice kernels with up to 2,001 bins"""
    c, want = lu.range_case(weights, 4500, 93)
    e = _engine(c, weights=weights, enabled=lu.enabled_of(weights))
    lu.same(_calls(e, c.pods, 31), want)
    assert e.mirror_check() == 0


@pytest.mark.parametrize("ranks", [2, 4])
@pytest.mark.parametrize("weights", [(7, 13), (0, 0)], ids=str)
def test_score_range_merged_levels(weights, ranks, monkeypatch):
    """merge_levels_kernel over shards whose lists end at their 32nd level, more than 32 distinct scores between them
    (7,13); one level on every shard, far beyond the exchange capacity (0,0)"""
    monkeypatch.setenv("GS_XCHG", "levels")
    c, want = lu.range_case(weights)
    _ranks_same(c, config.make_config(c.num_nodes, weights=weights), ranks, want)


@pytest.mark.parametrize("weights", [(7, 13), (0, 0)], ids=str)
def test_score_range_node_sampling(weights):
    """commit_window_kernel (percentageOfNodesToScore = 10) over the same rows"""
    c = lu.range_cluster(3000, 300, False)
    e, o = sampling_pair(c, 10, weights=weights)
    sampling_check(e, o, c.pods)
    assert e.mirror_check() == 0


def test_max_total_score_limit():
    """weights whose maximum total score passes 2047 are refused at construction; 2000 is admitted"""
    with pytest.raises(GpuScoreError):
        Engine(config.make_config(64, weights=(11, 10)))
    Engine(config.make_config(64, weights=(10, 10))).close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a context that has scheduled alone becomes a rank of a group

def test_reshard_after_scheduling_alone(monkeypatch):
    """Two contexts each place pods 0-255 alone over rows of 2,200 entries (both batch slots), then form a 2-rank group
    under GS_XCHG=levels (rows of 1,100) and place pods 256-383 together: one stream of 384 placements, the oracle's.
    The eval pass rewrites [0, 1280) of a row and the level kernels read [0, 1536): entries 1280-1535 (feasible, low
    scoring nodes in the lone phase) must be padding again after the comm init, or `feasible` counts them."""
    monkeypatch.setenv("GS_XCHG", "levels")
    c, want = lu.reshard_case()
    a = lu.RESHARD_ALONE
    seq = np.arange(lu.RESHARD_PODS, dtype=np.uint64)
    engines = [_engine(c), _engine(c)]
    for x in engines:
        lu.same(x.schedule(c.pods[:a], seq[:a]), want[:a])
        assert x.stats()["batches"] >= 2
    g = LocalGroup(2)
    for r, x in enumerate(engines):
        x.comm_init_local(g, r)
    res = [None, None]

    def run(r):
        try:
            res[r] = engines[r].schedule(c.pods[a:], seq[a:])
        except Exception as ex:   # noqa: BLE001 (reported per rank)
            res[r] = ex
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for r in range(2):
        assert not isinstance(res[r], Exception) and res[r] is not None, (r, res[r])
        lu.same(res[r], want[a:])
        assert engines[r].mirror_check() == 0
    assert engines[0].stats()["shard_end"] == engines[1].stats()["shard_begin"] == 1100
