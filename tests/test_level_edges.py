"""The inputs of tests/test_gpu_level_edges.py do what they claim, from the CPU oracle alone: every edge node is landed
on (and nothing else is), the capacity clusters' top level holds exactly the nodes that fit or pass the list, the wide
weight sets spread a row over more levels than a pod's lists hold, and the zero weights leave one level. Without these
the GPU comparisons could pass with the deciding nodes anywhere."""
import numpy as np
import pytest

from koordinator_amd import config, synth
from oracle import oracle as orc
from tests import level_edges_util as lu


def _landed_exactly_on_edges(want, edges):
    assert (want["node"] >= 0).all()
    assert set(want["node"].tolist()) == set(edges)


@pytest.mark.parametrize("n", sorted(set(lu.EDGE_SIZES + lu.SHARDED_EDGE_SIZES)))
def test_edge_clusters_land_on_every_edge_and_nowhere_else(n):
    _, want, edges = lu.edge_cluster(n)
    assert len(want) == 3 * len(edges)
    assert edges == tuple(e for e in sorted(set(lu.EDGE_POSITIONS + (n - 2, n - 1))) if 0 <= e < n)
    _landed_exactly_on_edges(want, edges)
    # the first pod sees every edge at the top level, every node feasible
    assert want["ties"][0] == len(edges) and (want["feasible"] == n).all()


def test_sliced_rows_geometry_and_edges():
    """135,169 nodes: 34 slices of 4096 entries, so cs_hist_kernel's second load and cs_list_kernel's second 2048 run;
    the edges sit at both ends of second halves, and alone in the last (512-entry) slice."""
    n = lu.SLICED_N
    lenv = (n + 511) // 512 * 512
    g0 = min(64, (lenv + 2047) // 2048)
    sl = ((lenv + g0 - 1) // g0 + 2047) // 2048 * 2048
    assert (lenv, sl, (lenv + sl - 1) // sl, lenv - 33 * sl) == (135_680, 4096, 34, 512)
    _, want, edges = lu.sliced_case()
    assert len(want) == 18 and all(e % sl >= 2048 or e // sl == 33 for e in edges) and n - 1 in edges
    _landed_exactly_on_edges(want, edges)


def test_stepcap_rows_geometry_and_edges():
    """262,657 nodes: waves 0-2 of cand_kernel take 129 steps, one past the 128 with a recorded maximum; the edges sit
    at both ends of that step, and at the end of the last wave's share."""
    n = lu.STEPCAP_N
    lenv = (n + 511) // 512 * 512
    seg = (lenv // 512 + 3) // 4 * 512
    assert n > 262_144 and seg == 129 * 512 and lenv - 3 * seg == 127 * 512
    _, want, edges = lu.stepcap_case()
    assert len(want) > 32
    for w in range(3):
        assert {w * seg + 128 * 512, w * seg + 128 * 512 + 511} <= set(edges)
    assert {e // seg for e in edges} == {0, 1, 2, 3}
    _landed_exactly_on_edges(want, edges)


@pytest.mark.parametrize("n", lu.CAPACITY_SIZES + lu.SHARD_CAPACITY_SIZES)
def test_capacity_clusters_top_level_is_the_whole_cluster(n):
    _, want = lu.capacity_case(n)
    assert want["ties"][0] == n and want["feasible"][0] == n
    # every later pod still sees a top level within a pod's distance of the capacity
    assert (want["ties"] >= n - len(want)).all() and (want["node"] >= 0).all()


def test_wide_weights_spread_rows_over_more_levels_than_the_lists_hold():
    """(7,13) on the 3,000-node synth cluster: hundreds of distinct scores per row; the 32 highest hold far fewer than
    the 128 nodes a full batch's last pod wants listed, so the level count (not the node count) ends the lists."""
    c = lu.range_cluster(3000, 300, False)
    o = orc.Oracle(config.make_config(3000, weights=(7, 13)))
    synth.load_into(o, c)
    scores, _, _ = o.evaluate(c.pods)
    distinct = np.array([len(np.unique(r[r >= 0])) for r in scores])
    cover = lu.top_levels_cover(scores)
    assert np.median(distinct) > 500 and scores.max() > 1500
    assert (cover < 128).mean() > 0.9 and np.median(cover) < 64, (np.median(cover), cover.max())
    assert (cover >= lu.LEVALL).all()


def test_zero_weights_leave_one_level():
    _, want = lu.range_case((0, 0))
    assert (want["ties"] == want["feasible"]).all() and (want["score"] == 0).all() and (want["feasible"] > 1000).all()


@pytest.mark.parametrize("weights", lu.WEIGHTS + lu.NUMA_WEIGHTS)
def test_weight_sets_place_pods(weights):
    _, want = lu.range_case(weights)
    assert (want["node"] >= 0).mean() > 0.9
    assert want["score"].max() <= 100 * sum(weights)
    if sum(weights) >= 20:
        assert want["score"].max() > 1000   # past the int8 range of a level index, the three-plugin sets included


def test_reshard_cluster_keeps_ghost_range_feasible_and_unlisted():
    c, want = lu.reshard_case()
    g = lu.RESHARD_GHOSTS
    assert (want["feasible"] == lu.RESHARD_N).all(), "a ghost-range node became infeasible: stale entries would hide"
    assert not ((want["node"] >= g.start) & (want["node"] < g.stop)).any()
    # two-rank shards of 1,100 rows: the eval pass rewrites [0, 1280), the level kernels read [0, 1536)
    per = (lu.RESHARD_N + 1) // 2
    assert ((per + 255) // 256 * 256, (per + 511) // 512 * 512) == (g.start, g.stop)
    assert len(np.unique(want["score"])) > 3
