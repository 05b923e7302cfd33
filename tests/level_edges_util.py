"""Input builders for the candidate-level stage's edges (cand_kernel, the cs_hist / cs_pick / cs_list slice kernels,
fix_levels_kernel, merge_levels_kernel): row lengths and deciding nodes at the kernels' 512-entry steps, wave shares
and slices, top levels at the list capacities, and score ranges from one bin to the admitted maximum.

Every builder is cached together with the oracle's placements of its pods (computed once, shared by the CPU test that
proves the input reaches its edge and the GPU tests that compare against it; neither changes them).

The geometry restated here (gs_kernels.hip): a row of `len` entries is read as lenv = round_up(len, 512); cand_kernel
gives wave w of 4 the steps [w * seg, (w + 1) * seg) with seg = ceil(lenv / 512 / 4) * 512 and records a per-step
maximum for the first 128 steps of a wave; a call's first batch of <= 32 pods over lenv >= 4096 runs the slice kernels
with slices of round_up(ceil(lenv / min(64, ceil(lenv / 2048))), 2048) entries.
"""
from __future__ import annotations

import functools

import numpy as np

from koordinator_amd import abi, config, synth
from oracle import oracle as orc

FIELDS = ("node", "score", "ties", "feasible")
GiB = 1 << 30

# deciding positions: around cand_kernel's 8-entry lanes, 64-lane waves, 512-entry steps and the slice threshold
EDGE_POSITIONS = (0, 7, 8, 63, 64, 511, 512, 1023, 1024, 2047, 2048, 3583, 3584, 4095, 4096)
EDGE_SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3584, 3585, 4096, 4097, 6145)
SHARDED_EDGE_SIZES = (513, 1025, 2049, 3073)
CAPACITY_SIZES = (2047, 2048, 2049)          # one rank: LCAP = 2048 listed nodes per pod
SHARD_CAPACITY_SIZES = (512, 514)            # two ranks, GS_XCHG=levels: XCAP = 256 per (pod, shard)
WEIGHTS = ((0, 0), (1, 0), (0, 1), (7, 13), (10, 10), (20, 0))
NUMA_WEIGHTS = ((7, 7, 6), (0, 0, 1), (19, 0, 1))
LEVALL = 32                                  # levels a pod's lists hold at most


def oracle_schedule(c, cfg, pods=None):
    pods = c.pods if pods is None else pods
    o = orc.Oracle(cfg)
    synth.load_into(o, c)
    # (the NodeNUMAResource profile costs the oracle ~20x more per pair: its per-node work over 8 threads, same result)
    return o.schedule(pods, np.arange(len(pods), dtype=np.uint64), nthreads=8 if c.numa is not None else 1)


def same(got, want):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{f} differs first at pod {bad[0]}: gpu {got[bad[0]]} oracle {want[bad[0]]}"


def plain(c):
    """no raw-allocatable overrides, custom thresholds, metrics or assigned pods (test_gpu_chain's _plain)"""
    c.nodes["raw_allocatable_mask"] = 0
    c.nodes["custom_flags"] = 0
    c.metrics["exists"] = 0
    c.assigned_pods = c.assigned_pods[:0]
    c.assigned_node = c.assigned_node[:0]
    c.assigned_ts = c.assigned_ts[:0]
    c.pod_metrics = c.pod_metrics[:0]
    c.pm_offsets[:] = 0
    return c


def identical(c, idx=slice(None)):
    """empty nodes of 64 cores / 256 GiB (test_gpu_chain's _identical)"""
    c.nodes["requested"][idx] = 0
    c.nodes["nonzero_requested"][idx] = 0
    c.nodes["pod_count"][idx] = 0
    c.nodes["allocatable"][idx, 0] = 64000
    c.nodes["allocatable"][idx, 1] = 256 * GiB


def default_edges(n):
    return tuple(sorted({e for e in EDGE_POSITIONS + (n - 2, n - 1) if 0 <= e < n}))


def _edge_cluster(n, edges, pods):
    c = plain(synth.make_cluster(n, pods, 4))
    identical(c)
    c.nodes["requested"][:, 0] = 32000
    c.nodes["requested"][:, 1] = 128 * GiB
    e = np.asarray(edges, np.int64)
    c.nodes["requested"][e] = 0
    c.nodes["nonzero_requested"] = c.nodes["requested"][:, :2]
    return c


@functools.lru_cache(maxsize=None)
def edge_cluster(n, edges=None, pods=None):
    """(cluster, oracle placements, edges): n identical nodes, half requested except the empty `edges`; 3 pods per
    edge unless `pods` says otherwise. The empty nodes hold every pod's top levels."""
    edges = default_edges(n) if edges is None else tuple(edges)
    c = _edge_cluster(n, edges, 3 * len(edges) if pods is None else pods)
    return c, oracle_schedule(c, config.make_config(n)), edges


# ---- large rows
SLICED_N = 135_169      # lenv 135,680: 34 slices of 4096 (two 2048-entry loads each), the last one of 512 entries
SLICED_EDGES = tuple(g * 4096 + 2048 + d for g in (0, 16, 32) for d in (0, 2047)) + (33 * 4096, )
STEPCAP_N = 262_657     # lenv 263,168: waves 0-2 take 129 steps each (step 128 has no recorded maximum), wave 3 127
STEPCAP_EDGES = tuple(w * 66_048 + 65_536 + d for w in range(3) for d in (0, 511)) + (STEPCAP_N - 2, STEPCAP_N - 1)


def sliced_case():
    """three calls of 6 pods over 135,169 nodes: the slice kernels, deciding nodes in the second 2048 of slices"""
    return edge_cluster(SLICED_N, SLICED_EDGES, 18)


def stepcap_case():
    """one call of 34 pods (batch_size 64) over 262,657 nodes: cand_kernel, deciding nodes in the 129th step of waves"""
    return edge_cluster(STEPCAP_N, STEPCAP_EDGES, 34)


# ---- list capacity
def homogeneous(nodes, pods, seed):
    """identical empty nodes: one level of `nodes` nodes (test_gpu_parity's homogeneous_cluster, restated so that the
    CPU tests do not import a GPU module)"""
    c = plain(synth.make_cluster(nodes, pods, seed))
    c.nodes["requested"] = 0
    c.nodes["nonzero_requested"] = 0
    c.nodes["allocatable"][:, 0] = 64000
    c.nodes["allocatable"][:, 1] = 256 * GiB
    return c


@functools.lru_cache(maxsize=None)
def capacity_case(n):
    c = homogeneous(n, 40, 6)
    return c, oracle_schedule(c, config.make_config(n))


# ---- score range
def enabled_of(weights):
    return abi.GS_ENABLE_ALL if len(weights) == 3 else abi.GS_ENABLE_LA_FIT


@functools.lru_cache(maxsize=None)
def range_cluster(nodes, pods, numa):
    c = synth.make_cluster(nodes, pods, 5)
    if numa:
        synth.make_numa(c)
    return c


@functools.lru_cache(maxsize=None)
def range_case(weights, nodes=3000, pods=300):
    """(cluster, oracle placements) of the C-synth cluster under the plugin weights `weights` (three of them: with the
    NodeNUMAResource plugin)"""
    c = range_cluster(nodes, pods, len(weights) == 3)
    return c, oracle_schedule(c, config.make_config(nodes, weights=weights, enabled=enabled_of(weights)))


def top_levels_cover(scores, levels=LEVALL):
    """per row of a (pods, nodes) score array: the nodes its `levels` highest distinct feasible scores hold"""
    out = np.zeros(len(scores), np.int64)
    for k, row in enumerate(scores):
        u, cnt = np.unique(row[row >= 0], return_counts=True)
        out[k] = cnt[-levels:].sum()
    return out


# ---- re-sharding a used context
RESHARD_N = 2200
RESHARD_GHOSTS = slice(1280, 1536)   # past round_up(1100, 256) = 1280 of a two-rank shard's row, below round_up(1100, 512)
RESHARD_ALONE, RESHARD_PODS = 256, 384


@functools.lru_cache(maxsize=None)
def reshard_case():
    """2,200 nodes, 384 pods: nodes 1280-1535 take every pod but are 87.5% requested (far below every listed level),
    the others lightly loaded at 13 x 7 different fills"""
    c = plain(synth.make_cluster(RESHARD_N, RESHARD_PODS, 8))
    identical(c)
    i = np.arange(RESHARD_N)
    c.nodes["requested"][:, 0] = (i % 13) * 1000
    c.nodes["requested"][:, 1] = (i % 7) * 4 * GiB
    c.nodes["requested"][RESHARD_GHOSTS, 0] = 56000
    c.nodes["requested"][RESHARD_GHOSTS, 1] = 224 * GiB
    c.nodes["nonzero_requested"] = c.nodes["requested"][:, :2]
    return c, oracle_schedule(c, config.make_config(RESHARD_N))
