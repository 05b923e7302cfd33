"""The per-batch commit chain (commit -> fix-up of the next batch's stale levels -> next commit), against the oracle's
sequential scheduleOne on node, score, ties and feasible. Needs an MI355X: -m gpu.

* Tie-break records: cand_kernel writes a batch's selectHost tie-break records beside the previous batch's commit, one
  buffer per batch slot; the commit's prologue computes them only where no cand_kernel ran for the batch (a short batch
  whose levels come from the cs_* slice kernels). Clusters of identical nodes make the tie-break position decide almost
  every pod.
* Fix-up: the commit leaves the rows its committed pods landed on in a slab (NUMA-policy rows first), and the next
  batch's fix_levels_kernel re-scores them from there and folds them into that batch's stale levels. A few nodes much
  emptier than the rest make several pods of a batch land on one node (one slab row for several placements), on
  NUMA-policy rows and rows without a policy; a pod whose cpuset the host selects ends a batch early (committed < b)."""
import functools

import numpy as np
import pytest

from koordinator_amd import abi, config, synth
from koordinator_amd.engine import Engine
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
FIELDS = ("node", "score", "ties", "feasible")


def _oracle(c, cfg, pods):
    o = orc.Oracle(cfg)
    synth.load_into(o, c)
    return o.schedule(pods, np.arange(len(pods), dtype=np.uint64))


def _engine(c, **kw):
    e = Engine(config.make_config(c.num_nodes, device=0, **kw))
    synth.load_into(e, c)
    return e


def _same(got, want):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{f} differs first at pod {bad[0]}: gpu {got[bad[0]]} oracle {want[bad[0]]}"


def _submit_three(e, pods, chunk):
    """pods in submissions of `chunk`, three of them outstanding at a time"""
    seq = np.arange(len(pods), dtype=np.uint64)
    hs, outs = [], []
    for lo in range(0, len(pods), chunk):
        hs.append(e.schedule_submit(pods[lo:lo + chunk], seq[lo:lo + chunk]))
        if len(hs) == 3:
            outs.append(e.schedule_wait(hs.pop(0)))
    outs += [e.schedule_wait(h) for h in hs]
    return np.concatenate(outs)


# ---------------------------------------------------------------------------------------------------------------------
# tie-breaks

def _identical(c, idx):
    c.nodes["requested"][idx] = 0
    c.nodes["nonzero_requested"][idx] = 0
    c.nodes["allocatable"][idx, 0] = 64000
    c.nodes["allocatable"][idx, 1] = 256 << 30


def _plain(c):
    c.nodes["raw_allocatable_mask"] = 0
    c.nodes["custom_flags"] = 0
    c.metrics["exists"] = 0
    c.assigned_pods = c.assigned_pods[:0]
    c.assigned_node = c.assigned_node[:0]
    c.assigned_ts = c.assigned_ts[:0]
    c.pod_metrics = c.pod_metrics[:0]
    c.pm_offsets[:] = 0
    return c


@functools.lru_cache(maxsize=None)
def _ties_case():
    """300 identical empty nodes, 384 pods: the top level holds hundreds of nodes until most rows are landed on"""
    c = _plain(synth.make_cluster(300, 384, 4))
    _identical(c, slice(None))
    want = _oracle(c, config.make_config(c.num_nodes), c.pods)
    assert np.median(want["ties"]) > 100 and (want["ties"] > 1).mean() > 0.95
    return c, want


@pytest.mark.parametrize("batch", [1, 31, 64, 65, 128])
def test_tiebreaks_blocking(batch):
    c, want = _ties_case()
    P = min(3 * batch + 45, 384)
    e = _engine(c, batch_size=batch)
    _same(e.schedule(c.pods[:P], np.arange(P, dtype=np.uint64)), want[:P])
    assert e.mirror_check() == 0


@pytest.mark.parametrize("batch", [1, 31, 64, 65, 128])
def test_tiebreaks_three_submissions_in_flight(batch):
    """Both tie-break buffers in use: batch k + 1's records are written while batch k's commit reads its own; the
    submissions' last batches are short ones."""
    c, want = _ties_case()
    P = min(3 * batch + 45, 384)
    e = _engine(c, batch_size=batch)
    _same(_submit_three(e, c.pods[:P], max(batch + 7, 16)), want[:P])
    assert e.mirror_check() == 0


def test_tiebreaks_short_batches_over_sliced_rows():
    """Rows of 4,500 entries: a call's first batch of <= 32 pods builds its levels with the cs_* slice kernels, which write
    no tie-break records (the commit computes them); the 300 identical empty nodes hold every top level."""
    c = _plain(synth.make_cluster(4500, 124, 4))
    _identical(c, slice(None))
    c.nodes["requested"][300:, 0] = 32000
    c.nodes["requested"][300:, 1] = 128 << 30
    c.nodes["nonzero_requested"][300:] = c.nodes["requested"][300:, :2]
    want = _oracle(c, config.make_config(c.num_nodes), c.pods)
    assert np.median(want["ties"]) > 100
    e = _engine(c)
    seq = np.arange(len(c.pods), dtype=np.uint64)
    got = np.concatenate([e.schedule(c.pods[lo:lo + 31], seq[lo:lo + 31]) for lo in range(0, 124, 31)])
    _same(got, want)
    assert e.mirror_check() == 0


# ---------------------------------------------------------------------------------------------------------------------
# fix-up

def _empty(c, idx):
    c.nodes["requested"][idx] = 0
    c.nodes["nonzero_requested"][idx] = 0
    c.nodes["pod_count"][idx] = 0
    c.metrics["node_usage"]["cpu_milli"][idx] = 0
    c.metrics["node_usage"]["memory"][idx] = 0


def _host_scope_nodes(c):
    """nodes whose topology has more cores than the device selects cpusets over (the mixed profile's SMT-1 classes)"""
    host_t = [i for i, t in enumerate(c.numa["topologies"]) if len(set(t["core_id"][:t["num_cpus"]].tolist())) > 128]
    return np.nonzero(np.isin(c.numa["node_numa"]["topology"], host_t))[0]


def _c3(host_pod):
    """The C3 synth at 3,000 nodes, 3 x 128 pods, six nodes emptied (three with a NUMA topology policy, three without).
    host_pod: the mixed topology classes, and pod 168 (the middle batch's) an LSR pod of 120 CPUs, which only the wide
    SMT-1 nodes hold: the host selects its cpuset."""
    c = synth.make_cluster(3000, 384, 2)
    synth.make_numa(c, cpuset_pod_pct=0 if host_pod else 3, mixed=host_pod)
    pol = c.numa["node_numa"]["numa_topology_policy"] != 0
    ok = c.metrics["exists"].astype(bool) & (c.nodes["custom_flags"] == 0)
    _empty(c, np.concatenate([np.nonzero(ok & pol)[0][:3], np.nonzero(ok & ~pol)[0][:3]]))
    if host_pod:
        p, k = c.pods, 168
        p["requests"][k, 0] = p["nonzero_requests"][k, 0] = p["limits"][k, 0] = 120_000
        p["requests"][k, 1] = p["nonzero_requests"][k, 1] = p["limits"][k, 1] = max(p["requests"][k, 1], 256 << 20)
        p["request_mask"][k] = (1 << abi.GS_RES_CPU) | (1 << abi.GS_RES_MEMORY)
        p["priority_class"][k] = abi.GS_PRIO_PROD
        p["qos_class"][k] = abi.GS_QOS_LSR
    want = _oracle(c, config.make_config(c.num_nodes, enabled=abi.GS_ENABLE_ALL), c.pods)
    for b in range(3):   # every batch: nodes several of its pods land on, landed rows with and without a policy
        n = want["node"][b * 128:(b + 1) * 128]
        u, cnt = np.unique(n[n >= 0], return_counts=True)
        assert (cnt > 1).sum() >= 5 and pol[u].sum() >= 10 and (~pol[u]).sum() >= 10, (b, cnt, pol[u].sum())
    if host_pod:
        assert want["node"][168] in _host_scope_nodes(c)
    return c, want


@pytest.mark.parametrize("host_pod", [False, True], ids=["full-batches", "middle-batch-ends-early"])
def test_fixup_landed_rows(host_pod):
    c, want = _c3(host_pod)
    e = _engine(c, enabled=abi.GS_ENABLE_ALL)
    _same(_submit_three(e, c.pods, 128), want)
    assert e.mirror_check() == 0
    st = e.stats()
    if host_pod:
        assert st["cuts"] >= 1, "no batch ended early: the host-selected cpuset was not exercised"
    else:
        assert st["cuts"] == 0 and st["slowpath_pods"] == 0, st
