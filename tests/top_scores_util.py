"""The top-N score tables (gs_schedule_top_scores): the truth from the CPU oracle, and the checks the tests share.

Truth: the oracle schedules the pods one at a time; before pod i, or_evaluate of pod i on the unchanged state gives every
node's total and plugin scores at the pod's turn. The pod has no table when fewer than two nodes are feasible
([upstream] schedulePod returns before prioritizeNodes with one feasible node); else its table is the first topn of
lexsort(node ascending, total descending) over the feasible nodes. The first KEEP entries are kept per pod, so one
truth serves every topn (the order is total, so the first topn of the first KEEP are the first topn)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from koordinator_amd import abi, synth
from oracle import oracle as orc
from tests import fit_diag_util as fd

WINDOW = 128
KEEP = abi.GS_MAX_TOP_SCORES + 1   # one more than the largest table: whether the cut goes through a tie level


def top_rows(scores, plugin, keep: int = KEEP) -> np.ndarray:
    """The first `keep` feasible nodes of one pod by (total descending, node ascending), as TOP_SCORE_DTYPE rows."""
    feas = np.nonzero(scores >= 0)[0]
    order = feas[np.lexsort((feas, -scores[feas].astype(np.int32)))][:keep]
    rows = np.zeros(len(order), abi.TOP_SCORE_DTYPE)
    rows["node"] = order
    rows["total"] = scores[order]
    rows["plugin"] = plugin[order]
    return rows


def _tables(o: orc.Oracle, pods) -> list[np.ndarray]:
    out = []
    for k in range(len(pods)):
        scores, _, plugin = o.evaluate(pods[k:k + 1])
        out.append(top_rows(scores[0], plugin[0]))
    return out


class Truth:
    """placements[P] of the oracle and kept[i]: pod i's first KEEP feasible nodes at its turn (every feasible node when
    fewer). windows: also the same at the start and at the end of the pod's 128-pod window (start[i], end[i])."""

    def __init__(self, c: synth.Cluster, cfg, windows: bool = True):
        o = orc.Oracle(cfg)
        synth.load_into(o, c)
        P = len(c.pods)
        self.cfg = cfg
        self.placements = np.zeros(P, abi.PLACEMENT_DTYPE)
        self.kept: list[np.ndarray] = []
        self.start: list[np.ndarray] = []
        self.end: list[np.ndarray] = []
        for i in range(P):
            if windows and i % WINDOW == 0:
                self.start += _tables(o, c.pods[i:i + WINDOW])
            self.kept += _tables(o, c.pods[i:i + 1])
            self.placements[i] = o.schedule(c.pods[i:i + 1], np.array([i], np.uint64))[0]
            if windows and (i % WINDOW == WINDOW - 1 or i == P - 1):
                self.end += _tables(o, c.pods[i - i % WINDOW:i + 1])
        o.close()
        self.feasible = self.placements["feasible"].astype(np.int64)

    def count(self, topn: int) -> np.ndarray:
        return np.where(self.feasible >= 2, np.minimum(self.feasible, topn), 0).astype(np.uint32)

    def table(self, i: int, topn: int) -> np.ndarray:
        return self.kept[i][:int(self.count(topn)[i])]

    def moved(self, topn: int) -> np.ndarray:
        """Pods with a table that differs from both the table at their window's start and the one at its end."""
        cnt = self.count(topn)
        out = np.zeros(len(cnt), bool)
        for i in np.nonzero(cnt)[0]:
            t = self.kept[i][:cnt[i]]
            out[i] = not np.array_equal(t, self.start[i][:topn]) and not np.array_equal(t, self.end[i][:topn])
        return out

    def cut_tie(self, topn: int) -> np.ndarray:
        """Pods whose table ends inside a level: the best node left out has the total of the last one taken."""
        out = np.zeros(len(self.kept), bool)
        for i in np.nonzero(self.count(topn) == topn)[0]:
            k = self.kept[i]
            out[i] = len(k) > topn and k["total"][topn] == k["total"][topn - 1]
        return out

    def short(self, topn: int) -> np.ndarray:
        cnt = self.count(topn)
        return (cnt > 0) & (cnt < topn)


@functools.lru_cache(maxsize=None)
def case(n: int, p: int, cid: int, numa: bool, windows: bool = True):
    """(cluster, truth) of one tight cluster (fit_diag_util's), computed once per session; callers leave both unchanged."""
    c = fd.tight_cluster(n, p, cid, numa)
    return c, Truth(c, fd.make_cfg(c, numa), windows)


def weights_of(cfg) -> np.ndarray:
    return np.array([cfg.plugin_weights[k] for k in range(abi.GS_NUM_PLUGINS)], np.int64)


def same_placements(a, b) -> None:
    for f in ("node", "score", "ties", "feasible", "flags"):
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{f} differs at pod {bad[0]}: {a[bad[0]]} vs {b[bad[0]]}"


def check(got, rows, count, truth: Truth, topn: int, lo: int = 0, hi: int | None = None) -> None:
    """Placements, every count and every field of every row of pods [lo, hi) against the truth, and the rows' own
    invariants."""
    hi = len(truth.placements) if hi is None else hi
    want = truth.placements[lo:hi]
    for f in ("node", "score", "ties", "feasible"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{f} differs at pod {lo + bad[0]}: gpu {got[bad[0]]} oracle {want[bad[0]]}"
    assert rows.shape == (hi - lo, topn)
    wcnt = truth.count(topn)[lo:hi]
    bad = np.nonzero(count != wcnt)[0]
    assert bad.size == 0, f"{bad.size} counts differ, first at pod {lo + bad[0]}: gpu {count[bad[0]]} oracle {wcnt[bad[0]]}"
    w = weights_of(truth.cfg)
    for k in range(hi - lo):
        n = int(count[k])
        t = truth.table(lo + k, topn)
        assert np.array_equal(rows[k, :n], t), (
            f"pod {lo + k}: table differs at row {np.nonzero(rows[k, :n] != t)[0][0]}:\ngpu    {rows[k, :n]}\noracle {t}")
        assert not rows[k, n:].view(np.uint8).any(), f"pod {lo + k}: rows past its count were written"
        if not n:
            continue
        r = rows[k, :n]
        assert np.array_equal(r["total"].astype(np.int64), r["plugin"].astype(np.int64) @ w), f"pod {lo + k}: total"
        key = list(zip((-r["total"].astype(np.int64)).tolist(), r["node"].tolist()))
        assert key == sorted(key) and len(set(r["node"].tolist())) == n, f"pod {lo + k}: order"
        # a scored pod is placed on one of its best nodes
        assert r["total"][0] == got["score"][k], f"pod {lo + k}: best total {r['total'][0]}, placed at {got['score'][k]}"
        best = r["node"][r["total"] == r["total"][0]]
        ties = int(got["ties"][k])
        assert len(best) >= min(ties, topn), f"pod {lo + k}: {len(best)} rows at the best total, {ties} ties"
        if len(best) == ties:   # every tied node made the table (else the cut may have dropped the chosen one)
            assert got["node"][k] in best, f"pod {lo + k}: node {got['node'][k]} is not among the best rows {best}"


ONE_FEASIBLE_POD = 20


@functools.lru_cache(maxsize=None)
def one_feasible_case():
    """48 pods of the tight 700-node cluster; pod ONE_FEASIBLE_POD also requests batch-cpu, which one node alone has
    (the node it fits worst at the start, so that none of the pods before it is likely to fill it): the pod is placed
    there with one feasible node, which [upstream] schedulePod does not score."""
    c0 = fd.tight_cluster(700, 48, 0, False)
    c = dataclasses.replace(c0, nodes=c0.nodes.copy(), pods=c0.pods.copy())
    cfg = fd.make_cfg(c, False)
    k, b = ONE_FEASIBLE_POD, abi.GS_RES_BATCH_CPU
    o = orc.Oracle(cfg)
    synth.load_into(o, c)
    scores = o.evaluate(c.pods[k:k + 1])[0][0]
    o.close()
    feas = np.nonzero(scores >= 0)[0]
    node = int(feas[np.argmin(scores[feas])])
    c.nodes["allocatable"][:, b] = 0
    c.nodes["requested"][:, b] = 0
    c.nodes["allocatable"][node, b] = 3000
    c.pods["requests"][k, b] = 2000
    c.pods["request_mask"][k] |= 1 << b
    return c, Truth(c, cfg, windows=False)


@functools.lru_cache(maxsize=None)
def homogeneous_case(n: int, p: int):
    """Every node alike and empty, so that every node a pod has not landed on ties: pod k's table is the topn
    lowest-indexed nodes of the best level. From 1,024 nodes up the first 250 nodes are a little fuller (the best level
    starts past them and a table crosses the 256-node boundary of the kernel's compaction step) and three nodes, one of
    them past index 2,048, a little emptier (entries above the threshold late in the row)."""
    c0 = synth.make_cluster(n, p, 0)
    nodes = np.zeros(n, abi.NODE_DTYPE)
    nodes["allocatable"][:, 0] = 128_000
    nodes["allocatable"][:, 1] = 1 << 40
    nodes["allocatable"][:, 2] = 500 << 30
    nodes["requested"][:, 0] = nodes["nonzero_requested"][:, 0] = 8_000
    nodes["allowed_pod_number"] = 110
    if n >= 1024:
        nodes["requested"][:250, 0] = nodes["nonzero_requested"][:250, 0] = 16_000
        for i in (1000, n - 50, n - 1):
            nodes["requested"][i, 0] = nodes["nonzero_requested"][i, 0] = 0
    metrics = np.zeros(n, abi.METRIC_DTYPE)
    metrics[:] = c0.metrics[np.nonzero(c0.metrics["exists"])[0][0]]
    metrics["node_usage"]["cpu_milli"] = 4_000
    metrics["node_usage"]["memory"] = 8 << 30
    c = synth.Cluster(c0.now_ns, nodes, metrics, c0.pod_metrics[:0], np.zeros(n + 1, np.uint32), c0.assigned_node[:0],
                      c0.assigned_pods[:0], c0.assigned_ts[:0], c0.pods)
    return c, Truth(c, fd.make_cfg(c, False), windows=False)
