"""The NodeNUMAResource evaluation of a NUMA-policy node (koordinator_amd/csrc/gs_numa_dev.h numa_eval in every way the
device code compiles it, and gs_pair_wave.h pair_score_wave) at its zone-shape edges, against the oracle. Needs an
MI355X: -m gpu.

The inputs come from tests/numa_edges_util.py (its docstring names the lines of gs_numa_dev.h every family is aimed at);
tests/test_numa_edges.py shows from the oracle alone that they reach those edges.

Pairs (nothing is scheduled): over all 64 x N pairs of the pairs cluster, under each of the three configured hint_score
variants and once with the NUMA Filter disabled,
* gs_evaluate (eval_numa_kernel: HintRegs, the rows from HBM and, for this batch of 64, from gather_numa_kernel's slab)
  equals the oracle's evaluate element for element: codes, per-plugin scores, totals;
* pair_probe mode 0 (row_score_wave: hints_merge_wave), mode 2 (pair_score_wave) over every pair and mode 1 (row_score
  over the HintTable hint_table_fill builds in LDS: every node x all 64 pods) equal the oracle's totals — the oracle's,
  not the engine's own evaluate.

Sequences: every walk case (pods of the call fill zone 0 exactly, the next ones are split over 2, 3 or 4 zones of the
state those pods left), every directed case (one per non-zero mask of every zone count) and every random 8-node cluster
runs through both commit kernels ("spec": commit_spec_kernel, percentage_of_nodes_to_score unset; "window":
commit_window_kernel, percentage_of_nodes_to_score = 50, which below 100 nodes makes the whole ring the window;
tests/test_gpu_cpuset_edges.py explains the selection) with one batch per call (batch_size 128: the slab path for the
random clusters' 128 pods) and with several: batch_size 16 for the random clusters; 4 for the directed cases, whose
calls have 6 and 3 pods (16 would be one batch again); 4 and 2 for the walk cases. With several batches
fix_levels_kernel and patch_kernel re-evaluate landed policy rows, and batches below 32 pods skip the slab. Over two gs_schedule calls node, score, ties, feasible, the Reserve flags
(GS_PLACED_NUMA, GS_PLACED_CPUSET, the affinity bits) and every allocation, byte for byte, equal the oracle's, under
verify_cpusets and with the HBM mirror equal to the host's afterwards; no batch is cut and no pod resolved on the host
(every topology is inside the device cpuset scope). The random clusters also run on 2 ranks over the callback transport:
winners on the other rank's shard enter as off-shard rows."""
import threading
import time

import numpy as np
import pytest

from koordinator_amd import abi
from tests import numa_edges_util as nu

pytestmark = pytest.mark.gpu

KERNELS = {"spec": False, "window": True}   # kernel -> node sampling (numa_edges_util's `sampled`)
CONFIGS = [(v, False) for v in nu.PAIR_VARIANTS] + [("default", True)]
CONFIG_IDS = [v + ("-score_only" if so else "") for v, so in CONFIGS]


def _pairs_engine(variant, score_only):
    from koordinator_amd.engine import Engine
    e = Engine(nu.pairs_config(variant, score_only, device=0))
    nu.load(e, nu.pairs_nodes())
    return e


def _name(j, i):
    return f"pod {j} ({nu.pairs_pods()[j].note}) on node {i} ({nu.pairs_nodes()[i].name})"


@pytest.mark.parametrize("variant,score_only", CONFIGS, ids=CONFIG_IDS)
def test_evaluate_matches_oracle(variant, score_only):
    e = _pairs_engine(variant, score_only)
    pods = nu.pod_records(nu.pairs_pods(), nu.UID_PAIRS)
    gs, gc, gp = e.evaluate(pods)
    os_, oc, op = nu.pairs_oracle(variant, score_only)
    e.close()
    bad = np.argwhere(gc != oc)
    assert not len(bad), f"{len(bad)} filter codes differ, first at {_name(*bad[0])}: gpu {gc[tuple(bad[0])]:#x} oracle {oc[tuple(bad[0])]:#x}"
    bad = np.argwhere(gp != op)
    assert not len(bad), f"{len(bad)} plugin scores differ, first at {_name(*bad[0][:2])}: gpu {gp[tuple(bad[0][:2])]} oracle {op[tuple(bad[0][:2])]}"
    bad = np.argwhere(gs != os_)
    assert not len(bad), f"{len(bad)} totals differ, first at {_name(*bad[0])}"


@pytest.mark.parametrize("variant,score_only", CONFIGS, ids=CONFIG_IDS)
def test_pair_probes_match_oracle(variant, score_only):
    e = _pairs_engine(variant, score_only)
    pods = nu.pod_records(nu.pairs_pods(), nu.UID_PAIRS)
    want, _, _ = nu.pairs_oracle(variant, score_only)       # [pod, node]
    want = want.astype(np.int32)
    P, N = want.shape
    pod_of, nodes = [a.ravel() for a in np.meshgrid(np.arange(P, dtype=np.int32), np.arange(N, dtype=np.uint32), indexing="ij")]
    ref = want[pod_of, nodes]
    for mode, what in ((0, "row_score_wave"), (2, "pair_score_wave")):
        s, _, _ = e.pair_probe(pods, nodes, pod_of, mode)
        bad = np.nonzero(s != ref)[0]
        assert not len(bad), (f"{what}: {len(bad)} pairs differ, first at {_name(pod_of[bad[0]], nodes[bad[0]])}: "
                              f"gpu {s[bad[0]]} oracle {ref[bad[0]]}")
    rows = np.arange(N, dtype=np.uint32)
    s1, _, _ = e.pair_probe(pods, rows, np.zeros(N, np.int32), 1)
    e.close()
    bad = np.argwhere(s1 != want.T)
    assert not len(bad), (f"row_score over the HintTable: {len(bad)} pairs differ, first at {_name(bad[0][1], bad[0][0])}: "
                          f"gpu {s1[tuple(bad[0])]} oracle {want.T[tuple(bad[0])]}")


# ---------------------------------------------------------------------------------------------------------------------
# sequences

def _compare(case, k, got, allocation, who=""):
    want = case.want[k]
    pods = case.calls[k]
    for f in nu.FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), f"{who}call {k}: {f} differs at pod {bad[0]} ({case.pods[k][bad[0]]}): gpu {got[bad[0]]} oracle {want[bad[0]]}"
    assert np.array_equal(got["flags"] & nu.RESERVE_MASK, want["flags"] & nu.RESERVE_MASK), \
        f"{who}call {k}: Reserve flags differ at pods {np.nonzero((got['flags'] ^ want['flags']) & nu.RESERVE_MASK)[0][:8]}"
    for j in np.nonzero(want["flags"] & (abi.GS_PLACED_CPUSET | abi.GS_PLACED_NUMA))[0]:
        a = allocation(int(got["node"][j]), int(pods["uid"][j]))
        wa = case.want_alloc[k][int(j)]
        assert (a is None) == (wa is None), f"{who}call {k} pod {j}: allocation presence differs"
        if a is not None and a.tobytes() != wa:
            w = np.frombuffer(wa, abi.POD_ALLOCATION_DTYPE)[0]
            raise AssertionError(f"{who}call {k} pod {j} ({case.pods[k][j]}) on node {got['node'][j]}: allocation differs: "
                                 f"gpu {a['numa'][:int(a['num_numa'])]} {nu.numa.cpus_of(a['cpuset'])} "
                                 f"oracle {w['numa'][:int(w['num_numa'])]} {nu.numa.cpus_of(w['cpuset'])}")


def _check(case, kernel, batch):
    from koordinator_amd.engine import Engine
    t0 = time.perf_counter()
    e = Engine(case.config(device=0, batch_size=batch))
    try:
        nu.load(e, case.nodes)
        e.verify_cpusets(True)
        e.reset_stats()
        lo = placed = 0
        for k, pods in enumerate(case.calls):
            got = e.schedule(pods, np.arange(lo, lo + len(pods), dtype=np.uint64))
            lo += len(pods)
            _compare(case, k, got, e.allocation)
            placed += int((got["node"] >= 0).sum())
        assert e.mirror_check() == 0, "HBM mirror diverged from the host mirror"
        st = e.stats()
    finally:
        e.close()
    print(f"{kernel}/{batch}: {placed} pods placed, cuts {st['cuts']}, slowpath_pods {st['slowpath_pods']}, "
          f"batches {st['batches']}, {time.perf_counter() - t0:.2f} s")
    assert st["cuts"] == 0 and st["slowpath_pods"] == 0, f"a batch was cut or a pod resolved on the host: {st}"
    return st


@pytest.mark.parametrize("batch", [128, 4])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", nu.directed_names())
def test_directed_case(name, kernel, batch):
    st = _check(nu.directed_case(name, KERNELS[kernel]), kernel, batch)
    assert st["batches"] >= (2 if batch == 128 else 3)


@pytest.mark.parametrize("batch", [128, 4, 2])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", nu.walk_names())
def test_walk_case(name, kernel, batch):
    """zone 0 filled exactly by pods of the call, then splits over 2, 3 or 4 zones computed from what those pods left:
    within one batch (128, and 4: the two fills and the splits) by the Reserve wave and the commit's re-scoring of the
    landed row; in batches of 2 the fills are one batch and the splits the next, so the splits' batch-start evaluation
    and fix_levels_kernel / patch_kernel read the landed row as well"""
    case = nu.walk_case(name, KERNELS[kernel])
    st = _check(case, kernel, batch)
    assert st["batches"] >= sum(-(-len(c) // batch) for c in case.calls)


@pytest.mark.parametrize("batch", [128, 16])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("seed", nu.RANDOM_SEEDS)
def test_random_cluster(seed, kernel, batch):
    st = _check(nu.edge_cluster(seed, KERNELS[kernel]), kernel, batch)
    assert st["batches"] >= (2 if batch == 128 else 9)


def _two_ranks(case, who):
    from koordinator_amd.engine import Engine
    engines, th = [], []
    barrier = threading.Barrier(2)
    try:
        for _ in range(2):
            engines.append(Engine(case.config(device=0)))
        for x in engines:
            nu.load(x, case.nodes)
            x.verify_cpusets(True)
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
        lo = 0
        for k, pods in enumerate(case.calls):
            res = [None, None]

            def run(r):
                res[r] = engines[r].schedule(pods, np.arange(lo, lo + len(pods), dtype=np.uint64))

            th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=120)
            assert not any(t.is_alive() for t in th), f"{who}: a rank did not finish call {k}"
            lo += len(pods)
            for r in range(2):
                assert res[r] is not None, f"{who}: rank {r} failed in call {k}"
                _compare(case, k, res[r], engines[r].allocation, f"{who} rank {r} ")
        for r in range(2):
            assert engines[r].mirror_check() == 0, f"{who} rank {r}: HBM mirror diverged"
            st = engines[r].stats()
            assert st["cuts"] == 0 and st["slowpath_pods"] == 0, f"{who} rank {r}: {st}"
    finally:
        # a rank still inside gs_schedule (its peer failed): release it from the all-gather before its engine goes
        if any(t.is_alive() for t in th):
            barrier.abort()
            for t in th:
                t.join(timeout=30)
        for r, x in enumerate(engines):
            if r >= len(th) or not th[r].is_alive():
                x.close()


def test_random_clusters_two_ranks_on_one_gpu_callback_transport():
    """Node-sharded (2 ranks, host all-gather) on one GPU: each rank owns 4 of the 8 nodes, every rank replays the same
    Reserve, and winners on the other rank's shard enter its commit as off-shard rows. No batch is cut and no pod
    resolved on the host on either rank; the engines are closed whatever happens."""
    for seed in nu.RANDOM_SEEDS:
        _two_ranks(nu.edge_cluster(seed), f"seed {seed}")
