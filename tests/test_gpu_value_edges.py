"""The HIP path on the edge-value cluster (tests/value_edges_util.py; its input conditions are checked on the CPU by
tests/test_value_edges.py): byte-granular capacities whose float32 division estimates need both +-1 corrections, odd
and zero allocatables, over-committed nodes, exact fits, last pod slots and the batch / mid resource slots, through
gs_evaluate, the commit's re-scoring forms (pair_probe) and the batch pipeline against the oracle's sequential run;
and the range / configuration gates in front of that arithmetic. Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from koordinator_amd import abi, config, synth
from oracle import oracle as orc
from tests import value_edges_util as ve
from tests.test_gpu_chain import FIELDS, _same, _submit_three

pytestmark = pytest.mark.gpu
TOP = 1 << 53


def _engine(c, cfg):
    from koordinator_amd.engine import Engine
    e = Engine(cfg)
    synth.load_into(e, c)
    return e


def _same_eval(got, want, what):
    for name, g, w in zip(("totals", "codes", "plugin scores"), got, want):
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: {name} differ at {len(bad)} entries, first (pod, node[, plugin]) {bad[0]}: " \
                             f"gpu {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


# ---------------------------------------------------------------------------------------------------------------------
# per-pair arithmetic

@pytest.mark.parametrize("profile,numa", [("default", False), ("weighted", False), ("weighted", True)],
                         ids=["default", "weighted", "weighted-numa"])
def test_evaluate_matches_oracle_and_integer_reference(profile, numa):
    c = ve.edge_cluster(numa)
    cfg, want = ve.oracle_eval(profile, numa)
    e = _engine(c, cfg)
    got = e.evaluate(c.pods)
    _same_eval(got, want, "gs_evaluate against the oracle")
    if not numa:   # (NodeResourcesFit does not read the NUMA state: the same columns)
        rcodes, rscores = ve.fit_reference(c, list(cfg.fit.resource_weights))
        assert np.array_equal(got[1] & np.uint16(0x1F), rcodes), "Fit filter codes differ from the integer reference"
        assert np.array_equal(got[2][:, :, abi.GS_PLUGIN_FIT], rscores), "Fit scores differ from the integer reference"


@pytest.mark.parametrize("numa", [False, True], ids=["plain", "numa"])
def test_pair_probe_matches_evaluate(numa):
    """The commit kernel's forms of the pair evaluation (whole-wave, lane-parallel, one pod per lane; scalar slots from
    the row copy) on every edge row, 64 pods at a time: the same totals as gs_evaluate, which equal the oracle's."""
    c = ve.edge_cluster(numa)
    cfg, (totals, _, _) = ve.oracle_eval("weighted", numa)
    e = _engine(c, cfg)
    nodes = np.arange(c.num_nodes, dtype=np.uint32)
    # one pod of every kind first, then the pods as they come
    first = {}
    for i in range(len(c.pods)):
        first.setdefault(ve.pod_kind(i), i)
    sel = list(first.values()) + [i for i in range(len(c.pods)) if i not in first.values()]
    for lo in (0, 64):
        pods = c.pods[sel[lo:lo + 64]]
        want, _, _ = e.evaluate(pods)
        assert np.array_equal(want, totals[sel[lo:lo + 64]]), "gs_evaluate differs from the oracle"
        pod_of = ((np.arange(c.num_nodes) * 7 + lo) % 64).astype(np.int32)
        ref = want[pod_of, nodes].astype(np.int32)
        for mode in (0, 2):
            s, _, _ = e.pair_probe(pods, nodes, pod_of, mode)
            bad = np.nonzero(s != ref)[0]
            assert not len(bad), f"mode {mode}: differs at nodes {bad[:5]}: got {s[bad[:5]]} want {ref[bad[:5]]}"
        s1, _, _ = e.pair_probe(pods, nodes, pod_of, 1)
        bad = np.argwhere(s1 != want.T.astype(np.int32))
        assert not len(bad), f"mode 1: differs first at (node, pod) {bad[0]}"


# ---------------------------------------------------------------------------------------------------------------------
# the batch pipeline on the edge rows

@pytest.mark.parametrize("how", ["batch-1", "batch-128", "three-in-flight"])
def test_schedule_matches_sequential_oracle(how):
    """Several pods of a batch land on one edge row, last pod slots and a node's batch-cpu run out inside a batch
    (test_value_edges.py asserts that on the oracle's run): the re-scored and fixed-up rows are the edge rows."""
    c = ve.edge_cluster()
    cfg, want, _ = ve.oracle_schedule()
    P = len(c.pods)
    cfg2 = ve.make_cfg(c, "weighted", batch_size=1 if how == "batch-1" else 128)
    e = _engine(c, cfg2)
    if how == "three-in-flight":
        got = _submit_three(e, c.pods, 128)
    else:
        got = e.schedule(c.pods[:P], np.arange(P, dtype=np.uint64))
    _same(got, want[:P])
    assert e.mirror_check() == 0


def test_schedule_with_node_sampling():
    """percentageOfNodesToScore = 50: the window commit kernel's own re-score of the edge rows, and the rotation's
    start index"""
    c = ve.edge_cluster()
    cfg, want, next_start = ve.oracle_schedule("weighted", 50)
    e = _engine(c, cfg)
    _same(e.schedule(c.pods, np.arange(len(c.pods), dtype=np.uint64)), want)
    assert e.stats()["next_start_node_index"] == next_start
    assert e.mirror_check() == 0


# ---------------------------------------------------------------------------------------------------------------------
# batch / mid slots under contention

BATCH_FIT = {"cpu": 1, "memory": 1, "kubernetes.io/batch-cpu": 2, "kubernetes.io/batch-memory": 1}


@pytest.mark.parametrize("batch,numa", [(128, False), (32, False), (128, True)], ids=["128", "32", "128-numa"])
def test_batch_slots_run_out(batch, numa):
    c = ve.batch_cluster(numa)
    cfg = config.make_config(c.num_nodes, fit=config.fit_args(BATCH_FIT), batch_size=batch,
                             enabled=abi.GS_ENABLE_ALL if numa else abi.GS_ENABLE_LA_FIT)
    o = orc.Oracle(cfg)
    synth.load_into(o, c)
    seq = np.arange(len(c.pods), dtype=np.uint64)
    want = o.schedule(c.pods, seq)
    be = c.pods["requests"][:, 3] > 0
    assert 0.35 < be.mean() < 0.45
    assert (want["node"][be] < 0).sum() >= 10 and (want["node"][be] >= 0).sum() >= 100, "the batch slots do not run out"
    e = _engine(c, cfg)
    _same(e.schedule(c.pods, seq), want)
    assert e.mirror_check() == 0
    assert e.stats()["cuts"] == 0     # (every topology is in the device's cpuset scope: no host-side Reserve)


# ---------------------------------------------------------------------------------------------------------------------
# configuration and range gates

@pytest.mark.parametrize("w", [-1, 0, 101])
def test_loadaware_weight_outside_range_is_refused(w):
    """validateResourceWeights (validation_pluginargs.go:61-70): a present key must lie in (0, 100]"""
    from koordinator_amd.engine import Engine, GpuScoreError
    la = config.loadaware_args(resourceWeights={"cpu": 1, "memory": w})
    with pytest.raises(GpuScoreError, match=f"gs_create failed: {abi.GS_EINVAL}"):
        Engine(config.make_config(64, la=la))


def test_loadaware_weight_100_is_exact():
    c = ve.edge_cluster()
    cfg = config.make_config(c.num_nodes, la=config.loadaware_args(resourceWeights={"cpu": 100, "memory": 37}),
                             fit=config.fit_args({"cpu": 100, "memory": 99, "kubernetes.io/batch-cpu": 100}))
    o = orc.Oracle(cfg)
    synth.load_into(o, c)
    _same_eval(_engine(c, cfg).evaluate(c.pods), o.evaluate(c.pods), "weights of 100")


def _small():
    c = synth.make_cluster(64, 8, 44)
    cfg = config.make_config(c.num_nodes)
    return c, cfg, _engine(c, cfg)


def test_top_of_the_range_is_accepted_and_exact():
    """allocatable, requested and pod requests of 2^53 - 1 in every slot the arithmetic reads"""
    c = synth.make_cluster(64, 8, 44)
    nd, p = c.nodes, c.pods
    nd["allocatable"][:8, :7] = TOP - 1
    nd["requested"][:4, :7] = 0
    nd["nonzero_requested"][:4] = 0
    nd["requested"][4:8, :7] = TOP - 1
    nd["nonzero_requested"][4:8] = TOP - 1
    nd["raw_allocatable_mask"][:8] = 0
    p["requests"][0, :2] = p["limits"][0, :2] = p["nonzero_requests"][0] = TOP - 1
    p["requests"][1, :2] = p["nonzero_requests"][1] = (TOP - 1) // 3
    p["limits"][1, :2] = TOP - 1
    p["requests"][2, 3] = p["limits"][2, 3] = TOP - 1
    p["request_mask"][2] |= 1 << 3
    cfg = config.make_config(c.num_nodes, fit=config.fit_args({"cpu": 1, "memory": 1, "kubernetes.io/batch-cpu": 1}))
    o = orc.Oracle(cfg)
    synth.load_into(o, c)
    e = _engine(c, cfg)
    want = o.evaluate(p)
    assert (want[1][0, :4] == 0).all() and (want[1][0, 4:8] != 0).all()   # fits the empty ones exactly
    _same_eval(e.evaluate(p), want, "quantities of 2^53 - 1")
    got, ws = e.schedule(p), o.schedule(p)
    for f in FIELDS:
        assert np.array_equal(got[f], ws[f]), f


@pytest.mark.parametrize("field,slot", [("allocatable", 1), ("allocatable", 3), ("requested", 0), ("requested", 4),
                                        ("nonzero_requested", 1), ("raw_allocatable", 0)])
def test_node_quantity_of_2_53_is_refused(field, slot):
    from koordinator_amd.engine import GpuScoreError
    c, _, e = _small()
    n = c.nodes[:1].copy()
    n[field][0, slot] = TOP
    with pytest.raises(GpuScoreError, match=f"gs_nodes_upsert: rc={abi.GS_EUNSUPPORTED}"):
        e.upsert_nodes(n, np.array([3], np.uint32))
    n[field][0, slot] = TOP - 1
    e.upsert_nodes(n, np.array([3], np.uint32))


@pytest.mark.parametrize("field,slot", [("requests", 1), ("requests", 4), ("limits", 0), ("nonzero_requests", 1)])
@pytest.mark.parametrize("call", ["schedule", "evaluate"])
def test_pod_quantity_of_2_53_is_refused(call, field, slot):
    from koordinator_amd.engine import GpuScoreError
    c, _, e = _small()
    p = c.pods.copy()
    p[field][5, slot] = TOP
    with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EUNSUPPORTED}"):
        getattr(e, call)(p)
    p[field][5, slot] = TOP - 1
    getattr(e, call)(p)


@pytest.mark.parametrize("field,slot", [("requested", 0), ("requested", 1), ("requested", 2), ("requested", 5),
                                        ("nonzero_requested", 0), ("nonzero_requested", 1)])
def test_negative_node_request_is_refused(field, slot):
    """NodeInfo never holds a negative Requested / NonZeroRequested; one would put the scored quantity above the
    capacity (the division's range is 0 <= x <= cap) and score 101 where the reference's plain division does not"""
    from koordinator_amd.engine import GpuScoreError
    c, _, e = _small()
    n = c.nodes[:1].copy()
    n[field][0, slot] = -1
    with pytest.raises(GpuScoreError, match=f"gs_nodes_upsert: rc={abi.GS_EINVAL}"):
        e.upsert_nodes(n, np.array([3], np.uint32))


@pytest.mark.parametrize("slot", [0, 1])
def test_negative_pod_nonzero_request_is_refused(slot):
    from koordinator_amd.engine import GpuScoreError
    c, _, e = _small()
    p = c.pods.copy()
    p["nonzero_requests"][2, slot] = -1
    with pytest.raises(GpuScoreError, match=f"rc={abi.GS_EUNSUPPORTED}"):
        e.evaluate(p)
