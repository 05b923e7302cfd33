"""The extension path (gs_schedule_ext: gs_ext.hip, ext_schedule_one, ext_device_reserve) against the oracle at its
request, device, reservation and select edges (tests/ext_edges_util.py builds the inputs and names the lines they are
aimed at; tests/test_ext_edges.py shows on the oracle alone that they reach them). Engine.ext_rows returns every node's
Filter verdict, raw scores, nomination and total beside the select result and changes no state, so a wrong verdict or
score on a losing node shows; the sequences then run the same pods through gs_schedule_ext, Reserves included.
Needs an MI355X: -m gpu."""
import types

import numpy as np
import pytest

from koordinator_amd import abi
from oracle import oracle as orc
from tests import ext_edges_util as xu
from tests import numa_edges_util as nu
from tests import test_gpu_ext as tge

pytestmark = pytest.mark.gpu


def _engine(case, args=None):
    from koordinator_amd.engine import Engine
    e = Engine(case.cfg())
    case.load(e, args)
    return e


def _state(x, case):
    """the state a Reserve would touch, as bytes"""
    devs = b"".join(x.devices(i).tobytes() for i in range(case.n))
    rsv = b"".join(x.reservation(int(r["uid"])).tobytes() for r in case.reservations)
    return devs, rsv


@pytest.mark.parametrize("key", xu.stateless_keys(), ids=str)
def test_rows_match_oracle_and_leave_no_state(key):
    case = xu.case_of(*key[:-1])
    e = _engine(case, xu.variant_args(case.args, dict(xu.VARIANTS)[key[-1]]))
    before = _state(e, case)
    xu.assert_rows_equal(xu.rows_of(e, case), xu.oracle_rows(*key), case.name)
    assert e.mirror_check() == 0 and _state(e, case) == before
    assert all(e.ext_reserved(int(u)) is None for u in case.pods["uid"])
    if case.numa_nodes is not None:
        assert all(e.allocation(i, int(u)) is None for u in case.pods["uid"] for i in (0, case.n - 1))
    # the rows once more after the probes: nothing they left behind changes them
    xu.assert_rows_equal(xu.rows_of(e, case, pods=range(0, len(case.pods), 7)),
                         [xu.oracle_rows(*key)[j] for j in range(0, len(case.pods), 7)], case.name + " (again)")


def _run_sequence(case, args=None, pods=None):
    """every pod in turn: the rows on the evolving state, then gs_schedule_ext against or_schedule_ext"""
    e, o = _engine(case, args), case.oracle(args)
    pods = range(len(case.pods)) if pods is None else pods
    got, want = [], []
    for k, j in enumerate(pods):
        seq = np.array([1000 + k], np.uint64)
        d = xu.rows_equal(e.ext_rows(case.pods[j], case.ext[j], 1000 + k), o.ext_rows(case.pods[j], case.ext[j], 1000 + k))
        assert d is None, f"{case.name}: rows of pod {j} ({k} scheduled before it): engine vs oracle {d}"
        got.append(e.schedule_ext(case.pods[j:j + 1], case.ext[j:j + 1], seq))
        want.append(o.schedule_ext(case.pods[j:j + 1], case.ext[j:j + 1], seq))
    ge = np.concatenate([x[0] for x in got]), np.concatenate([x[1] for x in got])
    oe = np.concatenate([x[0] for x in want]), np.concatenate([x[1] for x in want])
    c = types.SimpleNamespace(ext={"reservations": case.reservations, "devices": case.devices})
    placed = tge.check(c, e, o, ge, oe)
    return e, o, ge, oe, placed


@pytest.mark.parametrize("strategy,weights", [("LeastAllocated", (0, 1, 0)), ("MostAllocated", (1, 1, 1)),
                                              ("LeastAllocated", (3, 0, 2))], ids=str)
def test_pairs_cluster_in_sequence(strategy, weights):
    case = xu.ds_case(strategy, weights, 0)
    e, o, ge, oe, placed = _run_sequence(case)
    assert placed.sum() >= 30 and (ge[1]["gpu_count"] > 1).sum() >= 5 and (ge[1]["fail_code"] != 0).sum() >= 7


def test_mem0_and_policy_clusters_in_sequence():
    for case in (xu.ds_mem0_case(), xu.policy_case()):
        e, o, ge, oe, placed = _run_sequence(case)
        assert placed.sum() >= 10
        if case.numa_nodes is not None:
            assert np.array_equal(ge[0]["flags"][placed] & 6, oe[0]["flags"][placed] & 6)
            for j in np.nonzero(placed)[0]:
                uid, node = int(case.pods["uid"][j]), int(ge[0]["node"][j])
                a, b = e.allocation(node, uid), o.allocation(node, uid)
                assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), j


@pytest.mark.parametrize("variant", ["default", "coprime"])
def test_reservation_cluster_in_sequence(variant):
    case = xu.rsv_case()
    e, o, ge, oe, placed = _run_sequence(case, xu.variant_args(case.args, dict(xu.VARIANTS)[variant]))
    assert placed.sum() >= 25 and (ge[1]["reservation_uid"] > 0).sum() >= 12


def test_input_block_grows_with_the_owner():
    """owners with 1, then 600, then 5 matched records: the per-pod input block (ext_stage_reserve) starts at 64
    records, is reallocated for the second owner and serves the third"""
    rs = [xu.rsv(0xB000, 1, 3, xu.CM)]
    rs += [xu.rsv(0xC000 + i, 2, i, {0: 2000 + 100 * (i % 7), 1: 8 * xu.GiB}, order=(i % 13) if i % 3 == 0 else 0)
           for i in range(600)]
    rs += [xu.rsv(0xD000 + i, 3, 100 + i, xu.CM, policy="Restricted") for i in range(5)]
    nodes = xu.base_nodes(xu.N_WIDE)
    xu.hold(nodes, rs)
    c2 = {0: 2000, 1: 2 * xu.GiB}
    case = xu.Case("grow", nodes, np.zeros(xu.N_WIDE, abi.NODE_DEVICES_DTYPE), xu.pod_records([c2] * 6, 0xDA0000),
                   xu.ext_records(owner=[1, 2, 3, 2, 1, 3], required=[1, 0, 1, 1, 0, 0]), xu.ext_args(),
                   reservations=np.array(rs, abi.RESERVATION_DTYPE))
    e, o, ge, oe, placed = _run_sequence(case)
    assert placed.all() and (ge[1]["reservation_uid"] > 0).all()


@pytest.mark.parametrize("k", [1023, 1024, 1025, 2049])
def test_device_updates_across_the_staged_flush(k):
    """k Device objects change between two extension pods: ext_flush_devices stages 1024 images per copy"""
    n = 2100
    nodes = xu.base_nodes(n)
    devs = np.array([xu.device([xu.used_pct(0 if i % 10 == 0 else (3 * i + 10 * g) % 100) for g in range(4)])
                     for i in range(n)], abi.NODE_DEVICES_DTYPE)
    gpus = [{xu.KG: 100}, {xu.CO: 50, xu.RA: 50}, {xu.NV: 2}]
    case = xu.Case(f"flush-{k}", nodes, devs, xu.pod_records([{0: 1000, 1: xu.GiB}] * 3, 0xDB0000),
                   xu.ext_records(gpu=gpus), xu.ext_args("MostAllocated", (1, 1, 1)))
    e, o = _engine(case), case.oracle()
    seq = np.arange(3, dtype=np.uint64)
    got = [e.schedule_ext(case.pods[:1], case.ext[:1], seq[:1])]
    want = [o.schedule_ext(case.pods[:1], case.ext[:1], seq[:1])]
    idx = np.arange(k, dtype=np.uint32) * 2 + 1 if 2 * k < n else np.arange(n - k, n, dtype=np.uint32)   # odd nodes / a tail
    new = np.array([xu.device([xu.used_pct((5 * int(i) + 20 * g + 1) % 100) for g in range(4)]) for i in idx],
                   abi.NODE_DEVICES_DTYPE)
    for x in (e, o):
        x.upsert_devices(new, idx)
    for j in (1, 2):
        d = xu.rows_equal(e.ext_rows(case.pods[j], case.ext[j], j), o.ext_rows(case.pods[j], case.ext[j], j))
        assert d is None, f"pod {j} after {k} device updates: engine vs oracle {d}"
        got.append(e.schedule_ext(case.pods[j:j + 1], case.ext[j:j + 1], seq[j:j + 1]))
        want.append(o.schedule_ext(case.pods[j:j + 1], case.ext[j:j + 1], seq[j:j + 1]))
    for g, w in zip(got, want):
        assert g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes() and w[0]["node"][0] >= 0
    for i in list(idx[:40]) + list(idx[-40:]) + [int(w[0]["node"][0]) for w in want]:
        assert e.devices(int(i)).tobytes() == o.devices(int(i)).tobytes()
    assert e.mirror_check() == 0


# ---------------------------------------------------------------------------------------------------------------------
# select shapes

def _select(n, shapes, seqs):
    from koordinator_amd.engine import Engine
    e = None
    for shape in shapes:
        case = xu.select_case(n, shape)
        if e is None:
            e = Engine(case.cfg())
        o = case.oracle()
        case.load(e)
        ties = xu.select_ties(n, shape)
        for s in seqs:
            g, w = e.ext_rows(case.pods[0], case.ext[0], s), o.ext_rows(case.pods[0], case.ext[0], s)
            d = xu.rows_equal(g, w)
            assert d is None, f"{n} nodes, {shape}, seq {s}: engine vs oracle {d}"
            assert g["ties"] == len(ties)
    assert e.mirror_check() == 0


@pytest.mark.parametrize("n", xu.SELECT_N)
def test_select_shapes(n):
    _select(n, xu.SELECT_SHAPES, xu.SEQS)


def test_select_beyond_256_blocks():
    """262145 nodes are 257 blocks of 1024: the last block's threads own two block counts each (`per > 1`). Ties on the
    chunk and block boundaries of the first blocks, around the middle block, on the last full block's last node and on
    the last node alone (the only node of block 256). The oracle half takes 0.2 s per seq on the CPU (262145 nodes
    filtered and scored per call; 0.4 s to load them), 13 s for 64 seqs: cut to 20 seqs, 4.5 s."""
    _select(xu.SELECT_BIG, ("boundary",), range(20))


# ---------------------------------------------------------------------------------------------------------------------
# refusals: each by its message; the context stays usable and the next pod matches the oracle

def _next_pod_matches(e, o, case, j, seq=77):
    d = xu.rows_equal(e.ext_rows(case.pods[j], case.ext[j], seq), o.ext_rows(case.pods[j], case.ext[j], seq))
    assert d is None, d
    s = np.array([seq], np.uint64)
    g, w = e.schedule_ext(case.pods[j:j + 1], case.ext[j:j + 1], s), o.schedule_ext(case.pods[j:j + 1], case.ext[j:j + 1], s)
    for f in ("node", "feasible", "score", "ties"):
        assert g[0][f][0] == w[0][f][0], f
    # (Reserve flags: the oracle's schedule_ext reports the NUMA / cpuset bits, not the affinity hint)
    reserve = abi.GS_PLACED_NUMA | abi.GS_PLACED_CPUSET
    assert g[0]["flags"][0] & reserve == w[0]["flags"][0] & reserve
    assert g[1].tobytes() == w[1].tobytes() and w[0]["node"][0] >= 0
    assert e.mirror_check() == 0


def test_nine_matched_reservations_on_a_node_refused():
    from koordinator_amd.engine import GpuScoreError
    rs = [xu.rsv(0xE000 + k, 1, 5, {0: 1000, 1: xu.GiB}) for k in range(9)]
    rs += [xu.rsv(0xE100 + k, 2, 6, {0: 1000, 1: xu.GiB}) for k in range(8)]
    nodes = xu.base_nodes(16)
    xu.hold(nodes, rs)
    c2 = {0: 500, 1: xu.GiB}
    case = xu.Case("nine", nodes, np.zeros(16, abi.NODE_DEVICES_DTYPE), xu.pod_records([c2] * 3, 0xDC0000),
                   xu.ext_records(owner=[1, 2, 2], required=[1, 1, 0]), xu.ext_args(),
                   reservations=np.array(rs, abi.RESERVATION_DTYPE))
    e, o = _engine(case), case.oracle()
    for call in (lambda: e.ext_rows(case.pods[0], case.ext[0], 0),
                 lambda: e.schedule_ext(case.pods[:1], case.ext[:1], np.zeros(1, np.uint64))):
        with pytest.raises(GpuScoreError, match="more than 8 matched reservations on node 5"):
            call()
    _next_pod_matches(e, o, case, 1)     # eight pass
    _next_pod_matches(e, o, case, 2)


def test_gpu_on_a_foreign_numa_node_refused():
    from koordinator_amd.engine import GpuScoreError
    zone = (8000, 32 * xu.GiB)
    numa_nodes = tuple(nu.Node(f"n{i}", "Restricted", (zone, zone)) for i in range(4))
    devs = np.array([xu.device([xu.gpu(numa=g % 2) for g in range(4)]) for _ in range(4)], abi.NODE_DEVICES_DTYPE)
    bad = devs.copy()
    bad[2]["gpus"][1]["numa_node"] = 5     # none of the node's zones 0, 1
    case = xu.Case("foreign", np.zeros(4, abi.NODE_DTYPE), bad, xu.pod_records([{0: 2000, 1: 4 * xu.GiB}] * 2, 0xDD0000),
                   xu.ext_records(gpu=[{xu.KG: 100}, {xu.KG: 200}]), xu.ext_args(weights=(1, 1, 1)),
                   enabled=xu.FIT | abi.GS_ENABLE_NUMA_FILTER | abi.GS_ENABLE_NUMA_SCORE, numa_nodes=numa_nodes)
    e, o = _engine(case), case.oracle()
    for call in (lambda: e.ext_rows(case.pods[0], case.ext[0], 0),
                 lambda: e.schedule_ext(case.pods[:1], case.ext[:1], np.zeros(1, np.uint64))):
        with pytest.raises(GpuScoreError, match="a GPU's NUMA node is not one of its node's NUMA zones"):
            call()
    assert e.mirror_check() == 0 and all(e.ext_reserved(int(u)) is None for u in case.pods["uid"])
    for x in (e, o):                        # the Device object corrected: the same pods go through
        x.upsert_devices(devs[2:3], np.array([2], np.uint32))
    _next_pod_matches(e, o, case, 0)
    _next_pod_matches(e, o, case, 1)


def test_minor_and_quantity_ranges_refused():
    from koordinator_amd.engine import GpuScoreError
    case = xu.ds_case()
    e, o = _engine(case), case.oracle()
    one = np.array([2], np.uint32)
    for dev, msg in ((xu.device([xu.gpu(minor=32)]), "GPU minor outside 0..31"),
                     (xu.device([xu.gpu(minor=-1)]), "GPU minor outside 0..31"),
                     (xu.device([xu.gpu(total=(100, 100, 1 << 53))]), r"GPU quantity outside \[0, 2\^53\)"),
                     (xu.device([xu.gpu(used=(-1, 0, 0))]), r"GPU quantity outside \[0, 2\^53\)")):
        with pytest.raises(GpuScoreError, match=msg):
            e.upsert_devices(np.array([dev], abi.NODE_DEVICES_DTYPE), one)
    e.upsert_devices(np.array([xu.device([xu.gpu(minor=31, total=(100, 100, (1 << 53) - 1))])], abi.NODE_DEVICES_DTYPE), one)
    e.upsert_devices(case.devices[2:3], one)
    for r, msg in ((xu.rsv(1, 1, 0, {1: 1 << 50}), r"reservation quantity outside \[0, 2\^50\)"),
                   (xu.rsv(1, 1, 0, {1: 8}, allocated={1: 1 << 50}), r"reservation quantity outside \[0, 2\^50\)"),
                   (xu.rsv(1, 1, 0, {7: 8}), "reservation resource keys outside slots 0..6")):
        with pytest.raises(GpuScoreError, match=msg):
            e.upsert_reservations(np.array([r], abi.RESERVATION_DTYPE))
    assert e.reservation(1) is None
    j = case.pod_names.index("koord100")
    _next_pod_matches(e, o, case, j)
