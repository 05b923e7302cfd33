"""The speculative commit's edge inputs reach their edges: asserted on the CPU oracle alone (commit_edges_util.classify),
so that tests/test_gpu_commit_edges.py cannot pass vacuously. Conditions on the inputs, pod by pod; no shares."""
import numpy as np
import pytest

from tests import commit_edges_util as ce

CASES = dict(ce.all_cases())


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_edges(name):
    case = CASES[name]()
    recs = ce.classify(case)
    assert len(recs) == len(case.pods)
    ce.check_claims(case, recs)
    if case.slowpath is not None:
        assert sum(r["full_row"] for r in recs) == case.slowpath


def test_tiebreak_restatement_is_the_oracles():
    """the seq search's tiebreak_position against the oracle's selectHost: 300 identical nodes, every pod's node is
    the tie at the restated position"""
    c = ce.flat(300, {})
    pods = ce.pods_of(c, [ce.STEP] * 64)
    seq = np.arange(7, 7 + 64, dtype=np.uint64)
    case = ce.Case("ties", c, pods, seq, 64, None, [])
    case.want = case.oracle().schedule(pods, seq)
    recs = ce.classify(case)
    assert [r["T"] for r in recs][:3] == [300, 299, 298] and all(r["jp"] >= 1 for r in recs)


def test_chain_lengths_cover_the_undo_log_and_job_ring():
    short, long_ = CASES["chains-short"](), CASES["chains-long"]()
    runs = []
    for case in (short, long_):
        nodes = case.want["node"].tolist()
        q = 0
        while q < len(nodes):
            r = 1
            while q + r < len(nodes) and nodes[q + r] == nodes[q]:
                r += 1
            runs.append(r)
            q += r
    assert [r for r in runs if r > 1] == [2, 3, ce.SP_LAG - 1, ce.SP_LAG, ce.SP_LAG + 1, ce.SP_JOBQ + 1, 64, 127]


def test_paths_cross_the_winner_path_switches():
    """nold passes 58 -> 59 (the prep wave's 61 - 3) and 61 -> 62 inside one batch of 128, with the tie-break position
    at both ends of the ties on either side"""
    recs = ce.classify(CASES["paths-130"]())
    for q in (58, 59, 61, 62):
        assert recs[q]["nold"] == q and recs[q]["nnew"] == 0 and recs[q]["listed"]
    assert {recs[q]["jp"] for q in (57, 61)} == {1}
    assert all(recs[q]["jp"] == recs[q]["T"] for q in (58, 62))
    assert max(r["e"] for r in recs if r["e"] is not None) >= 64


@pytest.mark.parametrize("batch", [31, 32, 33, 64, 128])
def test_chains_span_batch_boundaries(batch):
    """the long chains at the batch sizes of the GPU test: the oracle's rows are consistent at every boundary, and a
    pod at position 0 of a batch continues a chain begun in the previous one (its winner is no dirty row of its batch)"""
    case = CASES["chains-long"]()
    recs = ce.classify(case, batch)
    heads = [q for q in range(batch, len(recs), batch) if case.want["node"][q] == case.want["node"][q - 1]]
    assert heads and all(recs[q]["fresh"] and recs[q]["nd"] == 0 for q in heads)


def test_hash_collisions_from_the_expression():
    case = CASES["hash"]()
    landed = sorted(set(case.want["node"][:ce.HASH_A + ce.HASH_Z].tolist()))
    assert len(landed) == ce.HASH_A + 1 >= 100 and {ce.sp_hash(n) for n in landed} == {ce.sp_hash(ce.HASH_C)}
