"""The inputs of tests/test_gpu_ext_edges.py reach the edges they claim (tests/ext_edges_util.py's docstring names the
lines of koordinator_amd/csrc/gs_ext.hip they are aimed at), shown on the oracle alone, and ext_edges_util's integer
restatement of the reference's arithmetic equals the oracle on every pair and case. No GPU.

Every condition is read off the oracle's per-node rows (Oracle.ext_rows); the restatement (py_device_pair,
py_score_reservation, py_totals) is written from the reference's Go text and is held against those rows here, so a
change to the oracle's float64 floor, its truncating divisions or its normalization shows up without a GPU.
Run with -s for the measured shares.

Left out: a byte request on a GPU whose memory total is 0 (memoryBytesToRatio divides by zero in the reference,
devicehandler_gpu.go:96); the mem0 nodes see ratio requests only.
"""
import collections

import numpy as np
import pytest

from koordinator_amd import abi
from tests import ext_edges_util as xu


def _ds_rows(strategy="LeastAllocated", weights=(0, 1, 0), ignored=0, variant="default"):
    return xu.ds_case(strategy, weights, ignored), xu.oracle_rows("ds", strategy, weights, ignored, variant)


def _pair(case, rows, pod, node):
    r = rows[case.pod_names.index(pod)][0]
    i = case.node_names.index(node)
    return bool(r["feasible"][i]), int(r["ds_raw"][i])


# ---------------------------------------------------------------------------------------------------------------------
# the restatement equals the oracle

@pytest.mark.parametrize("key", [k for k in xu.stateless_keys() if k[0] in ("ds", "mem0")], ids=str)
def test_device_restatement_equals_oracle_on_every_pair(key):
    case = xu.case_of(*key[:-1])
    args = xu.variant_args(case.args, dict(xu.VARIANTS)[key[-1]])
    rows = xu.oracle_rows(*key)
    assert len(case.pods) <= 48 and case.n <= 96
    for j, (r,) in enumerate(rows):
        pairs = [xu.py_device_pair(case.devices[i], case.ext[j], args) for i in range(case.n)]
        if pairs[0] is None:
            assert all(p is None for p in pairs) and r["fail_code"] == abi.GS_EXT_FAIL_POD and r["node"] == -1
            assert not r["feasible"].any()
            continue
        assert r["fail_code"] == 0
        want_f = np.array([p[0] for p in pairs])
        want_s = np.array([p[1] if p[0] else 0 for p in pairs])
        assert np.array_equal(r["feasible"].astype(bool), want_f), (case.pod_names[j], np.nonzero(r["feasible"] != want_f))
        assert np.array_equal(r["ds_raw"], want_s), (case.pod_names[j], np.nonzero(r["ds_raw"] != want_s))
        assert np.array_equal(xu.py_totals(r, args), r["total"]), case.pod_names[j]


@pytest.mark.parametrize("key", [k for k in xu.stateless_keys() if k[0] in ("rsv", "wide", "policy")], ids=str)
def test_reservation_scores_and_totals_restated(key):
    case = xu.case_of(*key[:-1])
    args = xu.variant_args(case.args, dict(xu.VARIANTS)[key[-1]])
    rows = xu.oracle_rows(*key)
    by_uid = {int(r["uid"]): r for r in case.reservations}
    rs_on = bool(args.enabled & abi.GS_EXT_RESERVATION)
    for j, (r,) in enumerate(rows):
        for i in np.nonzero(r["nominated_uid"])[0]:
            x = by_uid[int(r["nominated_uid"][i])]
            assert rs_on and int(x["node"]) == i and r["feasible"][i]
            assert int(r["rs_raw"][i]) == xu.py_score_reservation(case.pods[j], x), (j, i)
        assert not r["rs_raw"][r["nominated_uid"] == 0].any()
        assert np.array_equal(xu.py_totals(r, args), r["total"]), j
        if r["node"] >= 0:
            mx = r["total"].max()
            assert r["score"] == mx and r["ties"] == (r["total"] == mx).sum() and r["total"][r["node"]] == mx
            assert r["feasible_count"] == r["feasible"].sum()


# ---------------------------------------------------------------------------------------------------------------------
# the DeviceShare conditions

def test_deviceshare_conditions_reached():
    case, rows = _ds_rows()
    P = lambda pod, node: _pair(case, rows, pod, node)   # noqa: E731
    gpu_pods = [p for p, g in zip(case.pod_names, xu.ds_pods()) if g[1] and all(g[1].values())
                and rows[case.pod_names.index(p)][0]["fail_code"] == 0]   # (a request of 0 passes Fit anywhere)
    assert len(gpu_pods) >= 30
    for p in gpu_pods:
        assert P(p, "nodev-noalloc") == (False, 0) and P(p, "nodev-alloc") == (True, 0)
        for node in ("gpus0", "noinfo", "zerotot", "full"):
            assert P(p, node) == (False, 0), (p, node)
    assert P("plain", "nodev-noalloc")[0] and P("plain", "full")[0]
    # the first healthy GPU sets the per-instance memory
    assert P("koord100", "first-zero")[0] and P("nvidia2", "first-zero")[0]
    assert P("bytes58G", "eight")[0] and not P("bytes58G", "first-40")[0]      # 58 / 40 GiB: ratio 145
    assert P("bytes40G", "first-40")[0] and P("bytes40G", "first-40")[1] != P("bytes40G", "eight")[1]
    # counts at and above the GPU count
    assert P("nvidia1", "one")[0] and not P("nvidia2", "one")[0]
    assert P("nvidia8", "eight")[0] and P("koord800", "eight")[0]
    nine = rows[case.pod_names.index("nvidia9")][0]["feasible"]   # 9 GPUs fit no Device object, only a node without one
    assert [case.node_names[i] for i in np.nonzero(nine)[0]] == ["nodev-alloc"]
    assert P("koord200", "count2")[0] and not P("koord200", "count1")[0]
    assert not P("nvidia8", "count7")[0] and P("ratio400", "gaps")[0] and not P("core50-ratio300", "gaps-used")[0]
    assert P("koord100", "minors")[0] and P("core50-ratio50", "over")[0] and not P("koord100", "over")[0]
    assert not P("ratio1", "onekey")[0] and not P("bytes1", "onekey")[0]
    # free equal to the per-instance request, and one short on each key
    assert P("core50-ratio50", "exact")[0] and P("core50-bytes40G", "exact")[0]
    for node in ("short-core", "short-ratio", "short-mem"):
        assert not P("core50-ratio50", node)[0] and not P("core50-bytes40G", node)[0], node
    assert P("ratio50", "short-core")[0] and not P("ratio50", "short-ratio")[0] and not P("ratio50", "short-mem")[0]
    # int64(float64(bytes) / float64(total) * 100): 29, 57, 58 GiB of 100 GiB are ratio 28, 56, 57
    assert int(float(29 * xu.GiB) / float(100 * xu.GiB) * 100) == 28
    assert P("bytes29G", "t100-r28")[0] and not P("bytes29G", "t100-r27")[0]
    assert P("bytes57G", "t100-r56")[0] and not P("bytes57G", "t100-r55")[0]
    assert P("bytes58G", "t100")[0] and not P("bytes58G", "t100-r56")[0]
    assert P("bytes100G", "t100")[0] and not P("bytes100G", "eight")[0]        # 125 on 80 GiB
    assert P("bytes200G", "t100")[0] and not P("bytes200G", "eight")[0]        # 2 x 100 GiB; 250 on 80 GiB
    assert P("bytes160G", "eight")[0] and not P("bytes120G", "eight")[0] and not P("bytes120G", "t100")[0]
    # ratio * total / 100 floors on a total that 100 does not divide
    assert (80 * xu.GiB + 7) * 50 % 100 != 0 and P("ratio50", "odd-total")[0] and P("core50-ratio50", "odd-total-free")[0]
    # Fit's GPU-name scalars
    assert P("koord50", "fit-exact")[0] and not P("koord50", "fit-short")[0] and not P("koord1", "fit-neg")[0]
    assert P("nvidia2", "fit-nv-exact")[0] and not P("nvidia2", "fit-nv-short")[0] and P("nvidia1", "fit-nv-short")[0]
    icase, irows = _ds_rows(ignored=xu.IGNORE_KOORD)
    for node in ("fit-exact", "fit-short", "fit-neg"):
        assert _pair(icase, irows, "koord50", node)[0], node
    assert not _pair(icase, irows, "nvidia2", "fit-nv-short")[0]
    ncase, nrows = _ds_rows("MostAllocated", (1, 1, 1), 1 << xu.NV, "coprime")
    assert _pair(ncase, nrows, "nvidia2", "fit-nv-short")[0] and not _pair(ncase, nrows, "koord50", "fit-short")[0]
    # PreFilter failures
    for p in ("invalid150", "invalid250", "bad-nv-koord", "bad-core", "bad-core-ratio-mem", "bad-mem-ratio", "bad-nv-ratio"):
        assert rows[case.pod_names.index(p)][0]["fail_code"] == abi.GS_EXT_FAIL_POD, p
    # a masked request of 0 is a GPU pod: the Filter runs (no GPU passes on `full`), the score counts no request
    assert P("ratio0", "eight") == (True, 100) and not P("ratio0", "full")[0]
    # memory total 0: ratio requests pass, the byte keys are 0
    mcase = xu.ds_mem0_case()
    mrows = xu.oracle_rows("mem0", "LeastAllocated", "default")
    assert all(xu.ME not in g for _, g in xu.ds_pods() if _ in mcase.pod_names)
    assert _pair(mcase, mrows, "koord100", "mem0")[0] and _pair(mcase, mrows, "ratio50", "mem0-used")[0]
    assert not _pair(mcase, mrows, "koord100", "mem0-used")[0]


@pytest.mark.parametrize("strategy", xu.STRATEGIES)
@pytest.mark.parametrize("weights", xu.WEIGHTS, ids=str)
def test_deviceshare_shares(strategy, weights):
    case, rows = _ds_rows(strategy, weights)
    feas = tot = 0
    vals = collections.Counter()
    zero_mds = inexact = 0
    for (r,) in rows:
        if r["fail_code"]:
            continue
        tot += case.n
        feas += int(r["feasible"].sum())
        vals.update(r["ds_raw"][r["feasible"] != 0].tolist())
        if r["node"] >= 0:
            mds = int(r["ds_raw"][r["feasible"] != 0].max())
            zero_mds += mds == 0
            inexact += mds > 0 and any(100 * int(v) % mds for v in r["ds_raw"][r["feasible"] != 0])
    print(f"{strategy} {weights}: feasible {feas}/{tot} = {feas / tot:.2f}, {len(vals)} raw scores, MDS == 0 on "
          f"{zero_mds} pods, inexact 100 * ds / MDS on {inexact}")
    assert 0.2 <= feas / tot <= 0.8
    assert len(vals) >= 12 and 0 in vals and 100 in vals
    assert zero_mds >= 1 and inexact >= 5      # (the plain pod scores 0 everywhere)


def test_policy_nodes_reach_the_hint_edges():
    case = xu.policy_case()
    rows = xu.oracle_rows("policy", "default")
    assert case.n <= 48 and len(case.pods) == 16
    zone_of = lambda d: {int(g["numa_node"]) for g in d["gpus"][:int(d["num_gpus"])] if g["has_info"]}   # noqa: E731
    for i, nd in enumerate(case.numa_nodes):   # every GPU with a topology is on one of its node's zones
        assert zone_of(case.devices[i]) <= set(range(len(nd.zones))) | {-1}, nd.name
    feas = np.array([r["feasible"] for (r,) in rows])
    assert 0.2 <= feas.mean() <= 0.8
    for j in range(len(case.pods)):            # every count is feasible somewhere and refused somewhere
        assert feas[j].any() and not feas[j].all(), case.pod_names[j]
    # the affinity decides: a pair the Filter without affinity passes is refused on a policy node
    off = [xu.py_device_pair(case.devices[i], case.ext[j], case.args)[0] for j in range(len(case.pods)) for i in range(case.n)]
    assert (np.array(off).reshape(feas.shape) & ~feas.astype(bool)).sum() >= 20
    kinds = collections.Counter(n.rsplit("-", 1)[1] for n, f in zip(case.node_names, feas.any(axis=0)) if f)
    assert set(kinds) == {"onezone", "split", "notopo", "gaps"}


# ---------------------------------------------------------------------------------------------------------------------
# the reservation conditions

def test_reservation_conditions_reached():
    case = xu.rsv_case()
    rows = {n: r for n, (r,) in zip(case.pod_names, xu.oracle_rows("rsv", True, "default"))}
    assert case.n <= 64 and len(case.pods) <= 40
    by_uid = {int(r["uid"]): r for r in case.reservations}
    nom = lambda pod, node: int(rows[pod]["nominated_uid"][node])   # noqa: E731
    pol = lambda pod, node: int(by_uid[nom(pod, node)]["allocate_policy"])   # noqa: E731
    assert pol("default", 1) == abi.RSV_POLICY["Default"] and pol("aligned", 2) == abi.RSV_POLICY["Aligned"]
    assert pol("restricted-eq", 3) == abi.RSV_POLICY["Restricted"] and rows["restricted-eq"]["rs_raw"][3] == 100
    assert rows["restricted-eq"]["feasible_count"] == 1
    for p in ("restricted-cpu+1", "restricted-mem+1"):     # one more than the remainder: the only matched node fails
        assert rows[p]["node"] == -1 and rows[p]["feasible_count"] == 0
    # slots 3-6 on the pod and the reservation
    assert rows["slots"]["feasible_count"] == 3 and nom("slots", 4) and rows["slots+1"]["feasible_count"] == 2
    assert not rows["slots+1"]["feasible"][4] and rows["slots-mid"]["feasible"][4] and not rows["slots-mid"]["feasible"][5]
    # a names mask disjoint from the pod's
    assert rows["disjoint-cpu"]["node"] == -1 and rows["disjoint-mem"]["feasible_count"] == 1
    assert rows["disjoint-free"]["feasible"][7] and not nom("disjoint-free", 7)
    # allocated above allocatable, req > alloc in one slot, zero allocatable entries
    assert nom("over", 9) and rows["over"]["rs_raw"][9] == 0 and not rows["over-req"]["feasible"][10]
    assert nom("reqgt", 11) and 0 < rows["reqgt"]["rs_raw"][11] < 50
    assert nom("zeroalloc", 12) and nom("zeroalloc", 13) and rows["zeroalloc"]["rs_raw"][13] == 0
    # 1, 2 and 8 matched reservations on a node
    per_node = collections.Counter((int(r["owner_key"]), int(r["node"])) for r in case.reservations)
    assert {per_node[xu.O_DEFAULT, 1], per_node[xu.O_TWO, 14], per_node[xu.O_EIGHT, 15]} == {1, 2, 8}
    assert nom("two", 14) and nom("eight", 15) and nom("eight-free", 15)
    # every reservation allocate-once-used / unschedulable: nothing matches
    assert rows["once-req"]["node"] == -1 and rows["unsched-req"]["node"] == -1 and not rows["once"]["nominated_uid"].any()
    # nomination by order (the first of two equal orders) and by score (the first of equal scores)
    o18 = sorted((int(r["uid"]), int(r["order"])) for r in case.reservations if r["node"] == 18)
    assert nom("order", 18) == next(u for u, o in o18 if o == 3) and rows["order"]["pref_node"] == 18
    s19 = [(xu.py_score_reservation(case.pods[case.pod_names.index("score")], r), int(r["uid"]))
           for r in case.reservations if r["node"] == 19]
    assert nom("score", 19) == max(s19)[1] and len({s for s, _ in s19}) == 3
    assert nom("eqscore", 20) == min(int(r["uid"]) for r in case.reservations if r["node"] == 20)
    # orders: 0 counts as none, equal lowest on two nodes (the first node), lowest on an infeasible node
    assert rows["order2"]["pref_node"] == 21 and rows["order2"]["node"] == 21 and rows["order2"]["feasible"][22]
    assert not rows["orderbad"]["feasible"][25] and rows["orderbad"]["pref_node"] == 26
    assert rows["score"]["pref_node"] == -1
    # owners: required / not, without a reservation, a GPU owner pod nominates none
    assert rows["none-req"]["node"] == -1 and rows["none"]["feasible_count"] == rows["no-owner"]["feasible_count"] > 50
    for p in ("gpu-owner", "gpu-owner-req"):
        assert rows[p]["node"] >= 0 and not rows[p]["nominated_uid"].any()
    assert rows["gpu-owner-req"]["feasible_count"] == 4
    assert rows["q46"]["feasible_count"] == 2 and nom("q46", 42) and not rows["q46+1"]["nominated_uid"][41] == 0
    # the pod-count term of fitsNode decides once Fit's own Filter is off: at allowed_pods, one below, one above
    nofit = {n: r for n, (r,) in zip(case.pod_names, xu.oracle_rows("rsv", False, "default"))}
    assert nofit["pods"]["feasible"][28:31].tolist() == [1, 1, 0] and nofit["pods-zero"]["feasible"][28:31].tolist() == [1, 1, 0]
    assert nofit["pods-free"]["feasible"][28:31].all() and not nofit["pods-free"]["nominated_uid"][30]
    # the preferred node's 1000 against the others' 100 * r / 1000
    r = rows["order2"]
    others = [i for i in np.nonzero(r["rs_raw"])[0] if i != r["pref_node"]]
    assert others and all(100 * int(r["rs_raw"][i]) // 1000 < 100 for i in others)


@pytest.mark.parametrize("nrec", xu.WIDE_NREC)
def test_wide_owner_reaches_the_record_stride(nrec):
    case = xu.rsv_wide_case(nrec)
    rows = {n: r for n, (r,) in zip(case.pod_names, xu.oracle_rows("wide", nrec, "default"))}
    assert case.n == xu.N_WIDE
    assert (rows["wide-req"]["nominated_uid"] != 0).sum() == nrec - 1          # node 250 has no room
    assert (rows["wide2-req"]["nominated_uid"] != 0).sum() == nrec
    # equal lowest orders: the first node; the lowest order of all on an infeasible node; on the last record alone
    assert not rows["wide"]["feasible"][250] and rows["wide"]["pref_node"] == 6
    assert rows["wide2"]["pref_node"] == nrec - 1 == rows["wide2"]["node"]


# ---------------------------------------------------------------------------------------------------------------------
# the select shapes

def _picks(n, shape):
    c = xu.select_case(n, shape)
    o = c.oracle()
    return [o.ext_rows(c.pods[0], c.ext[0], s) for s in xu.SEQS]


@pytest.mark.parametrize("n", xu.SELECT_N)
def test_select_shapes(n):
    for shape in xu.SELECT_SHAPES:
        ties = xu.select_ties(n, shape)
        rows = _picks(n, shape)
        for r in rows:
            assert r["ties"] == len(ties) and (r["node"] in ties if ties else r["node"] == -1), (shape, r["node"])
            assert r["feasible_count"] == (0 if shape == "none" else 1 if shape == "last-only" else n)
        picks = [r["node"] for r in rows]
        if shape == "boundary":    # every tie rank is chosen at least once
            assert set(picks) == set(ties), (n, sorted(set(ties) - set(picks)))
        if shape == "all-tie" and n >= 2049:
            blocks = collections.defaultdict(set)
            for p in picks:
                blocks[p // 1024].add(p % 1024 // 256)
            last_full = n // 1024 - 1
            assert 0 in blocks and last_full in blocks and max(len(v) for v in blocks.values()) >= 3, dict(blocks)
        if shape == "last-block" and n > 1024:
            assert min(picks) >= (n - 1) // 1024 * 1024
