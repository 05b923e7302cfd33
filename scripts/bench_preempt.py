"""Cost of the ElasticQuota PostFilter dry run (gs_preempt_dry_run) on one GPU: the C3 cluster of bench.py (50k nodes,
NodeNUMAResource profile), ~30 resident pods per node, 1 / 16 / 128 quota-rejected preemptors per call (row = -1: every
node is potential, the worst case). Prints one JSON line. Run: python scripts/bench_preempt.py [--calls 10]

Per preemptor count: wall time per call with the table unchanged (median), per call after a change to 64 nodes' lists
(the incremental upload: the difference is the upload share), and once after the table's first load (the whole image).
table_device_bytes: 160 B per record slot of the pool (segments of 8 .. 128 records) + 8 B per node.
cpu_estimate: the same dry run by the oracle-backed restatement (tests/preempt_util.py) on a --sample-nodes node
sample of the same cluster, scaled by nodes / sample: an ESTIMATE, marked as such.

  --only N   N preemptors per call only, no CPU estimate, for a profiler:
             rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_preempt.py --only 16 --calls 5
             (preempt_nodes_kernel<...> and preempt_pick_kernel are the dry run's kernels)
  --pdbs K   the cost of PodDisruptionBudgets instead: K PDBs with budgets 0 / 1 / 2 in turn, every resident in 0-2
             of them; gs_preempt_dry_run_pdb and gs_preempt_dry_run on the same table, alternating in one session.
             Prints ms per call of both (min / median / max over --calls) and the share of candidate nodes with a
             non-empty violating group. With --only N under rocprofv3: preempt_partition_kernel,
             preempt_nodes_pdb_kernel<...> and preempt_pick_pdb_kernel are the new call's kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--residents", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--sample-nodes", type=int, default=500)
    ap.add_argument("--pdbs", type=int, default=0)
    args = ap.parse_args()

    from koordinator_amd import abi, config, synth
    from koordinator_amd.engine import Engine
    from tests import preempt_util as pu

    N = args.nodes
    cluster = synth.make_cluster(N, 256, config_id=2)
    synth.make_numa(cluster)
    cluster.nodes["pod_count"] = np.maximum(cluster.nodes["pod_count"], args.residents + 8)
    cfg = config.make_config(N, enabled=abi.GS_ENABLE_ALL)
    s = np.random.RandomState(1)
    counts = np.clip(args.residents + s.randint(-8, 9, N), 0, abi.GS_MAX_NODE_PODS)
    node_idx, res = pu.make_residents(cluster, counts, 41)
    used = pu.quota_used(res)

    def preemptors(n):
        pre = []
        for k in range(n):
            p = cluster.pods[k].copy()
            if p["requests"][0] == 0:
                p["requests"][0] = p["nonzero_requests"][0] = 2000
                p["request_mask"] |= 3
            pre.append(pu.make_preemptor(p, -1, used, used + p["requests"][:2] - np.array([4000, 0])))
        return np.stack(pre)

    eng = Engine(cfg)
    synth.load_into(eng, cluster)
    t0 = time.perf_counter()
    eng.node_pods_add(node_idx, res)
    t_add = time.perf_counter() - t0
    slots = int(sum(max(8, 1 << int(np.ceil(np.log2(max(int(c), 1))))) for c in counts.tolist() if c))
    out = {"what": "gs_preempt_dry_run", "nodes": N, "residents": int(len(res)), "table_add_s": round(t_add, 3),
           "table_device_bytes": slots * 160 + 8 * N, "per_call": {}}
    if args.pdbs:
        out = pdb_cost(eng, args, node_idx, res, preemptors, out)
        eng.close()
        print(json.dumps(out))
        return
    first = True
    churn = s.permutation(N)[:64]
    for n in ([args.only] if args.only else [1, 16, 128]):
        pre = preemptors(n)
        t0 = time.perf_counter()
        r, _, _ = eng.preempt_dry_run(pre, None, detail=False)
        t_first = time.perf_counter() - t0
        steady, changed = [], []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            eng.preempt_dry_run(pre, None, detail=False)
            steady.append(time.perf_counter() - t0)
        for _ in range(args.calls):
            m = np.nonzero(np.isin(node_idx, churn))[0]
            m = m[np.unique(node_idx[m], return_index=True)[1]]   # one resident of each of the 64 nodes
            eng.node_pods_remove(node_idx[m], res["uid"][m])
            eng.node_pods_add(node_idx[m], res[m])
            t0 = time.perf_counter()
            eng.preempt_dry_run(pre, None, detail=False)
            changed.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        eng.preempt_dry_run(pre, None, detail=True)
        t_detail = time.perf_counter() - t0
        e = {"ms_per_call": round(1e3 * float(np.median(steady)), 3),
             "ms_per_call_after_64_node_change": round(1e3 * float(np.median(changed)), 3),
             "ms_with_detail_readback": round(1e3 * t_detail, 3),
             "nominated": int((r["status"] == abi.GS_PREEMPT_NOMINATED).sum()),
             "candidates_mean": float(r["num_candidates"].mean()), "errors_mean": float(r["num_errors"].mean())}
        e["upload_share"] = round(max(0.0, 1.0 - e["ms_per_call"] / max(e["ms_per_call_after_64_node_change"], 1e-9)), 3)
        if first:
            e["ms_first_call_with_whole_image_upload"] = round(1e3 * t_first, 3)
            first = False
        out["per_call"][str(n)] = e
    eng.close()

    if not args.only:   # the restatement over the CPU oracle on a node sample, scaled
        from oracle import oracle as orc
        from tests import fit_diag_util as fd
        S = args.sample_nodes
        sub = synth.make_cluster(S, 256, config_id=2)
        synth.make_numa(sub)
        sub.nodes["pod_count"] = np.maximum(sub.nodes["pod_count"], args.residents + 8)
        ni, rs = pu.make_residents(sub, np.clip(args.residents + s.randint(-8, 9, S), 0, 128), 41)
        o = orc.Oracle(fd.make_cfg(sub, True))
        synth.load_into(o, sub)
        table = pu.Table(S)
        table.add(ni, rs)
        u = pu.quota_used(rs)
        p = sub.pods[1].copy()
        pre1 = pu.make_preemptor(p, -1, u, u + p["requests"][:2] - np.array([4000, 0]))
        t0 = time.perf_counter()
        pu.dry_run(o, sub.nodes, table, pre1)
        dt = time.perf_counter() - t0
        o.close()
        out["cpu_estimate"] = {"estimate": True, "sample_nodes": S, "s_per_preemptor_on_sample": round(dt, 3),
                               "s_per_preemptor_scaled": round(dt * N / S, 2),
                               "note": "Python restatement over the oracle's Filter, scaled by nodes / sample"}
    print(json.dumps(out))


def pdb_cost(eng, args, node_idx, res, preemptors, out):
    """gs_preempt_dry_run_pdb against gs_preempt_dry_run on the same table, alternating."""
    from koordinator_amd import abi
    s = np.random.RandomState(2)
    K, M = args.pdbs, len(res)
    ids = np.full((M, abi.GS_MAX_POD_PDBS), abi.GS_PDB_NONE, np.uint16)
    n = s.randint(0, 3, M)
    a, b = s.randint(0, K, M), s.randint(0, K - 1, M)
    b = np.where(b >= a, b + 1, b)                      # distinct from a
    ids[n >= 1, 0] = a[n >= 1]
    ids[n >= 2, 1] = b[n >= 2]
    t0 = time.perf_counter()
    eng.node_pods_set_pdbs(node_idx, res["uid"], ids)
    eng.pdbs_upsert(np.arange(K, dtype=np.uint32), (np.arange(K) % 3).astype(np.int32))
    out.update({"what": "gs_preempt_dry_run_pdb vs gs_preempt_dry_run", "pdbs": K, "memberships_per_resident": "0-2",
                "budgets": "0 / 1 / 2 in turn", "set_lists_and_budgets_s": round(time.perf_counter() - t0, 3)})

    def stat(ts):
        return {"min": round(1e3 * min(ts), 3), "median": round(1e3 * float(np.median(ts)), 3), "max": round(1e3 * max(ts), 3)}
    for n in ([args.only] if args.only else [1, 16, 128]):
        pre = preemptors(n)
        r, status, _, viol, nviol = eng.preempt_dry_run_pdb(pre, None, detail=True)    # (the first call uploads)
        eng.preempt_dry_run(pre, None, detail=False)
        cand = status == abi.GS_PNODE_CANDIDATE
        t_old, t_new = [], []
        for i in range(args.calls):
            for which in ((0, 1) if i % 2 == 0 else (1, 0)):
                t0 = time.perf_counter()
                if which:
                    eng.preempt_dry_run_pdb(pre, None, detail=False)
                else:
                    eng.preempt_dry_run(pre, None, detail=False)
                (t_new if which else t_old).append(time.perf_counter() - t0)
        out["per_call"][str(n)] = {
            "ms_per_call_without_pdbs": stat(t_old), "ms_per_call_with_pdbs": stat(t_new),
            "candidates_mean": float(r["num_candidates"].mean()),
            "share_of_candidates_with_violating_group": round(float((cand & viol.any(axis=2)).sum() / max(cand.sum(), 1)), 3),
            "share_of_candidates_with_violations": round(float((cand & (nviol > 0)).sum() / max(cand.sum(), 1)), 3),
            "nominated": int((r["status"] == abi.GS_PREEMPT_NOMINATED).sum())}
    return out


if __name__ == "__main__":
    main()
