"""Cost of the top-N score tables on one GPU: the C3 workload of bench.py (50k nodes, NodeNUMAResource profile, 2048
pods per step submitted one step ahead) through gs_schedule_submit_top_scores at topn 8 and 64, beside the same run
through gs_schedule_submit. Prints one JSON line. Run: python scripts/bench_top_scores.py [--steps 20]

  --host-timing   one more run per topn under GS_HOST_TIMING=1: the library prints, on stderr, the host time per batch
                  spent deriving landed-row versions, in the landed pass and in the merge
  --only N        the run at topn N only, for a profiler:
                  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_top_scores.py --only 8 --steps 5
                  (top_scores_kernel and top_scores_landed_kernel are the feature's kernels)"""
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
    ap.add_argument("--pods-per-step", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-timing", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    args = ap.parse_args()

    from koordinator_amd import abi, config, synth
    from koordinator_amd.engine import Engine

    P, total = args.pods_per_step, (args.warmup + args.steps) * args.pods_per_step
    cluster = synth.make_cluster(args.nodes, total, config_id=2)
    synth.make_numa(cluster)
    cfg = config.make_config(args.nodes, enabled=abi.GS_ENABLE_ALL)
    w = np.array([cfg.plugin_weights[k] for k in range(abi.GS_NUM_PLUGINS)], np.int64)
    seq = np.arange(total, dtype=np.uint64)
    pods = cluster.pods

    def run(topn: int):
        eng = Engine(cfg)
        synth.load_into(eng, cluster)
        if topn:
            submit = lambda p, q: eng.schedule_submit_top_scores(p, q, topn=topn)
        else:
            submit = eng.schedule_submit
        for k in range(args.warmup):
            eng.schedule_wait(submit(pods[k * P:(k + 1) * P], seq[k * P:(k + 1) * P]))
        eng.synchronize()
        t0 = time.perf_counter()
        tables = rows = 0
        s0 = args.warmup
        h = submit(pods[s0 * P:(s0 + 1) * P], seq[s0 * P:(s0 + 1) * P])
        for s in range(s0 + 1, s0 + args.steps + 1):
            h2 = submit(pods[s * P:(s + 1) * P], seq[s * P:(s + 1) * P]) if s < s0 + args.steps else None
            r = eng.schedule_wait(h)
            if topn:   # every scored pod has its table, headed by the total it was placed at
                out, tr, cnt = r
                scored = (out["node"] >= 0) & (out["feasible"] >= 2)
                assert np.array_equal(cnt > 0, scored) and (tr["total"][scored, 0] == out["score"][scored]).all()
                assert (tr["total"][scored, 0] == tr["plugin"][scored, 0].astype(np.int64) @ w).all()
                tables += int(scored.sum())
                rows += int(cnt.sum())
            h = h2
        eng.synchronize()
        dt = time.perf_counter() - t0
        bad = eng.mirror_check()
        eng.close()
        assert bad == 0
        res = {"pods_per_s": round(args.steps * P / dt, 1)}
        if topn:
            res.update(tables=tables, rows=rows)
        return res

    out = {"workload": f"C3 {args.nodes} nodes x {args.steps} steps of {P} pods, submitted one step ahead"}
    if args.only is not None:
        out[f"top{args.only}"] = run(args.only)
    else:
        out["plain"] = run(0)
        for topn in (8, 64):
            out[f"top{topn}"] = run(topn)
            out[f"top{topn}_over_plain"] = round(out[f"top{topn}"]["pods_per_s"] / out["plain"]["pods_per_s"], 4)
            if args.host_timing:
                os.environ["GS_HOST_TIMING"] = "1"
                print(f"host timing, topn {topn}:", file=sys.stderr, flush=True)
                run(topn)
                del os.environ["GS_HOST_TIMING"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
