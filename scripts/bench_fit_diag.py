"""Cost of the FitError diagnosis on one GPU: the C3 workload of bench.py (50k nodes, NodeNUMAResource profile, 2048
pods per step submitted one step ahead) through gs_schedule_submit_diag beside the same run through
gs_schedule_submit, in two variants: the workload as it is, and with every 17th pod oversized (no node holds it).
Prints one JSON line. Run: python scripts/bench_fit_diag.py [--steps 20]

  --host-timing   one more diagnosed run per variant under GS_HOST_TIMING=1: the library prints, on stderr, the host time
                  per batch spent deriving landed-row versions and in the landed pass
  --only V        run variant V (as_is | every17) diagnosed only, for a profiler:
                  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_fit_diag.py --only every17 --steps 5
                  (fit_diag_kernel<...> and fit_diag_landed_kernel are the diagnosis' kernels)
  --nodes-map     a third run per variant through gs_schedule_submit_diag_nodes, with a status row for every FitError pod
                  of a step (cap_rows = pods per step): its pods/s, the rows and their device-to-host bytes, and the
                  ratio to the counters-only run beside it; with --only, the diagnosed run is that one
                  (fit_diag_kernel<..., true> and fit_diag_landed_map_kernel are its kernels)"""
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
    ap.add_argument("--only", choices=["as_is", "every17"], default=None)
    ap.add_argument("--nodes-map", action="store_true")
    args = ap.parse_args()

    from koordinator_amd import abi, config, synth
    from koordinator_amd.engine import Engine

    P, total = args.pods_per_step, (args.warmup + args.steps) * args.pods_per_step
    cluster = synth.make_cluster(args.nodes, total, config_id=2)
    synth.make_numa(cluster)
    cfg = config.make_config(args.nodes, enabled=abi.GS_ENABLE_ALL)
    seq = np.arange(total, dtype=np.uint64)
    big = cluster.pods.copy()
    big["requests"][5::17, 0] = big["nonzero_requests"][5::17, 0] = 400_000
    big["request_mask"][5::17] |= 1
    variants = {"as_is": cluster.pods, "every17": big}

    npad = (args.nodes + 1023) // 1024 * 1024   # the device rows' stride

    def run(pods, diag: bool, nodes_map: bool = False):
        eng = Engine(cfg)
        synth.load_into(eng, cluster)
        submit = eng.schedule_submit_diag if diag else eng.schedule_submit
        if nodes_map:
            submit = lambda p, q: eng.schedule_submit_diag_nodes(p, q, cap_rows=P)
        first = (lambda r: r[0]) if diag else (lambda r: r)
        rows = 0
        for w in range(args.warmup):
            eng.schedule_wait(submit(pods[w * P:(w + 1) * P], seq[w * P:(w + 1) * P]))
        eng.synchronize()
        t0 = time.perf_counter()
        unplaced = diagnosed = 0
        s0 = args.warmup
        h = submit(pods[s0 * P:(s0 + 1) * P], seq[s0 * P:(s0 + 1) * P])
        for s in range(s0 + 1, s0 + args.steps + 1):
            h2 = submit(pods[s * P:(s + 1) * P], seq[s * P:(s + 1) * P]) if s < s0 + args.steps else None
            r = eng.schedule_wait(h)
            unplaced += int((first(r)["node"] < 0).sum())
            if diag:
                diagnosed += int(r[1]["valid"].sum())
                assert (r[1]["failed_nodes"][r[1]["valid"] == 1] == args.nodes).all()
            if nodes_map:   # a row for every such pod, in queue order, no entry without a status
                assert np.array_equal(np.nonzero(r[3] >= 0)[0], np.nonzero(r[1]["valid"])[0]) and (r[2] != 0).all()
                rows += len(r[2])
            h = h2
        eng.synchronize()
        dt = time.perf_counter() - t0
        bad = eng.mirror_check()
        eng.close()
        assert bad == 0 and (not diag or diagnosed == unplaced)
        res = {"pods_per_s": round(args.steps * P / dt, 1), "fit_errors": unplaced}
        if nodes_map:   # (the landed pass's words, at most 32 KiB per batch, are not counted)
            res.update(rows=rows, d2h_bytes_per_batch=round(rows * npad * 2 / (args.steps * P / 128)))
        return res

    out = {"workload": f"C3 {args.nodes} nodes x {args.steps} steps of {P} pods, submitted one step ahead"}
    for name, pods in variants.items():
        if args.only and name != args.only:
            continue
        if args.only:
            out[name] = {"map" if args.nodes_map else "diag": run(pods, True, args.nodes_map)}
            continue
        plain, diag = run(pods, False), run(pods, True)
        out[name] = {"plain": plain, "diag": diag,
                     "diag_over_plain": round(diag["pods_per_s"] / plain["pods_per_s"], 4)}
        if args.nodes_map:
            out[name]["map"] = run(pods, True, True)
            out[name]["map_over_diag"] = round(out[name]["map"]["pods_per_s"] / diag["pods_per_s"], 4)
        if args.host_timing:
            os.environ["GS_HOST_TIMING"] = "1"
            print(f"host timing, variant {name}:", file=sys.stderr, flush=True)
            run(pods, True, args.nodes_map)
            del os.environ["GS_HOST_TIMING"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
