"""The plane stage (mm3d_set_planes) measured: what mm3d_remove_planes costs on one headline map -- 500 k raw points,
down-sampled at 0.1, radius-filtered -- for 256, 1 024 and 4 096 draws and 1 and 4 planes, warm and cold, next to
removeSmallClusters in the same process; and the count kernel's share against its arithmetic.  Stand-alone; bench.py is not
touched.  One JSON line per row as it finishes; --append adds them to profiles/planes.jsonl.

  python scripts/bench_planes.py
  python scripts/bench_planes.py --one-call      # two calls of the default setting, for a kernel trace around them
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import __graft_entry__ as ge  # noqa: E402
from bench_cluster_filter import headline_map, timed  # noqa: E402

DISTANCE = 0.05                                            # half the resolution: what distance 0 stands for
FLOPS_PER_TEST = 12                                        # three differences, a dot product of five, a square, a compare and a vote


def emit(args, row):
    row = {"label": args.label, **row}
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--one-call", action="store_true", help="two calls with 1 024 draws and one plane on the headline map and nothing else")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes.jsonl"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    mm = ge.load()
    host = headline_map()
    ctx = mm.Context(0)
    down = ctx.downSample(ctx.cloud(host), 0.1)
    filt = ctx.removeOutliers(down, 0.8, 50)
    if args.one_call:
        for _ in range(2):
            kept = ctx.removePlanes(filt, distance=DISTANCE)
        ctx.synchronize()
        print("kept", len(kept), "of", len(filt), ctx.last_plane_stats, ctx.last_planes, flush=True)
        ctx.close()
        return
    rows = {"clusters_min_size_100": lambda f: ctx.removeSmallClusters(f, 0.2, mm.ClusterMethod.MIN_SIZE, 100)}
    for planes in (1, 4):
        for samples in (256, 1024, 4096):
            rows["planes_%d_samples_%d" % (planes, samples)] = (
                lambda f, planes=planes, samples=samples: ctx.removePlanes(f, max_planes=planes, samples=samples, distance=DISTANCE))
    for mode in ("warm", "cold"):
        times = {r: [] for r in rows}
        kept, stats = {}, {}
        for rep in range(args.reps + 1):                   # (the first round warms the pools up and is not counted)
            for r, call in rows.items():                   # the rows take turns
                f = ctx.removeOutliers(down, 0.8, 50) if mode == "cold" else filt      # cold: a fresh cloud, nothing cached on it
                ms, out = timed(ctx, lambda: call(f))
                if rep:
                    times[r].append(ms)
                kept[r] = len(out)
                stats[r] = ctx.last_plane_stats if r.startswith("planes_") else ctx.last_cluster_stats
        for r in rows:
            row = {"what": "stage", "mode": mode, "row": r, "raw_points": len(host), "down_sampled": len(down), "filtered": len(filt), "kept": kept[r],
                   "ms_median": statistics.median(times[r]), "ms_min": min(times[r]), "ms_all": [round(t, 4) for t in times[r]], "stats": stats[r]}
            if r.startswith("planes_"):                    # samples x m tests per round that drew, m shrinking with every plane found
                row["tests_upper_bound"] = stats[r]["draws"] * len(filt)
                row["f64_ops_upper_bound"] = row["tests_upper_bound"] * FLOPS_PER_TEST
            emit(args, row)
    ctx.close()


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("bench_planes: %.1f s" % (time.time() - t0), flush=True)
