"""The reference's radius outlier filter against the statistical one (mm3d_set_outlier_filter) on one headline map -- 500 k raw
points, down-sampled at 0.1 -- and through the whole 16 x 500 k call.  Stand-alone; bench.py is only read for the headline
workload.  One JSON line per row as it finishes; --append adds them to profiles/outliers_statistical.jsonl.

  python scripts/bench_outliers_statistical.py                    # the stage calls taking turns in one process, then the whole call
  python scripts/bench_outliers_statistical.py --stages-only      # ... the stage calls alone
  python scripts/bench_outliers_statistical.py --one-call --row statistical_16   # two calls of one row, for a kernel trace around them
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

ROWS = {"radius_0.8_50": None, "statistical_16": (16, 2.0), "statistical_50": (50, 1.0)}


def emit(args, row):
    row = {"label": args.label, **row}
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def stage_call(ctx, down, row):
    if ROWS[row] is None:
        return ctx.removeOutliers(down, 0.8, 50)
    return ctx.removeOutliersStatistical(down, *ROWS[row])


def stages(mm, args, raw):
    ctx = mm.Context(0)
    down = ctx.downSample(ctx.cloud(raw), 0.1)
    if args.one_call:
        for _ in range(2):
            kept = stage_call(ctx, down, args.row)
        ctx.synchronize()
        print(args.row, "kept", len(kept), "of", len(down), flush=True)
        return
    times = {r: [] for r in ROWS}
    kept = {}
    for rep in range(args.reps + 1):                       # (the first round warms the pools and the cloud's grids up and is not counted)
        for r in ROWS:                                      # the rows take turns
            ctx.synchronize()
            t0 = time.perf_counter()
            out = stage_call(ctx, down, r)
            ctx.synchronize()
            if rep:
                times[r].append((time.perf_counter() - t0) * 1e3)
            kept[r] = len(out)
            out.free()
    # how many queries looked past their first box of cells, and how many the second launch served (costs a wait: its own round)
    search = {}
    mm.lib().mm3d_set_debug(ctx._h, 1)
    for r, o in ROWS.items():
        if o is None:
            continue
        counters = (C.c_longlong * 3)()
        mm.lib().mm3d_debug_outlier_search(counters, 1)
        stage_call(ctx, down, r).free()
        mm.lib().mm3d_debug_outlier_search(counters, 1)
        search[r] = [int(v) for v in counters]
    mm.lib().mm3d_set_debug(ctx._h, 0)
    for r in ROWS:
        row = {"what": "stage", "row": r, "raw_points": len(raw), "down_sampled": len(down), "kept": kept[r], "kept_share": kept[r] / len(down),
               "ms_median": statistics.median(times[r]), "ms_all": [round(t, 4) for t in times[r]]}
        if r in search:
            q, second, listed = search[r]
            row.update(queries=q, past_first_box=second, second_launch=listed, past_first_box_share=second / max(q, 1),
                       second_launch_share=listed / max(q, 1))
        emit(args, row)
    ctx.close()


def whole_call(mm, args, host):
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    ctxs = {}
    for name, opt in (("radius", None), ("statistical_16", (16, 2.0))):
        c = mm.Context(0)
        c.setStreams(args.streams)
        if opt:
            c.setOutlierFilter(method=mm.OutlierMethod.STATISTICAL, mean_k=opt[0], stddev_mult=opt[1])
        ctxs[name] = c
    times = {n: [] for n in ctxs}
    sizes = {}
    for rep in range(args.reps + 1):
        for name, c in ctxs.items():                        # the two take turns
            c.srand(1)
            t0 = time.perf_counter()
            _, pairs = c.estimateMapsTransforms(host, params, return_pairs=True)
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
            sizes[name] = (c.lastRunMapSizes(), len(pairs))
    for name, c in ctxs.items():
        (pts, kps), n_pairs = sizes[name]
        emit(args, {"what": "whole_call", "row": name, "maps": len(host), "streams": args.streams, "ms_median": statistics.median(times[name]),
                    "ms_all": [round(t, 3) for t in times[name]], "pairs": n_pairs, "points_per_map_mean": float(np.mean(pts)),
                    "keypoints_per_map_mean": float(np.mean(kps))})
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--stages-only", action="store_true")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--row", choices=tuple(ROWS), default="statistical_16")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outliers_statistical.jsonl"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    mm = ge.load()
    import bench
    n_maps = 1 if (args.stages_only or args.one_call) else 16
    host, _, _ = bench.make_workload_gt(16, 500000, cache=True, window=0.0)
    stages(mm, args, host[0])
    if n_maps > 1:
        whole_call(mm, args, host)


if __name__ == "__main__":
    main()
