"""The MLS smoothing (mm3d_set_smoothing) measured with the library's profile scopes (mm3d_profile_*: device time per kernel name):
on one headline map -- 500 k raw points, down-sampled at 0.1 and radius-filtered, r = 0.3 -- beside the stand-alone normals
launch, which walks a comparable neighbourhood once, in float; and on the composed headline map -- the sixteen maps at their
true poses, one voxel pass at 0.1, r = 0.3.  Stand-alone; bench.py is not touched.  One JSON line per row as it finishes;
--append adds them to profiles/smoothing.jsonl.

  python scripts/bench_smoothing.py                  # the map, then the composed map
  python scripts/bench_smoothing.py --map-only
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

RADIUS = 0.3
KERNELS = ("mls_fit", "mls_stats", "mls_apply")


def emit(args, row):
    row = {"label": args.label, **row}
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def headline_maps(which, n_maps=16, n_points=500000):
    """Maps `which` of bench.py's headline workload (synth.synth_maps(16, 500000)) and their true poses."""
    from map_merge_amd import synth
    w = synth.window_for(n_points)
    loop_r = 0.5 * w * n_maps / (2.0 * np.pi)
    world = synth.synth_world(1234, extent=max(2.0 * (loop_r + w / 2.0 + 2.0), w + 4.0))
    out = []
    for i in which:
        x, c, T = synth.synth_map(world, i, n_points, n_maps=n_maps)
        out.append((synth.pack_points(x, c), T))
    return out


def profiled(ctx, reps, call):
    """Device milliseconds per kernel name (median over reps, after one uncounted round) and the call's wall time."""
    per, wall = {}, []
    for rep in range(reps + 1):
        ctx.profile_reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            wall.append(ms)
            for k, v in ctx.profile_entries().items():
                per.setdefault(k, []).append(v["ms"])
    return {k: statistics.median(v) for k, v in per.items()}, statistics.median(wall), out


def one_map(mm, args):
    (host, _), = headline_maps([0])
    ctx = mm.Context(0)
    down = ctx.downSample(ctx.cloud(host), 0.1)
    filt = ctx.removeOutliers(down, 0.8, 50)
    ctx.profile(True)
    for order in (2, 1):
        per, wall, out = profiled(ctx, args.reps, lambda: ctx.smoothCloud(filt, RADIUS, order, 6))
        emit(args, {"what": "map", "row": "smooth_order_%d" % order, "raw_points": len(host), "filtered": len(filt), "radius": RADIUS,
                    "kernel_ms": {k: round(per.get(k, 0.0), 4) for k in KERNELS}, "wall_ms": round(wall, 4), "stats": ctx.last_smooth_stats})
    per, wall, _ = profiled(ctx, args.reps, lambda: ctx.computeSurfaceNormals(filt, 0.6))
    emit(args, {"what": "map", "row": "normals_0.6", "kernel_ms": {k: round(v, 4) for k, v in per.items()}, "wall_ms": round(wall, 4)})
    per, wall, _ = profiled(ctx, args.reps, lambda: ctx.computeSurfaceNormals(filt, RADIUS))
    emit(args, {"what": "map", "row": "normals_0.3", "kernel_ms": {k: round(v, 4) for k, v in per.items()}, "wall_ms": round(wall, 4)})
    ctx.close()


def composed(mm, args):
    maps = headline_maps(range(16))
    ctx = mm.Context(0)
    clouds = [ctx.cloud(h) for h, _ in maps]
    poses = [np.linalg.inv(T).astype(np.float32) for _, T in maps]      # (T maps the world into the map's frame)
    first = ctx.composeMaps(clouds, poses, 0.1)
    ctx.profile(True)
    per, wall, out = profiled(ctx, args.reps, lambda: ctx.smoothCloud(first, RADIUS, 2, 6))
    emit(args, {"what": "composed", "row": "smooth_order_2", "points": len(first), "radius": RADIUS,
                "kernel_ms": {k: round(per.get(k, 0.0), 4) for k in KERNELS}, "wall_ms": round(wall, 4), "stats": ctx.last_smooth_stats})
    ctx.profile(False)
    plain_ms, smooth_ms = [], []
    for rep in range(args.reps + 1):
        for opt, acc in ((dict(method=0), plain_ms), (dict(method=1, radius=RADIUS), smooth_ms)):
            ctx.setSmoothing(**opt)
            ctx.synchronize()
            t0 = time.perf_counter()
            res = ctx.composeMaps(clouds, poses, 0.1)
            ctx.synchronize()
            if rep:
                acc.append((time.perf_counter() - t0) * 1e3)
            if opt["method"]:
                fused = len(res)
    emit(args, {"what": "composed", "row": "compose_maps", "points_plain": len(first), "points_smoothed": fused,
                "wall_ms_plain": round(statistics.median(plain_ms), 3), "wall_ms_smoothed": round(statistics.median(smooth_ms), 3)})
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--label", default="smoothing")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothing.jsonl"))
    ap.add_argument("--map-only", action="store_true")
    ap.add_argument("--composed-only", action="store_true")
    args = ap.parse_args()
    mm = ge.load()
    if not args.composed_only:
        one_map(mm, args)
    if not args.map_only:
        composed(mm, args)


if __name__ == "__main__":
    main()
