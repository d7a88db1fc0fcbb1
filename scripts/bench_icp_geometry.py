"""The geometric ICP rejectors (mm3d_set_icp_geometry_rejection, mm3d_boundary_points) measured.  Stand-alone; bench.py is not
involved.  One JSON line per row as it finishes, appended to profiles/icp_geometry.jsonl with --append.

  python scripts/bench_icp_geometry.py --kernel     # the boundary stage call alone on one headline map (500 k raw points, the
                                                    # defaults) and on one dense map (2 M raw points in a 30 m window at
                                                    # resolution 0.05): ms per call and the share of points flagged
  python scripts/bench_icp_geometry.py              # accuracy on the lattice scene of DESIGN.md section 7c (4 x 200 k points,
                                                    # overlap_step 0.25, FPFH, prerejective alignment, 8 streams, seeds 1 2 3):
                                                    # pairs within --bound (Frobenius), median final error, iteration histogram
  python scripts/bench_icp_geometry.py --timing     # ms per call: the inactive context and one selecting context take turns in
                                                    # one process, --reps timed calls each after a warm-up round
  python scripts/bench_icp_geometry.py --one-call   # one warm-up and one call with --row, for a kernel trace around it
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

ROWS = collections.OrderedDict([
    ("inactive", {}),
    ("boundary", dict(boundary=1)),
    ("normals_45", dict(normals=1, normal_angle_deg=45.0)),
    ("normals_30", dict(normals=1, normal_angle_deg=30.0)),
    ("boundary+normals_45", dict(boundary=1, normals=1, normal_angle_deg=45.0)),
])


def context(mm, args, options):
    ctx = mm.Context(0)
    ctx.setStreams(args.streams)
    ctx.setAlignment(method=mm.AlignMethod.PREREJECTIVE)
    if options:
        ctx.setIcpGeometryRejection(**options)
    return ctx


def emit(args, row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(os.path.join(ROOT, "profiles", "icp_geometry.jsonl"), "a") as f:
            f.write(line + "\n")


def one_map(n_points, window):
    """Map 0 of a 16-map loop of the synthetic world at this size, without sampling the other fifteen."""
    from map_merge_amd import synth
    w = window or synth.window_for(n_points)
    loop_r = 0.5 * w * 16 / (2.0 * np.pi)
    world = synth.synth_world(1234, extent=max(2.0 * (loop_r + w / 2.0 + 2.0), w + 4.0))
    xyz, rgb, _ = synth.synth_map(world, 0, n_points, n_maps=16, window=w)
    return synth.pack_points(xyz, rgb)


def neighbourhood_sizes(xyz, radius, sample=20000):
    """Points within `radius` of a seeded sample of the cloud's points, themselves excluded, from a k-d tree on the host (scipy):
    quantiles, and the share of neighbourhoods above the kernel's 512-direction arena.  None where scipy is missing."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    xyz = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    pick = np.random.default_rng(1).choice(len(xyz), min(sample, len(xyz)), replace=False)
    counts = cKDTree(xyz).query_ball_point(xyz[pick], radius, return_length=True) - 1
    q = {f"p{int(p)}": int(np.percentile(counts, p)) for p in (0, 10, 50, 90, 99, 100)}
    return {"sample": int(len(pick)), **q, "share_above_512": round(float((counts > 512).mean()), 4),
            "histogram_edges": [0, 32, 64, 128, 256, 512, 1024, 1 << 30],
            "histogram": np.histogram(counts, bins=[0, 32, 64, 128, 256, 512, 1024, 1 << 30])[0].tolist()}


def kernel(mm, args):
    cases = [("headline_500k", 500000, 0.0, {}), ("dense_2M_30m_res0.05", 2000000, 30.0, dict(resolution=0.05))]
    for name, n, window, pkw in cases:
        params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, **pkw)
        ctx = mm.Context(0)
        m = ctx.mapFeatures(ctx.cloud(one_map(n, window)), params)
        points = m.points
        normals = ctx.computeSurfaceNormals(points, params.normal_radius)
        radius = params.normal_radius
        ms, flagged = [], 0
        for rep in range(args.reps + 1):                   # (the first call builds the grid and is not counted)
            t0 = time.perf_counter()
            flags, flagged = ctx.boundaryPoints(points, normals, radius)
            ms.append((time.perf_counter() - t0) * 1e3)
        a = points.numpy()
        sizes = neighbourhood_sizes(np.stack([a["x"], a["y"], a["z"]], axis=1), radius)
        emit(args, {"row": "boundary_stage_call", "map": name, "raw_points": n, "points": len(points), "radius": radius, "angle_deg": 90.0,
                    "flagged": flagged, "flagged_share": round(flagged / max(len(points), 1), 4), "first_call_ms": round(ms[0], 2),
                    "ms_per_call_median": round(statistics.median(ms[1:]), 3), "ms_per_call_min": round(min(ms[1:]), 3),
                    "ms_per_call_max": round(max(ms[1:]), 3), "includes": "the flags' copy to the host and the count",
                    "neighbourhood_sizes": sizes})
        ctx.close()


def accuracy(mm, args, scene, host, T_gt, params):
    from map_merge_amd import synth
    for name, options in ROWS.items():
        errors, iters = [], collections.Counter()
        for seed in args.seeds:
            ctx = context(mm, args, options)
            ctx.srand(seed)
            _, pairs = ctx.estimateMapsTransforms(host, params, return_pairs=True)
            ctx.close()
            for p in pairs:
                s, t = int(p["source_idx"]), int(p["target_idx"])
                errors.append(float(np.linalg.norm(p["transform"].reshape(4, 4).T - synth.relative_gt(T_gt[s], T_gt[t]))))
                iters[int(p["icp_iterations"])] += 1
        emit(args, {"scene": scene, "row": name, "options": options, "seeds": args.seeds, "streams": args.streams, "bound": args.bound,
                    "pairs": len(errors), "recovered": int(sum(e <= args.bound for e in errors)),
                    "median_error": round(statistics.median(errors), 5), "errors": [round(e, 4) for e in errors],
                    "icp_iterations": {str(k): v for k, v in sorted(iters.items())}})


def timing(mm, args, scene, host, params):
    """The inactive context runs the machine code the library had before the selection existed: it is the baseline."""
    for name in args.timing_rows:
        ctxs = {"inactive": context(mm, args, {}), name: context(mm, args, ROWS[name])}
        times = {k: [] for k in ctxs}
        for rep in range(args.reps + 1):                   # (the first round warms the pools up and is not counted)
            for k in (list(ctxs) if rep % 2 == 0 else list(ctxs)[::-1]):
                ctxs[k].srand(1)
                t0 = time.perf_counter()
                ctxs[k].estimateMapsTransforms(host, params)
                times[k].append((time.perf_counter() - t0) * 1e3)
        for k, c in ctxs.items():
            c.close()
            ms = times[k][1:]
            emit(args, {"scene": scene, "row": "ms_per_call_" + k, "against": name, "streams": args.streams, "reps": args.reps,
                        "ms_per_call_median": round(statistics.median(ms), 2), "ms_per_call_min": round(min(ms), 2),
                        "ms_per_call_max": round(max(ms), 2), "ms_per_call": [round(t, 2) for t in ms]})


def one_call(mm, args, host, params):
    ctx = context(mm, args, ROWS[args.row])
    for _ in range(2):
        ctx.srand(1)
        ctx.estimateMapsTransforms(host, params)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--row", default="boundary+normals_45", choices=list(ROWS))
    ap.add_argument("--timing-rows", nargs="*", default=["boundary", "normals_45", "boundary+normals_45"], choices=list(ROWS)[1:])
    ap.add_argument("--append", action="store_true", help="also append the rows to profiles/icp_geometry.jsonl")
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--bound", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--streams", type=int, default=8)
    args = ap.parse_args()
    mm = ge.load()
    if args.kernel:
        kernel(mm, args)
        return
    from map_merge_amd import synth
    host, T_gt, _ = synth.cached_maps(4, 200000, family="lattice", overlap_step=0.25)
    scene = "lattice_4x200k"
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    if args.one_call:
        one_call(mm, args, host, params)
    elif args.timing:
        timing(mm, args, scene, host, params)
    else:
        accuracy(mm, args, scene, host, T_gt, params)


if __name__ == "__main__":
    main()
