"""What one ICP iteration costs with a robust kernel (mm3d_set_icp_robust), beside a default iteration and a rejecting one
(mm3d_set_icp_rejection), on one pair of headline-sized maps: the library's own profile table (mm3d_profile_*) around the
stage-level calls, kernel time summed per iteration's launches.  Stand-alone; bench.py is not involved.

  python scripts/icp_robust_cost.py [--points 500000] [--iterations 10] [--reps 5] [--out profiles/icp_robust_cost.json]

Every row runs the same fixed number of iterations from the same guess (transformation_epsilon 0 and a robust schedule that stays
above its final scale, so that no convergence test ends a run early where that can be avoided); ms_per_iteration is the kernel time of the row's
launches divided by the iterations the call reports.  One JSON document: the rows and the three headline numbers."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

KERNELS = {"default": ("icp_corr_reduce", "icp_finalize"),
           "default_plane": ("icp_plane_corr_reduce", "icp_plane_finalize"),
           "robust": ("icp_robust_corr_reduce", "icp_robust_finalize"),
           "rejecting": ("icp_reject_begin", "icp_reject_search", "icp_reject_select", "icp_reject_reduce", "icp_finalize", "icp_plane_finalize")}


def measure(ctx, names, call, reps):
    """median over reps of (kernel ms of `names` / iterations), and the last call's per-kernel split"""
    per_iter, split, iters = [], {}, 0
    for rep in range(reps + 1):                           # (the first round warms the pools up and is not counted)
        ctx.profile_reset()
        call()
        iters = int(ctx.last_icp_iterations)
        entries = ctx.profile_entries()
        split = {k: {"ms": round(entries[k]["ms"], 4), "launches": int(entries[k]["launches"])} for k in names if k in entries}
        if rep and iters:
            per_iter.append(sum(v["ms"] for v in split.values()) / iters)
    return {"iterations": iters, "ms_per_iteration": round(statistics.median(per_iter), 4) if per_iter else None,
            "ms_per_iteration_min": round(min(per_iter), 4) if per_iter else None,
            "ms_per_iteration_max": round(max(per_iter), 4) if per_iter else None, "last_call": split}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    _, maps = synth.synth_maps(2, args.points)
    ctx = mm.Context(0)
    clouds = []
    for x, col, _ in maps:                                # the pair stage's input: the filtered maps
        d = ctx.downSample(ctx.cloud(synth.pack_points(x, col)), 0.1)
        clouds.append(ctx.removeOutliers(d, 0.8, 50))
    src, tgt = clouds
    normals = ctx.computeSurfaceNormals(tgt, 0.6)
    guess = np.eye(4, dtype=np.float32)
    it, corr = args.iterations, 1.0
    gm = mm.IcpRobustOptions(kernel=mm.RobustKernel.GEMAN_MCCLURE, scale=0.01, scale_start=0.4, anneal=0.9)
    trimmed = mm.IcpRejectionOptions(distance=mm.RejectDistance.TRIMMED, overlap_ratio=0.7)
    rows = [("default", "default", lambda: ctx.estimateTransformICP(src, tgt, guess, corr, 0.5, it, 0.0)),
            ("default_plane", "default_plane", lambda: ctx.estimateTransformICPPlane(src, tgt, normals, guess, corr, it, 0.0)),
            ("robust_geman_mcclure", "robust", lambda: ctx.estimateTransformICPRobust(src, tgt, None, guess, corr, gm, it, 0.0)),
            ("robust_geman_mcclure_plane", "robust", lambda: ctx.estimateTransformICPRobust(src, tgt, normals, guess, corr, gm, it, 0.0)),
            ("robust_huber", "robust", lambda: ctx.estimateTransformICPRobust(src, tgt, None, guess, corr, mm.IcpRobustOptions(kernel=mm.RobustKernel.HUBER), it, 0.0)),
            ("rejecting_trimmed_0.7", "rejecting", lambda: ctx.estimateTransformICPRejecting(src, tgt, None, guess, corr, trimmed, it, 0.0)),
            ("rejecting_trimmed_0.7_plane", "rejecting", lambda: ctx.estimateTransformICPRejecting(src, tgt, normals, guess, corr, trimmed, it, 0.0))]
    ctx.profile(True)
    out = {"raw_points_per_map": args.points, "source_points": len(src), "target_points": len(tgt), "max_correspondence_distance": corr,
           "iterations_asked": it, "reps": args.reps, "rows": {}}
    for name, kind, call in rows:
        out["rows"][name] = measure(ctx, KERNELS[kind], call, args.reps)
        print(json.dumps({name: out["rows"][name]}), flush=True)
    ctx.profile(False)
    ctx.close()
    r = out["rows"]
    out["headline_ms_per_iteration"] = {"default": r["default"]["ms_per_iteration"], "robust": r["robust_geman_mcclure"]["ms_per_iteration"],
                                        "rejecting": r["rejecting_trimmed_0.7"]["ms_per_iteration"]}
    print(json.dumps(out["headline_ms_per_iteration"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
