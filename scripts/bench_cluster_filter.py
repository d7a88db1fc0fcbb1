"""The cluster filter (mm3d_set_cluster_filter) measured: what it costs beside the radius filter it follows, on one headline map
-- 500 k raw points, down-sampled at 0.1 -- and whether it helps registration, on two views of one synthetic room with their
own blobs.  Stand-alone; bench.py is not touched.  One JSON line per row as it finishes; --append adds them to
profiles/cluster_filter.jsonl.

  python scripts/bench_cluster_filter.py                  # cost, then registration
  python scripts/bench_cluster_filter.py --cost-only
  python scripts/bench_cluster_filter.py --registration-only
  python scripts/bench_cluster_filter.py --cost-only --one-call      # two calls, for a kernel trace around them
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402

TOL = 0.2                                                  # twice the resolution: what tolerance 0 stands for


def emit(args, row):
    row = {"label": args.label, **row}
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = f()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def headline_map(n_maps=16, n_points=500000):
    """Map 0 of bench.py's headline workload (synth.synth_maps(16, 500000)), without generating the other fifteen."""
    from map_merge_amd import synth
    w = synth.window_for(n_points)
    loop_r = 0.5 * w * n_maps / (2.0 * np.pi)
    world = synth.synth_world(1234, extent=max(2.0 * (loop_r + w / 2.0 + 2.0), w + 4.0))
    x, c, _ = synth.synth_map(world, 0, n_points, n_maps=n_maps)
    return synth.pack_points(x, c)


def cost(mm, args):
    """The stage calls taking turns in one process.  `warm`: on one cloud, whose grid the first round built (how the radius
    filter's figure of DESIGN.md section 7n was taken).  `cold`: on a fresh copy of the cloud each time, its bounding box known,
    so that the call builds its grid as it does behind a whole-map call."""
    import cluster_cases as cc
    host = [headline_map()]
    ctx = mm.Context(0)
    down = ctx.downSample(ctx.cloud(host[0]), 0.1)
    filt = ctx.removeOutliers(down, 0.8, 50)
    if args.one_call:                                      # two calls, for a kernel trace around them
        for _ in range(2):
            kept = ctx.removeSmallClusters(filt, TOL, mm.ClusterMethod.MIN_SIZE, 100)
        ctx.synchronize()
        print("kept", len(kept), "of", len(filt), ctx.last_cluster_stats, flush=True)
        ctx.close()
        return
    rows = {
        "radius_0.8_50": lambda d, f: ctx.removeOutliers(d, 0.8, 50),
        "clusters_min_size_100": lambda d, f: ctx.removeSmallClusters(f, TOL, mm.ClusterMethod.MIN_SIZE, 100),
        "clusters_largest": lambda d, f: ctx.removeSmallClusters(f, TOL, mm.ClusterMethod.LARGEST, 1),
        "cluster_labels": lambda d, f: ctx.clusterLabels(f, TOL),
    }
    for mode in ("warm", "cold"):
        times = {r: [] for r in rows}
        kept, stats = {}, {}
        for rep in range(args.reps + 1):                   # (the first round warms the pools up and is not counted)
            if mode == "cold":                             # fresh clouds: no grid on them yet (their boxes come with them)
                d = ctx.downSample(ctx.cloud(host[0]), 0.1)
                f = ctx.removeOutliers(d, 0.8, 50)
            else:
                d, f = down, filt
            for r, call in rows.items():                   # the rows take turns
                if mode == "cold" and r != "radius_0.8_50":
                    f = ctx.removeOutliers(d, 0.8, 50)     # (every cluster row its own fresh cloud)
                if mode == "cold" and r == "radius_0.8_50":
                    d = ctx.downSample(ctx.cloud(host[0]), 0.1)
                ms, out = timed(ctx, lambda: call(d, f))
                if rep:
                    times[r].append(ms)
                kept[r] = len(out)
                stats[r] = ctx.last_cluster_stats if r.startswith("clusters_") else None
        for r in rows:
            emit(args, {"what": "stage", "mode": mode, "row": r, "raw_points": len(host[0]), "down_sampled": len(down), "filtered": len(filt),
                        "kept": kept[r], "ms_median": statistics.median(times[r]), "ms_min": min(times[r]), "ms_all": [round(t, 4) for t in times[r]],
                        "last_cluster_stats": stats[r]})
    # the chain: the longest path a cloud of its size can have, and the blob: every hook on one root
    for name in ("a_chain", "d_dense_blob", "i_random_1"):
        xyz, tol = cc.cases()[name]
        a = np.zeros(len(xyz), dtype=mm.POINT)
        a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        cl = ctx.cloud(a)
        ts = []
        for rep in range(args.reps + 1):
            ms, lab = timed(ctx, lambda: ctx.clusterLabels(cl, tol))
            if rep:
                ts.append(ms)
        emit(args, {"what": "case", "row": name, "points": len(xyz), "clusters": int(len(np.unique(lab[lab >= 0]))), "ms_median": statistics.median(ts),
                    "ms_min": min(ts), "hook_launches": 1, "kernel_launches": 4})
    ctx.close()


def _pose(yaw, shift):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = shift
    return T


def registration(mm, args):
    """Two views of tests/cluster_cases.py's room, each with its own three blobs; FPFH; MATCHING and SAC_IA, with and without the
    ICP; srand 1 .. seeds.  Rotation and translation error of the one pair record against the ground truth, filter off and on,
    and how many of the keypoints lay on blobs."""
    import cluster_cases as cc
    from map_merge_amd import synth
    views = ((1, 0.0, (0.0, 0.0, 0.0)), (2, 0.35, (1.5, -0.8, 0.0)))
    raws, Tg, boxes = [], [], []
    for seed, yaw, shift in views:
        xyz, rgb, _, bx = cc.room_with_blobs(seed, yaw, shift)
        raws.append(synth.pack_points(xyz, rgb))
        Tg.append(_pose(yaw, shift))
        boxes.append(bx)

    def on_blobs(cloud, i):
        a = cloud.numpy()
        p = np.stack([a["x"], a["y"], a["z"], np.ones(len(a))], axis=1) @ np.linalg.inv(Tg[i]).T      # back in the room's frame
        return int(np.any([((p[:, :3] >= lo) & (p[:, :3] <= hi)).all(axis=1) for lo, hi in boxes[i]], axis=0).sum())

    for method in ("MATCHING", "SAC_IA"):
        for refine in (0, 1):
            p = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=getattr(mm.EstimationMethod, method), refine_transform=refine)
            for on in (False, True):
                c = mm.Context(0)
                if on:
                    c.setClusterFilter(method=mm.ClusterMethod.MIN_SIZE, min_size=cc.ROOM_MIN_SIZE)
                feats = [c.mapFeatures(c.cloud(r), p) for r in raws]
                kp = [len(m.keypoints) for m in feats]
                kp_blob = [on_blobs(m.keypoints, i) for i, m in enumerate(feats)]
                pts = [len(m.points) for m in feats]
                rot, tra, conf = [], [], []
                for seed in range(1, args.seeds + 1):
                    c.srand(seed)
                    _, pairs = c.estimateMapsTransforms(raws, p, return_pairs=True)
                    if len(pairs) == 0:
                        rot.append(None), tra.append(None), conf.append(None)
                        continue
                    r = pairs[0]
                    T = r["transform"].reshape(4, 4).T.astype(np.float64)
                    gt = synth.relative_gt(Tg[int(r["source_idx"])], Tg[int(r["target_idx"])])
                    dR = T[:3, :3] @ gt[:3, :3].T
                    rot.append(float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))))
                    tra.append(float(np.linalg.norm(T[:3, 3] - gt[:3, 3])))
                    conf.append(float(r["confidence"]))
                emit(args, {"what": "registration", "method": method, "icp": refine, "cluster_filter": on, "points": pts, "keypoints": kp,
                            "keypoints_on_blobs": kp_blob, "rot_err_deg": rot, "trans_err_m": tra, "confidence": conf})
                c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--cost-only", action="store_true")
    ap.add_argument("--registration-only", action="store_true")
    ap.add_argument("--one-call", action="store_true", help="with --cost-only: two MIN_SIZE calls on the headline map and nothing else")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_filter.jsonl"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    mm = ge.load()
    if not args.registration_only:
        cost(mm, args)
    if not args.cost_only:
        registration(mm, args)


if __name__ == "__main__":
    main()
