"""Point-to-point against point-to-plane ICP (mm3d_set_icp_method) on the benchmark's scenes: ms per
mm3d_estimate_maps_transforms call (median), the icp_iterations of every pair, the converged fraction (a pair record carries
no converged flag: the fraction of pairs whose ICP stopped before max_iterations), and the rotation / translation error of
every pair against synth.relative_gt.  Stand-alone; bench.py is not involved.

  python scripts/bench_icp_method.py                        # headline: 16 x 500 k, FPFH + SAC_IA + ICP
  python scripts/bench_icp_method.py --config indoor        # dense indoor: 8 x 2 M, SHOT, 30 m windows, resolution 0.05
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

import bench  # noqa: E402
import __graft_entry__ as ge  # noqa: E402

CONFIGS = {
    "headline": dict(maps=16, points=500000, descriptor="FPFH", window=0.0, resolution=0.0),
    "indoor": dict(maps=8, points=2000000, descriptor="SHOT", window=30.0, resolution=0.05),
}


def rot_trans_err(T, G):
    D = np.linalg.inv(G) @ T
    c = np.clip((np.trace(D[:3, :3]) - 1.0) * 0.5, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(D[:3, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="headline")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=16)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    mm = ge.load()
    from map_merge_amd import synth
    host, T_gt, _ = bench.make_workload_gt(cfg["maps"], cfg["points"], cache=True, window=cfg["window"])
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor[cfg["descriptor"]], estimation_method=mm.EstimationMethod.SAC_IA,
                                 refine_transform=1)
    if cfg["resolution"] > 0:
        params.resolution = cfg["resolution"]
    rows = {}
    for method in (mm.IcpMethod.POINT_TO_POINT, mm.IcpMethod.POINT_TO_PLANE):
        ctx = mm.Context(0)
        ctx.setStreams(args.streams)
        ctx.setIcpMethod(method)
        times, pairs = [], None
        for _ in range(args.reps + 1):                 # (the first call warms the pools up and is not counted)
            ctx.srand(1)
            t0 = time.perf_counter()
            _, pairs = ctx.estimateMapsTransforms(host, params, return_pairs=True)
            times.append((time.perf_counter() - t0) * 1e3)
        it = pairs["icp_iterations"].astype(int)
        errs = [rot_trans_err(p["transform"].reshape(4, 4).T.astype(np.float64),
                              synth.relative_gt(T_gt[int(p["source_idx"])], T_gt[int(p["target_idx"])])) for p in pairs]
        good = [e for e in errs if e[0] < 5.0 and e[1] < 1.0]    # pairs whose initial estimate found the basin
        rows[method.name] = {
            "ms_per_call_median": statistics.median(times[1:]), "ms_per_call": times[1:], "pairs": len(pairs),
            "icp_iterations_hist": {int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))},
            "icp_iterations_mean": float(it.mean()) if len(it) else 0.0,
            "converged_fraction": float((it < params.max_iterations).mean()) if len(it) else 0.0,
            "rot_err_deg_median": statistics.median([e[0] for e in errs]) if errs else None,
            "trans_err_m_median": statistics.median([e[1] for e in errs]) if errs else None,
            "pairs_in_basin": len(good),
            "rot_err_deg_median_in_basin": statistics.median([e[0] for e in good]) if good else None,
            "trans_err_m_median_in_basin": statistics.median([e[1] for e in good]) if good else None,
        }
        ctx.close()
    print(json.dumps({"config": args.config, **cfg, "streams": args.streams, "methods": rows}))


if __name__ == "__main__":
    main()
