"""The reference's SIFT keypoints against uniform keypoints (mm3d_set_keypoints) on the scenes whose ground truth is known:
keypoints per map, pairs recovered and ms per mm3d_estimate_maps_transforms call (median of --reps calls after a warm-up).
Stand-alone; bench.py is only read for the headline workload.  One JSON line per configuration as it finishes.

  python scripts/bench_keypoints.py                         # lattice 4 x 200 k, prerejective, seeds 1 2 3: SIFT, then uniform at
                                                            # leaf = descriptor_radius / 1, 2, 4, 8 (the default-leaf sweep)
  python scripts/bench_keypoints.py --scene colourless      # the same maps with every point one colour, uniform at the default
  python scripts/bench_keypoints.py --scene independent     # 4 x 200 k independently sampled maps, SIFT and uniform, both alignments
  python scripts/bench_keypoints.py --scene headline        # 16 x 500 k independent maps: pairs of >= 30 % overlap within 0.5
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


def run(mm, synth, host, T_gt, params, streams, seed, reps, prerejective, leaf, judge):
    """leaf: None = the reference's detector, 0 = uniform at the default, > 0 = uniform at that leaf."""
    ctx = mm.Context(0)
    ctx.setStreams(streams)
    if prerejective:
        ctx.setAlignment(method=mm.AlignMethod.PREREJECTIVE)
    if leaf is not None:
        ctx.setKeypoints(source=mm.KeypointSource.UNIFORM, leaf=leaf)
    times, pairs = [], None
    for _ in range(reps + 1):                              # (the first call warms the pools up and is not counted)
        ctx.srand(seed)
        t0 = time.perf_counter()
        _, pairs = ctx.estimateMapsTransforms(host, params, return_pairs=True)
        times.append((time.perf_counter() - t0) * 1e3)
    errs = [float(np.linalg.norm(p["transform"].reshape(4, 4).T - synth.relative_gt(T_gt[int(p["source_idx"])], T_gt[int(p["target_idx"])])))
            for p in pairs]
    _, kps = ctx.lastRunMapSizes()
    row = {"keypoints": "sift" if leaf is None else "uniform", "leaf": leaf, "alignment": "prerejective" if prerejective else "sac_ia",
           "seed": seed, "ms_per_call_median": statistics.median(times[1:]) if reps else times[0], "pairs": len(pairs),
           "keypoints_per_map_mean": float(np.mean(kps)) if len(kps) else 0.0, "keypoints_per_map": [int(k) for k in kps]}
    row.update(judge(pairs, errs))
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("lattice", "colourless", "independent", "headline"), default="lattice")
    ap.add_argument("--divisors", type=float, nargs="*", default=[1, 2, 4, 8], help="leaf = descriptor_radius / divisor (lattice sweep)")
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=8)
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)

    def within_one(pairs, errs):
        return {"recovered_within_1.0": int(sum(e <= 1.0 for e in errs)), "errors": [round(e, 3) for e in errs]}

    def emit(host, T_gt, seed, prerejective, leaf, judge):
        print(json.dumps({"scene": args.scene, **run(mm, synth, host, T_gt, params, args.streams, seed, args.reps, prerejective, leaf, judge)}),
              flush=True)

    if args.scene in ("lattice", "colourless"):
        host, T_gt, _ = synth.cached_maps(4, 200000, family="lattice", overlap_step=0.25)
        if args.scene == "colourless":
            host = [h.copy() for h in host]
            for h in host:
                h["rgba"] = 0xFF808080
            for seed in args.seeds:
                emit(host, T_gt, seed, True, 0.0, within_one)
            return
        for seed in args.seeds:
            emit(host, T_gt, seed, True, None, within_one)
        for d in args.divisors:
            for seed in args.seeds:
                emit(host, T_gt, seed, True, params.descriptor_radius / d, within_one)
    elif args.scene == "independent":
        host, T_gt, _ = synth.cached_maps(4, 200000, overlap_step=0.25)
        for prerejective in (True, False):
            for leaf in (None, 0.0):
                for seed in args.seeds if prerejective else args.seeds[:1]:
                    emit(host, T_gt, seed, prerejective, leaf, within_one)
    else:
        import bench
        n_maps, n_points = 16, 500000
        host, T_gt, _ = bench.make_workload_gt(n_maps, n_points, cache=True, window=0.0)

        def judge(pairs, errs):
            sel = [k for k, p in enumerate(pairs)
                   if synth.window_overlap(n_maps, n_points, int(p["source_idx"]), int(p["target_idx"])) >= 0.3]
            return {"pairs_overlap_ge_0.3": len(sel), "within_0.5": int(sum(errs[k] <= 0.5 for k in sel))}
        for prerejective in (True, False):
            for leaf in (None, 0.0):
                emit(host, T_gt, args.seeds[0], prerejective, leaf, judge)


if __name__ == "__main__":
    main()
