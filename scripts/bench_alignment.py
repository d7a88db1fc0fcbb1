"""SAC-IA against the prerejective alignment (mm3d_set_alignment) on the scenes whose ground truth is known: pairs recovered,
survivors per draw and ms per mm3d_estimate_maps_transforms call (median of --reps calls after a warm-up).  Stand-alone;
bench.py is only read for the headline workload.  One JSON line per configuration as it finishes.

  python scripts/bench_alignment.py                          # lattice 4 x 200 k: SAC-IA at 500 and at 20 000 hypotheses (the
                                                             # yardstick), prerejective at 2^16 .. 2^22 draws, seeds 1 2 3
  python scripts/bench_alignment.py --samples 20 --seeds 1   # one setting
  python scripts/bench_alignment.py --scene headline         # 16 x 500 k independent maps: pairs of >= 30 % overlap within 0.5
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


def run(mm, synth, host, T_gt, params, streams, seed, reps, align=None, judge=None):
    ctx = mm.Context(0)
    ctx.setStreams(streams)
    if align:
        ctx.setAlignment(method=mm.AlignMethod.PREREJECTIVE, **align)
    times, pairs = [], None
    for _ in range(reps + 1):                              # (the first call warms the pools up and is not counted)
        ctx.srand(seed)
        t0 = time.perf_counter()
        _, pairs = ctx.estimateMapsTransforms(host, params, return_pairs=True)
        times.append((time.perf_counter() - t0) * 1e3)
    errs = [float(np.linalg.norm(p["transform"].reshape(4, 4).T - synth.relative_gt(T_gt[int(p["source_idx"])], T_gt[int(p["target_idx"])])))
            for p in pairs]
    row = {"seed": seed, "ms_per_call_median": statistics.median(times[1:]) if reps else times[0], "pairs": len(pairs)}
    row.update(judge(pairs, errs))
    if align:                                              # the survivors of one pair, through the stage call
        one = mm.Context(0)
        one.srand(seed)
        maps = [one.mapFeatures(one.cloud(x), params) for x in host[:2]]
        _, st = one.estimateTransformPrerejective(maps[0].keypoints, maps[0].descriptors, maps[1].keypoints, maps[1].descriptors,
                                                  params.max_correspondence_distance,
                                                  mm.AlignmentOptions(method=mm.AlignMethod.PREREJECTIVE, **align))
        row["pair_0_1"] = st
        row["survivors_per_draw"] = st["survivors"] / max(st["draws"], 1)
        one.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("lattice", "headline"), default="lattice")
    ap.add_argument("--samples", type=int, nargs="*", default=[16, 18, 20, 22], help="log2 of the draws")
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--skip-sac-ia", action="store_true")
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    if args.scene == "lattice":
        n_maps, n_points = 4, 200000
        host, T_gt, _ = synth.cached_maps(n_maps, n_points, family="lattice", overlap_step=0.25)

        def judge(pairs, errs):
            return {"recovered_within_1.0": int(sum(e <= 1.0 for e in errs)), "errors": [round(e, 3) for e in errs]}
    else:
        import bench
        n_maps, n_points = 16, 500000
        host, T_gt, _ = bench.make_workload_gt(n_maps, n_points, cache=True, window=0.0)

        def judge(pairs, errs):
            sel = [k for k, p in enumerate(pairs)
                   if synth.window_overlap(n_maps, n_points, int(p["source_idx"]), int(p["target_idx"])) >= 0.3]
            return {"pairs_overlap_ge_0.3": len(sel), "within_0.5": int(sum(errs[k] <= 0.5 for k in sel))}
    if not args.skip_sac_ia:
        for it in (500, 20000) if args.scene == "lattice" else (500,):
            params.max_iterations = it
            print(json.dumps({"scene": args.scene, "method": "sac_ia", "max_iterations": it,
                              **run(mm, synth, host, T_gt, params, args.streams, 1, args.reps, None, judge)}), flush=True)
    params.max_iterations = 500
    for lg in args.samples:
        for seed in args.seeds:
            print(json.dumps({"scene": args.scene, "method": "prerejective", "log2_samples": lg,
                              **run(mm, synth, host, T_gt, params, args.streams, seed, args.reps, dict(samples=1 << lg), judge)}),
                  flush=True)


if __name__ == "__main__":
    main()
