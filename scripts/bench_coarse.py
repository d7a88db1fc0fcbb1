"""The pair stage's initial estimates side by side (mm3d_set_alignment, mm3d_set_coarse_alignment): SAC-IA, the prerejective
alignment and the correlative search over a sweep of cell x yaw_steps x candidates.  Stand-alone; bench.py is not involved.
One JSON line per row as it finishes (the rows of profiles/coarse_correlative.jsonl).

  python scripts/bench_coarse.py                     # the lattice scene of section 7c: 4 x 200 k, overlap_step 0.25, FPFH,
                                                     # 8 streams, seeds 1 2 3: pairs of six within 1.0 of the truth and ms
                                                     # per call (median of --reps after a warm-up)
  python scripts/bench_coarse.py --headline          # 16 x 500 k independent maps: of the pairs with >= 30 % overlap, how
                                                     # many end within 0.5 of the truth
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


def rows_of(mm, args):
    rows = [("sac_ia_500", dict(max_iterations=500)), ("prerejective", dict(align=True))]
    for cell in args.cells:
        for steps in args.yaw_steps:
            for cand in args.candidates:
                rows.append(("correlative_c%g_y%d_k%d" % (cell, steps, cand), dict(coarse=dict(cell=cell, yaw_steps=steps, candidates=cand))))
    return rows


def run(mm, args, scene, host, T_gt, judged, bound):
    from map_merge_amd import synth
    for name, how in rows_of(mm, args):
        params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
        if "max_iterations" in how:
            params.max_iterations = how["max_iterations"]
        for seed in args.seeds:
            ctx = mm.Context(0)
            ctx.setStreams(args.streams)
            if how.get("align"):
                ctx.setAlignment(method=mm.AlignMethod.PREREJECTIVE)
            if "coarse" in how:
                ctx.setCoarseAlignment(method=mm.CoarseMethod.CORRELATIVE, **how["coarse"])
            times, pairs = [], None
            for _ in range(args.reps + 1):                 # (the first call warms the pools up and is not counted)
                ctx.srand(seed)
                t0 = time.perf_counter()
                _, pairs = ctx.estimateMapsTransforms(host, params, return_pairs=True)
                times.append((time.perf_counter() - t0) * 1e3)
            ctx.close()
            errs = {(int(p["source_idx"]), int(p["target_idx"])): float(np.linalg.norm(
                p["transform"].reshape(4, 4).T - synth.relative_gt(T_gt[int(p["source_idx"])], T_gt[int(p["target_idx"])]))) for p in pairs}
            seen = [errs[k] for k in judged if k in errs] if judged is not None else list(errs.values())
            print(json.dumps({"scene": scene, "row": name, "seed": seed, "streams": args.streams, "bound": bound,
                              "recovered": int(sum(e <= bound for e in seen)), "pairs_judged": len(seen), "pairs": len(pairs),
                              "errors": [round(e, 3) for e in seen], "ms_per_call_median": statistics.median(times[1:]),
                              "ms_per_call": [round(t, 2) for t in times[1:]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--cells", type=float, nargs="*", default=[0.25, 0.5, 1.0], help="fine cell side in metres")
    ap.add_argument("--yaw-steps", type=int, nargs="*", default=[360, 720])
    ap.add_argument("--candidates", type=int, nargs="*", default=[8, 32, 128])
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=8)
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    if args.headline:
        host, T_gt, _ = synth.cached_maps(16, 500000)
        judged = [(i, j) for i in range(16) for j in range(i + 1, 16) if synth.window_overlap(16, 500000, i, j) >= 0.3]
        run(mm, args, "independent_16x500k", host, T_gt, judged, 0.5)
    else:
        host, T_gt, _ = synth.cached_maps(4, 200000, family="lattice", overlap_step=0.25)
        run(mm, args, "lattice_4x200k", host, T_gt, None, 1.0)


if __name__ == "__main__":
    main()
