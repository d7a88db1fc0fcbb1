"""The two confidences of a pair record side by side (mm3d_set_confidence): the reference's 1 / transformScore and the overlap
confidence over a sweep of voxel x view_margin.  Stand-alone; bench.py is not involved.  One JSON line per row as it finishes
(the rows of profiles/confidence_overlap.jsonl).

For every pair of a scene the whole-map call runs once per seed with the reference confidence; the overlap confidence of each
swept option set is then taken at the record's transform with mm3d_transform_overlap on the maps' own points, which is the
number the whole-map call puts into the record (tests/test_gpu_confidence.py holds the two bit-equal).  A pair counts as
recovered when its transform lies within --bound (Frobenius) of the ground truth; the figure per confidence is the share of
(recovered, unrecovered) couples of pairs that the confidence ranks the right way round (a tie counts half).  No threshold is
fixed in advance.

  python scripts/bench_confidence.py                 # the lattice scene of section 7c: 4 x 200 k, overlap_step 0.25, FPFH,
                                                     # prerejective alignment, 8 streams, seeds 1 2 3
  python scripts/bench_confidence.py --headline      # the headline's 16 x 500 k independent maps, SAC-IA
  python scripts/bench_confidence.py --planted       # no estimate at all: every pair at its ground truth and at planted wrong
                                                     # poses (0.3 m, 1 m and 2 m slides, 2 and 5 degrees of yaw), both confidences
  python scripts/bench_confidence.py --timing        # ms per call, reference and overlap contexts alternating
  python scripts/bench_confidence.py --one-call      # one warm-up and one overlap call, for a kernel trace around it
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


def ranked_right(conf, recovered):
    """Share of (recovered, unrecovered) couples with conf[recovered] > conf[unrecovered]; ties count half; None without a couple."""
    good = [c for c, r in zip(conf, recovered) if r]
    bad = [c for c, r in zip(conf, recovered) if not r]
    if not good or not bad:
        return None
    score = sum(1.0 if g > b else 0.5 if g == b else 0.0 for g in good for b in bad)
    return score / (len(good) * len(bad))


def context(mm, args, prerejective, confidence=None):
    ctx = mm.Context(0)
    ctx.setStreams(args.streams)
    if prerejective:
        ctx.setAlignment(method=mm.AlignMethod.PREREJECTIVE)
    if confidence is not None:
        ctx.setConfidence(method=mm.ConfidenceMethod.OVERLAP, **confidence)
    return ctx


def sweep(mm, args, scene, host, T_gt, prerejective):
    from map_merge_amd import synth
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    rows = [(m, v) for m in args.multiples for v in args.view_margins]
    ref_conf, recovered, errors = [], [], []
    ovl_conf = {row: [] for row in rows}
    stats = {row: [] for row in rows}
    one = mm.Context(0)
    maps = [one.mapFeatures(one.cloud(x), params) for x in host]
    for seed in args.seeds:
        ctx = context(mm, args, prerejective)
        ctx.srand(seed)
        _, pairs = ctx.estimateMapsTransforms(host, params, return_pairs=True)
        ctx.close()
        for p in pairs:
            s, t = int(p["source_idx"]), int(p["target_idx"])
            T = p["transform"].reshape(4, 4).T
            err = float(np.linalg.norm(T - synth.relative_gt(T_gt[s], T_gt[t])))
            errors.append(round(err, 3))
            recovered.append(err <= args.bound)
            ref_conf.append(float(p["confidence"]))
            for row in rows:
                st = one.transformOverlap(maps[s].points, maps[t].points, T, method=mm.ConfidenceMethod.OVERLAP, voxel=row[0] * params.resolution,
                                          view_margin=row[1])
                ovl_conf[row].append(st["confidence"])
                stats[row].append([st["in_st"], st["hit_st"], st["in_ts"], st["hit_ts"]])
    base = {"scene": scene, "seeds": args.seeds, "streams": args.streams, "bound": args.bound, "pairs": len(recovered),
            "recovered": int(sum(recovered)), "errors": errors}
    print(json.dumps({**base, "row": "reference", "ranked_right": ranked_right(ref_conf, recovered),
                      "confidence": [round(c, 4) for c in ref_conf]}), flush=True)
    for row in rows:
        print(json.dumps({**base, "row": "overlap_v%gx_m%d" % row, "voxel": row[0] * params.resolution, "view_margin": row[1],
                          "ranked_right": ranked_right(ovl_conf[row], recovered), "confidence": [round(c, 4) for c in ovl_conf[row]],
                          "in_hit_st_ts": stats[row]}), flush=True)
    one.close()


def planted(mm, args, scene, host, T_gt):
    """Both confidences at poses whose quality is known by construction: the ground truth of every pair against the same pose
    slid or turned.  The reference's figure is 1 / mm3d_transform_score at max_correspondence_distance, what the pair stage computes."""
    from map_merge_amd import synth
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    one = mm.Context(0)
    maps = [one.mapFeatures(one.cloud(x), params) for x in host]

    def moved(dx=0.0, dy=0.0, yaw=0.0):
        M = np.eye(4)
        c, s = np.cos(np.radians(yaw)), np.sin(np.radians(yaw))
        M[:2, :2] = [[c, -s], [s, c]]
        M[:2, 3] = [dx, dy]
        return M
    poses = [("truth", moved()), ("slide_0.3", moved(dx=0.3)), ("slide_1", moved(dy=1.0)), ("slide_2", moved(dx=2.0)), ("yaw_2", moved(yaw=2.0)),
             ("yaw_5", moved(yaw=5.0))]
    rows = [(m, v) for m in args.multiples for v in args.view_margins]
    live = [(i, j) for i in range(len(host)) for j in range(i + 1, len(host))
            if scene != "independent_16x500k" or synth.window_overlap(16, 500000, i, j) >= 0.3]
    table = {name: {"reference": [], **{row: [] for row in rows}} for name, _ in poses}
    for s_, t_ in live:
        gt = synth.relative_gt(T_gt[s_], T_gt[t_])
        for name, M in poses:
            T = (M @ gt).astype(np.float32)
            score = one.transformScore(maps[s_].points, maps[t_].points, T, params.max_correspondence_distance)
            table[name]["reference"].append(1.0 / score)
            for row in rows:
                table[name][row].append(one.transformOverlap(maps[s_].points, maps[t_].points, T, method=mm.ConfidenceMethod.OVERLAP,
                                                             voxel=row[0] * params.resolution, view_margin=row[1])["confidence"])
    for key in ["reference"] + rows:
        label = key if key == "reference" else "overlap_v%gx_m%d" % key
        out = {"scene": scene, "mode": "planted", "row": label, "pairs": len(live)}
        for name, _ in poses:
            out["median_" + name] = round(statistics.median(table[name][key]), 4)
            if name != "truth":
                # per pair: is the truth ranked above this wrong pose of the SAME pair, and above this wrong pose of ANY pair
                same = [1.0 if a > b else 0.5 if a == b else 0.0 for a, b in zip(table["truth"][key], table[name][key])]
                out["truth_above_" + name + "_same_pair"] = round(sum(same) / len(same), 4)
                out["truth_above_" + name + "_any_pair"] = round(ranked_right(table["truth"][key] + table[name][key],
                                                                              [True] * len(live) + [False] * len(live)), 4)
        print(json.dumps(out), flush=True)
    one.close()


def timing(mm, args, scene, host, prerejective):
    """ms per call of whole-map calls, a reference context and an overlap context taking turns (neither sees a cold device)."""
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    ctxs = {"reference": context(mm, args, prerejective), "overlap": context(mm, args, prerejective, {})}
    times = {k: [] for k in ctxs}
    for rep in range(args.reps + 1):                       # (the first round warms the pools up and is not counted)
        for name in (("reference", "overlap") if rep % 2 == 0 else ("overlap", "reference")):
            ctxs[name].srand(1)
            t0 = time.perf_counter()
            ctxs[name].estimateMapsTransforms(host, params)
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, c in ctxs.items():
        c.close()
        print(json.dumps({"scene": scene, "row": "ms_per_call_" + name, "streams": args.streams, "reps": args.reps,
                          "ms_per_call_median": statistics.median(times[name][1:]), "ms_per_call": [round(t, 2) for t in times[name][1:]]}),
              flush=True)


def one_call(mm, args, host, prerejective):
    params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
    ctx = context(mm, args, prerejective, {})
    for _ in range(2):
        ctx.srand(1)
        ctx.estimateMapsTransforms(host, params)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--planted", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--multiples", type=float, nargs="*", default=[1.0, 2.0, 4.0], help="voxel side in units of params.resolution")
    ap.add_argument("--view-margins", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--bound", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--streams", type=int, default=8)
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    if args.headline:
        host, T_gt, _ = synth.cached_maps(16, 500000)
        scene, prerejective = "independent_16x500k", False
    else:
        host, T_gt, _ = synth.cached_maps(4, 200000, family="lattice", overlap_step=0.25)
        scene, prerejective = "lattice_4x200k", True
    if args.one_call:
        one_call(mm, args, host, prerejective)
    elif args.planted:
        planted(mm, args, scene, host, T_gt)
    elif args.timing:
        timing(mm, args, scene, host, prerejective)
    else:
        sweep(mm, args, scene, host, T_gt, prerejective)


if __name__ == "__main__":
    main()
