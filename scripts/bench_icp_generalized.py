"""Generalized ICP (mm3d_set_icp_generalized) measured: accuracy and call time of whole-map calls with the selection inactive,
with point-to-plane ICP and with generalized ICP.  Stand-alone; bench.py is not involved.  One JSON line per row as it finishes,
appended to profiles/icp_generalized.jsonl with --append.

The scene is the lattice scene of DESIGN.md section 7c: 4 x 200 k points, overlap_step 0.25, FPFH, prerejective alignment,
8 streams, seeds 1 2 3.  A pair counts as recovered when its transform lies within --bound (Frobenius) of the ground truth.

  python scripts/bench_icp_generalized.py              # accuracy: pairs recovered, median final error, ICP iteration histogram
  python scripts/bench_icp_generalized.py --timing     # ms per call: the inactive, the point-to-plane and the generalized context
                                                       # take turns in one process, --reps timed calls each after a warm-up round
  python scripts/bench_icp_generalized.py --one-call   # one warm-up and one call of --row, for a kernel trace around them
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
    ("point_to_plane", dict(icp_method=1)),
    ("generalized_1e-3", dict(enabled=1)),
])


def context(mm, args, options):
    ctx = mm.Context(0)
    ctx.setStreams(args.streams)
    ctx.setAlignment(method=mm.AlignMethod.PREREJECTIVE)
    if "icp_method" in options:
        ctx.setIcpMethod(options["icp_method"])
    elif options:
        ctx.setIcpGeneralized(**options)
    return ctx


def emit(args, row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(os.path.join(ROOT, "profiles", "icp_generalized.jsonl"), "a") as f:
            f.write(line + "\n")


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
    """The inactive context runs the machine code the library had before the selection existed: it is the baseline.  The three
    contexts take turns, the order reversed every other round."""
    ctxs = collections.OrderedDict((name, context(mm, args, options)) for name, options in ROWS.items())
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
        emit(args, {"scene": scene, "row": "ms_per_call_" + k, "streams": args.streams, "reps": args.reps,
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
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--row", default="generalized_1e-3", choices=list(ROWS))
    ap.add_argument("--append", action="store_true", help="also append the rows to profiles/icp_generalized.jsonl")
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--bound", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--streams", type=int, default=8)
    args = ap.parse_args()
    mm = ge.load()
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
