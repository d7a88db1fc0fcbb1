"""Consistency-graph estimation (mm3d_set_estimator) measured: stand-alone calls of mm3d_estimate_transform_consistency beside
mm3d_estimate_transform_from_correspondences (the reference's RANSAC) on the scene of tests/consistency_cases.py.  Stand-alone;
bench.py is not involved.  One JSON line per row as it finishes, appended to profiles/consistency.jsonl with --append.

  python scripts/bench_consistency.py                 # ms per call at C = 1 500 and C = 15 000, the two estimators taking turns in
                                                      # one process, --reps timed calls each after a warm-up round; true inliers held
  python scripts/bench_consistency.py --one-call C    # one warm-up and --calls calls of the consistency estimator at C
                                                      # correspondences, for a kernel trace around them
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
from consistency_cases import THRESHOLD, identity_corr, points, scene  # noqa: E402


def emit(args, row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(os.path.join(ROOT, "profiles", "consistency.jsonl"), "a") as f:
            f.write(line + "\n")


def inputs(mm, ctx, n, share):
    p, q, inl, _, _ = scene(1, n, share)
    return ctx.cloud(points(p, mm.POINT)), ctx.cloud(points(q, mm.POINT)), identity_corr(n, mm.CORR), inl


def timing(mm, args):
    ctx = mm.Context(0)
    for n in args.sizes:
        s, t, corr, inl = inputs(mm, ctx, n, args.share)
        calls = {"consistency": lambda: ctx.estimateTransformConsistency(s, t, corr, THRESHOLD)[1],
                 "ransac": lambda: ctx.estimateTransformFromCorrespondences(s, t, corr, THRESHOLD)[1]}
        times, held = {k: [] for k in calls}, {}
        for rep in range(args.reps + 1):               # (the first round warms the pools up and is not counted)
            for k in (list(calls) if rep % 2 == 0 else list(calls)[::-1]):
                t0 = time.perf_counter()
                found = calls[k]()
                times[k].append((time.perf_counter() - t0) * 1e3)
                held[k] = (int(inl[found["index_query"]].sum()), len(found))
        for k in calls:
            ms = times[k][1:]
            emit(args, {"row": "ms_per_call_" + k, "correspondences": n, "share": args.share, "true_inliers": int(inl.sum()),
                        "held": held[k][0], "returned": held[k][1], "reps": args.reps, "ms_per_call_median": round(statistics.median(ms), 3),
                        "ms_per_call_min": round(min(ms), 3), "ms_per_call_max": round(max(ms), 3)})
    ctx.close()


def one_call(mm, args):
    ctx = mm.Context(0)
    s, t, corr, _ = inputs(mm, ctx, args.one_call, args.share)
    for _ in range(1 + args.calls):
        ctx.estimateTransformConsistency(s, t, corr, THRESHOLD)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-call", type=int, default=0, metavar="C")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1500, 15000])
    ap.add_argument("--share", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--append", action="store_true", help="also append the rows to profiles/consistency.jsonl")
    args = ap.parse_args()
    mm = ge.load()
    if args.one_call:
        one_call(mm, args)
    else:
        timing(mm, args)


if __name__ == "__main__":
    main()
