"""ICP source sampling (mm3d_set_icp_sampling) measured: a point-to-plane ICP call on a 500 k-point source against its target with
every source point, and with a normal-space or strided sample of a quarter and of a tenth of them; and the time to make a sample.
Stand-alone; bench.py is not involved.  One JSON line per row as it finishes, appended to profiles/icp_sample.jsonl with --append.

The scene: two maps of the independent synthetic family, 500 000 raw points each at overlap_step 0.5, their normals at
normal_radius 0.6; the guess is the ground truth moved by 0.1 m and one degree; max correspondence distance 1.0, at most 30
iterations, epsilon 1e-9, so a call runs several iterations.

  python scripts/bench_icp_sample.py                   # every row, --reps timed calls each after one warm-up call, in turns
  MM3D_LIB=/path/to/another/libmm3d.so python scripts/bench_icp_sample.py
                                                       # the same calls on another build of the library: a build without the stage
                                                       # runs the full-cloud row only ("library": what was loaded)
  python scripts/bench_icp_sample.py --one-call --row normal_space_0.1     # one warm-up and one call, for a kernel trace
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

NONE, STRIDE, NORMAL_SPACE = 0, 1, 2
ROWS = collections.OrderedDict([
    ("full", None),
    ("normal_space_0.25", dict(method=NORMAL_SPACE, fraction=0.25)),
    ("normal_space_0.1", dict(method=NORMAL_SPACE, fraction=0.1)),
    ("stride_0.25", dict(method=STRIDE, fraction=0.25)),
    ("stride_0.1", dict(method=STRIDE, fraction=0.1)),
])
ICP = dict(max_corr=1.0, max_iter=30, eps=1e-9)


def emit(args, row):
    row = dict(row, library=os.environ.get("MM3D_LIB") or "tree", label=args.label)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(os.path.join(ROOT, "profiles", "icp_sample.jsonl"), "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--row", default="normal_space_0.1", choices=list(ROWS))
    ap.add_argument("--append", action="store_true", help="also append the rows to profiles/icp_sample.jsonl")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    host, T_gt, _ = synth.cached_maps(2, args.points, overlap_step=0.5)
    has_stage = hasattr(mm.lib(), "mm3d_sample_icp_source")
    rows = [k for k in ROWS if has_stage or ROWS[k] is None]
    c = mm.Context(0)
    src, tgt = c.cloud(host[0]), c.cloud(host[1])
    s_nrm, t_nrm = c.computeSurfaceNormals(src, 0.6), c.computeSurfaceNormals(tgt, 0.6)
    T_true = synth.relative_gt(T_gt[0], T_gt[1])
    a = np.radians(1.0)
    off = np.eye(4)
    off[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    off[:3, 3] = [0.06, -0.07, 0.04]
    guess = (off @ T_true).astype(np.float32)
    scene = "independent_2x%dk" % (args.points // 1000)

    def call(name):
        o = ROWS[name]
        t0 = time.perf_counter()
        if o is None:
            T = c.estimateTransformICPPlane(src, tgt, t_nrm, guess, ICP["max_corr"], ICP["max_iter"], ICP["eps"])
        else:
            T = c.estimateTransformICPSampled(src, s_nrm, tgt, t_nrm, guess, ICP["max_corr"], max_iterations=ICP["max_iter"],
                                              transformation_epsilon=ICP["eps"], **o)
        return (time.perf_counter() - t0) * 1e3, T

    if args.one_call:
        call(args.row)
        call(args.row)
        c.close()
        return
    times = {k: [] for k in rows}
    last = {}
    for rep in range(args.reps + 1):                   # (the first round builds the clouds' search structures and is not counted)
        for k in (rows if rep % 2 == 0 else rows[::-1]):
            ms, T = call(k)
            times[k].append(ms)
            last[k] = (T, c.last_icp_iterations, c.last_icp_converged, c.lastIcpSamplingStats() if has_stage and ROWS[k] else None)
    for k in rows:
        ms = times[k][1:]
        T, it, conv, st = last[k]
        emit(args, {"scene": scene, "row": "icp_plane_" + k, "options": ROWS[k], "icp": ICP, "reps": args.reps, "source_points": len(src),
                    "searched_points": st["sampled"] if st else len(src), "iterations": it, "converged": conv,
                    "error_to_ground_truth": round(float(np.linalg.norm(T - T_true)), 5),
                    "ms_per_call_median": round(statistics.median(ms), 3), "ms_per_call_min": round(min(ms), 3),
                    "ms_per_call_max": round(max(ms), 3), "ms_per_iteration_median": round(statistics.median(ms) / max(it, 1), 3)})
    if has_stage:
        # the sample alone (what mm3d_map_prepare pays once per map, before the sample's query order), and the ICP on that fresh
        # sample (its query order included)
        for k in rows:
            if ROWS[k] is None:
                continue
            build, icp = [], []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                sample, _ = c.sampleIcpSource(src, s_nrm, indices=False, **ROWS[k])
                t1 = time.perf_counter()
                c.estimateTransformICPPlane(sample, tgt, t_nrm, guess, ICP["max_corr"], ICP["max_iter"], ICP["eps"])
                t2 = time.perf_counter()
                build.append((t1 - t0) * 1e3)
                icp.append((t2 - t1) * 1e3)
            emit(args, {"scene": scene, "row": "sample_build_" + k, "options": ROWS[k], "reps": args.reps, "source_points": len(src),
                        "sampled_points": len(sample), "build_ms_median": round(statistics.median(build[1:]), 3),
                        "build_ms_min": round(min(build[1:]), 3), "build_ms_max": round(max(build[1:]), 3),
                        "icp_on_fresh_sample_ms_median": round(statistics.median(icp[1:]), 3)})
    c.close()


if __name__ == "__main__":
    main()
