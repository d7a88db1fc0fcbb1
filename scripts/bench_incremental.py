"""The map cache (mm3d_set_map_cache) on the reference's calling pattern: estimateMapsTransforms again and again with every
robot's latest map (R/src/map_merge_node.cpp:133-153), most of them unchanged since the last call.

Workload: 16 maps x 500 000 points from synth, 16 streams, FPFH, with SAC_IA (BASELINE.json's headline) and MATCHING (the
reference's default method).  Per method: a cold call, then calls in which k of the 16 maps changed (a one-ulp nudge of one
coordinate of one point counts as a change), k in {0, 1, 4, 16}, each `--reps` times.  Every call is checked bit for bit --
transforms, pair records, map sizes -- against a plain context (no cache) run in lock-step from the same generator state.
Under SAC_IA the generator moves on from call to call, so pairs are not reused (features are); `--srand` re-seeds both
contexts before every call, the case in which SAC_IA's pairs are reused too.

    python scripts/bench_incremental.py [--points 500000] [--maps 16] [--streams 16] [--reps 3] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--methods", default="SAC_IA,MATCHING")
    ap.add_argument("--srand", action="store_true", help="re-seed both contexts before every call")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mm = ge.load()
    from map_merge_amd import synth
    base, _, _ = synth.cached_maps(args.maps, args.points)
    out = {"workload": {"maps": args.maps, "points": args.points, "streams": args.streams, "descriptor": "FPFH",
                        "srand_each_call": bool(args.srand)}, "methods": {}}
    for method in args.methods.split(","):
        params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod[method], refine_transform=1)
        clouds = [c.copy() for c in base]
        cached, plain = mm.Context(0), mm.Context(0)
        rows = []
        try:
            for c in (cached, plain):
                c.setStreams(args.streams)
                c.srand(1)
            cached.setMapCache(args.maps * 2)
            for c in (cached, plain):                           # (warm both contexts' pools: the cold call is then a cold CACHE)
                c.estimateMapsTransforms(clouds[:2], params)
                c.srand(1)
            cached.clearMapCache()
            cached.mapCacheStats(reset=True)
            nudged = 0

            def call(label, k):
                if args.srand:
                    cached.srand(1)
                    plain.srand(1)
                t0 = time.perf_counter()
                T, pairs = cached.estimateMapsTransforms(clouds, params, return_pairs=True)
                t_cached = time.perf_counter() - t0
                sizes = cached.lastRunMapSizes()
                t0 = time.perf_counter()
                T1, pairs1 = plain.estimateMapsTransforms(clouds, params, return_pairs=True)
                t_plain = time.perf_counter() - t0
                sizes1 = plain.lastRunMapSizes()
                same = (np.array_equal(np.stack(T).view(np.uint32), np.stack(T1).view(np.uint32))
                        and np.array_equal(pairs.view(np.uint8), pairs1.view(np.uint8))
                        and all(np.array_equal(a, b) for a, b in zip(sizes, sizes1)))
                st = cached.mapCacheStats(reset=True)
                row = {"call": label, "changed_maps": k, "ms_cached": round(t_cached * 1e3, 2), "ms_plain": round(t_plain * 1e3, 2),
                       "bit_equal": bool(same), "pairs": int(len(pairs)), **st}
                rows.append(row)
                print(json.dumps({"method": method, **row}), flush=True)
                if not same:
                    raise SystemExit(f"{method} {label}: the caching context differs from the plain one")

            call("cold", args.maps)
            for k in (0, 1, 4, 16):
                for r in range(args.reps):
                    for i in range(min(k, args.maps)):      # a different map each time; one coordinate of one point, one ulp
                        m = (nudged + i) % args.maps
                        x = clouds[m]["x"]
                        x[r % len(x)] = np.nextafter(x[r % len(x)], np.float32(np.inf))
                    nudged += k
                    call(f"k{k}_rep{r}", k)
        finally:
            cached.close()
            plain.close()
        cold = rows[0]
        summary = {}
        for k in (0, 1, 4, 16):
            sel = [r for r in rows if r["call"].startswith(f"k{k}_")]
            summary[f"k{k}"] = {"ms_cached_median": float(np.median([r["ms_cached"] for r in sel])),
                                "ms_plain_median": float(np.median([r["ms_plain"] for r in sel]))}
        summary["cold_ms_cached"] = cold["ms_cached"]
        summary["cold_ms_plain"] = cold["ms_plain"]
        out["methods"][method] = {"calls": rows, "summary": summary}
    out["all_bit_equal"] = all(r["bit_equal"] for m in out["methods"].values() for r in m["calls"])
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({m: v["summary"] for m, v in out["methods"].items()}))


if __name__ == "__main__":
    main()
