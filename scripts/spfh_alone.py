"""`spfh` alone on the GPU: the launches of headline maps 0 and 1 on one stream (what bench.py's kernel_bounds_isolated times), REPS times
over, for the library MM3D_LIB selects -- one line: label, launches, average and smallest launch in microseconds.  For the A/B of the
-DMM3D_SPFH_* builds.
    MM3D_LIB=<libmm3d_x.so> scripts/spfh_alone.py <label> [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
import bench
mm = ge.load()
label = sys.argv[1] if len(sys.argv) > 1 else "base"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
host = bench.make_workload(16, 500000)
ctx = mm.Context(0)
P = mm.MapMergingParams(descriptor_type=2, estimation_method=1)
per_rep = []
for rep in range(REPS + 1):                     # (the first round warms the pools up)
    ctx.profile_reset(); ctx.profile(True)
    for i in (0, 1):
        m = ctx.mapFeatures(ctx.cloud(host[i]), P)
        m.free()
    ctx.synchronize(); ctx.profile(False)
    e = ctx.profile_entries()["spfh"]
    if rep:
        per_rep.append(1e3 * e["ms"] / e["launches"])
print("%-8s spfh launches per round %d  avg_launch_us %.1f  min %.1f  max %.1f  (rounds: %s)"
      % (label, e["launches"], sum(per_rep) / len(per_rep), min(per_rep), max(per_rep), " ".join("%.1f" % v for v in per_rep)))
