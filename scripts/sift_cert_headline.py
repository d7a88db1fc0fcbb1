"""The certified SIFT octaves on the headline maps: runs the feature chain of every map once and prints
mm3d_debug_sift_cert_stats -- [0] octaves on the certified path, [1] their points, [2] points that took the exact path
(k_sift_dog_marked), [3] points left open by the first pass, [4] octaves sent back to the sorted lists, [5] bound violations,
[6] points still open after the second pass, [7] items the unsorted pass could not stage.  [4], [5] and [6] must be 0; [2] is
what a change of the exact path may not move.  EVIDENCE TOOL (GPU box):
    python3 scripts/sift_cert_headline.py [maps] [points]          (default 16 x 500000; MM3D_LIB picks another build)
Exits with status 1 when an octave was sent back, a bound was violated or a point stayed open."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
import bench  # noqa: E402

mm = ge.load()
n_maps = int(sys.argv[1]) if len(sys.argv) > 1 else 16
n_pts = int(sys.argv[2]) if len(sys.argv) > 2 else 500000
host = bench.make_workload(n_maps, n_pts)
params = mm.MapMergingParams(descriptor_type=mm.Descriptor.FPFH, estimation_method=mm.EstimationMethod.SAC_IA, refine_transform=1)
ctx = mm.Context(0)
mm.sift_cert_stats(reset=True)
total = [0] * 8
for i in range(n_maps):
    m = ctx.mapFeatures(ctx.cloud(host[i]), params)
    st = [int(v) for v in mm.sift_cert_stats(reset=True)]
    print(f"map {i:2d}: keypoints {len(m.keypoints):6d}  sift_cert_stats {st}", flush=True)
    total = [a + b for a, b in zip(total, st)]
    m.free()
ctx.close()
print(f"all {n_maps} maps: sift_cert_stats {total}")
sys.exit(0 if total[4] == 0 and total[5] == 0 and total[6] == 0 else 1)
