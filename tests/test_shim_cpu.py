"""The reference-side binding (include/map_merge_3d_shim.hpp) is a complete, linkable
replacement for R/src/{features,matching,map_merging,graph}.cpp.

This image has no PCL / ROS / Eigen, so the shim is compiled against the reference's own public headers
(read where they lie) plus the declaration-only stand-ins of tests/shim/mock: a syntax, signature and
link check (every function the reference's headers declare -- including MapMergingParams::fromCommandLine,
::fromROSNode and operator<<, R/src/map_merging.cpp:10-123 -- is defined, nothing is undefined against
libmm3d.so), and the reference's five gtest cases (R/test/test_map_merging.cpp), which need no device.
It pins nothing numerically.  The program and its object file are what __graft_entry__.build() made under oracle/_ref/
(tests/shim/build.sh, where the reference's headers could be read); the tests read nothing outside the tree."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BUILD = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(REF_BUILD, "shim_check")
OBJ = os.path.join(REF_BUILD, "shim_check.o")


@pytest.fixture(scope="module")
def shim_check(mm):
    if not os.path.exists(EXE):
        pytest.skip("no shim_check: the reference's headers were not readable when the tree was built")
    return EXE


def test_shim_compiles_links_and_passes_the_reference_gtests(shim_check):
    r = subprocess.run([shim_check, "cpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "shim_check cpu: ok" in r.stdout, r.stdout + r.stderr


def test_every_declared_function_is_defined_exactly_once(shim_check):
    """The symbols a caller of the reference's headers can reference (map_merge_node.cpp:16-25,141-142,
    map_merge_tool.cpp:22-49, registration_visualisation.cpp:52-162) are all defined by the shim TU."""
    assert os.path.exists(OBJ), "oracle/_ref/shim_check.o is missing beside shim_check: rebuild the tree"
    nm = subprocess.run(["nm", "-C", "--defined-only", OBJ], capture_output=True, text=True).stdout
    for name in ("map_merge_3d::downSample(", "map_merge_3d::removeOutliers(", "map_merge_3d::computeSurfaceNormals(",
                 "map_merge_3d::detectKeypoints(", "map_merge_3d::computeLocalDescriptors(",
                 "map_merge_3d::findFeatureCorrespondences(", "map_merge_3d::estimateTransformFromCorrespondences(",
                 "map_merge_3d::estimateTransformFromDescriptorsSets(", "map_merge_3d::estimateTransformICP(",
                 "map_merge_3d::estimateTransform(", "map_merge_3d::transformScore(", "map_merge_3d::estimateMapsTransforms(",
                 "map_merge_3d::composeMaps(", "map_merge_3d::MapMergingParams::fromCommandLine(",
                 "map_merge_3d::MapMergingParams::fromROSNode(", "map_merge_3d::operator<<(std::ostream&, map_merge_3d::MapMergingParams const&)"):
        hits = [l for l in nm.splitlines() if " T " in l and name in l]
        assert len(hits) == 1, (name, hits)
