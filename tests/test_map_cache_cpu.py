"""The map cache of mm3d_estimate_maps_transforms (mm3d_set_map_cache) without a GPU: its four entry points are declared and
exported and behave on a NULL context, and the cache's HOST code -- map_cache.cpp and the drivers that use it (driver_streams.cpp) --
runs under ThreadSanitizer and AddressSanitizer + UBSan on the fake HIP runtime and fake device layer of tests/host_san
(tests/host_san_cache: repeats, changed, reordered and evicted maps, parameter changes, SAC_IA with and without srand, calls
that fail half-way; every call bit-equal to a plain context, the counters exact)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang++")
NAMES = ("mm3d_set_map_cache", "mm3d_get_map_cache", "mm3d_map_cache_clear", "mm3d_map_cache_stats")


def test_entry_points_are_declared_and_exported(mm):
    hdr = open(os.path.join(ROOT, "include", "mm3d.h")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    L = mm.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    # the header says what the cache is, what it keys on and what it costs
    comment = " ".join(re.findall(r"/\*.*?\*/", hdr, flags=re.S))
    for words in ("Feature / pair cache", "byte for byte", "SAC_IA", "mm3d_srand", "16 B per point", "MM3D_EUNSUPPORTED"):
        assert words in comment, words


def test_null_context(mm):
    L = mm.lib()
    out = (C.c_longlong * 6)()
    assert L.mm3d_set_map_cache(None, 4) == -1
    assert L.mm3d_set_map_cache(None, 0) == -1
    assert L.mm3d_get_map_cache(None) == 0
    assert L.mm3d_map_cache_stats(None, out, 0) == -1
    L.mm3d_map_cache_clear(None)                     # does nothing, does not crash


def test_python_mirror(mm):
    for name in ("setMapCache", "getMapCache", "clearMapCache", "mapCacheStats", "lastRunMapSizes"):
        assert callable(getattr(mm.Context, name, None)), name


def test_shim_reads_the_environment():
    shim = open(os.path.join(ROOT, "include", "map_merge_3d_shim.hpp")).read()
    assert "MM3D_MAP_CACHE" in shim and "mm3d_set_map_cache" in shim


@pytest.mark.parametrize("kind", ["thread", "address"])
def test_map_cache_host_code_under_sanitizer(kind):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang with HIP support here")
    subprocess.check_call([os.path.join(HERE, "host_san_cache", "build.sh"), kind], stdout=subprocess.DEVNULL)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("MM3D_FEATURE_WORKERS", None)
    env.pop("MM3D_FAKE_DIGEST_FAIL_POINTS", None)
    r = subprocess.run([os.path.join(HERE, "host_san_cache", "_build", "san_" + kind)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "map cache host driver ok" in r.stdout
    for word in ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-6000:]
