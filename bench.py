#!/usr/bin/env python3
"""bench.py -- map-pairs/sec of the registration hot path on MI355X (BASELINE.json metric).

One "step" = one full estimateMapsTransforms over the workload: per-map features (voxel grid ->
outlier filter -> normals -> SIFT keypoints -> FPFH), every map pair (SAC-IA -> ICP -> score) and
the pose graph, with the raw clouds already resident in HBM when the timed region starts.

  python bench.py --gpus 1 --steps 2 --warmup 1                       # N = 1
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W        # N > 1, one rank per GPU

N > 1: strong scaling of the SAME job, driven from inside the library (mm3d_shard_*).  A rank computes
the features of the maps it owns, ONE all-gather (RCCL) hands every rank all feature bundles, a rank
estimates the pairs whose TARGET it owns (so it builds target-side search structures for 16 / N maps
only), the pair records are all-gathered (RCCL) and every rank solves the pose graph.  Every rank
replays the rand() draws of all pairs, so the stream matches the reference's single global one.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times
--steps steps and prints the headline (`value`, `ms_per_step`) with what the steps themselves report
(pair-transform CRC, stage seconds of the last step, host CPU).  `--full` adds everything that takes
work of its own: `roofline` (dominant kernel, HIP-event timed on the engine's own stream; the kernels
are bracketed with events only then), the isolated per-kernel pass, the pair stage alone, the
PCIe-inclusive steps, the ground-truth error and, at N = 1, `cpu_baseline` (the CPU oracle, single
thread like the reference, on a bounded sample of the same workload) with its `parity_check`.

`--dump-outputs DIR` writes what the last timed step returned (the global transforms and the pair
records, field by field) as DIR/<name>.npy, so that two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import sys
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_F32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense f32-input MFMA (v_mfma_f32_32x32x2_f32)
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16), measured 2495
# kernels whose profile "bytes" field carries the FLOPs they execute (csrc/desc_knn.hip), and the matrix peak they run against:
# the f32 selector on the f32 cores, the split-bf16 selector of the wide rows (three bf16 products per float product) on the bf16 ones
MFMA_KERNELS = {"desc_knn_mfma": MFMA_F32_PEAK_TFLOPS, "desc_knn_mfma_bf16": MFMA_BF16_PEAK_TFLOPS}
# VALU issue peak, wave-instructions per second over the chip.  MEASURED: independent v_fma_f32 streams at 4 and 8 waves per
# SIMD on all 256 CUs sustain 8.4e11 (scripts/micro/valu_rate.hip, profiles/r04_valu_rate.txt; v_add_f32 / v_mul_f32 /
# integer adds and logic 6.5 - 8.3e11; v_max / v_cvt / shifts / v_mbcnt / packed f32 / DPP adds / f64 4.2 - 5.0e11;
# v_exp / v_rcp / v_sqrt 2.9e11).  NOMINAL by the guide's table (MI355X_MICROARCH.md: v_fma_f32 2 cycles per wave64 on a
# SIMD-32): 256 x 4 x 2.4e9 / 2 = 1.23e12, which the chip does not sustain -- the all-VALU loop clocks down as its waves
# per SIMD go up and the rate stays at 8.4e11.  Round 3 used 6.14e11 (4 cycles per instruction): 27 % too low.
VALU_PEAK_WINSTR_S = 8.4e11
VALU_PEAK_NOMINAL_WINSTR_S = 256 * 4 * 2.4e9 / 2
# profile name (MM3D_LAUNCH) of the kernels whose C++ symbol differs from it (scripts/pmc_summary.py prints symbols)
KERNEL_OF_SYMBOL = {"k_sift_dog_lds": "sift_dog", "k_sift_dog_lds_dense": "sift_dog_dense", "k_sift_dog_lds_exact": "sift_dog_exact", "k_normals_lds": "normals_radius", "k_sift_dog": "sift_dog_big", "k_spfh": "spfh", "k_normals": "normals_radius_big",
                    "k_nn_wave<0>": "icp_corr_reduce", "k_nn_wave<1>": "score_nn_reduce", "k_sacia_err": "sacia_err", "k_sacia_exact": "sacia_seq_sum", "k_sacia_select": "sacia_select", "k_sift_dog_fast": "sift_dog_fast", "k_sift_reject": "sift_reject",
                    "k_sift_extrema_one": "sift_extrema_one",
                    "k_fpfh_weight": "fpfh_weight", "k_knn_mfma": "desc_knn_mfma", "k_knn_mfma_wide_bf": "desc_knn_mfma_bf16", "k_knn_rerank": "desc_knn_rerank",
                    "k_radius_count": "radius_outlier_count"}


# The PMC / SQ figures under profiles/ carry a hash of each kernel's MACHINE CODE as it was when the counters were collected
# (scripts/assemble_profiles.py; kernel_source_hash below); a figure whose kernel has changed since is reported with
# "stale": true instead of passing for a measurement of the code that ran.


# registration_visualisation's stage boundaries (R/src/registration_visualisation.cpp:51-158): which stage a kernel's
# time belongs to.  PCL builds a kd-tree inside each of its stages; here the grids / Hilbert orders / scans are shared
# between stages and cached, so they are their own line.
STAGE_OF_PREFIX = [("voxel", "downSample"), ("radius_outlier", "removeOutliers"), ("compact", "removeOutliers"),
                   ("normals", "computeSurfaceNormals"), ("fill_nan", "computeSurfaceNormals"), ("sift", "detectKeypoints"),
                   ("fpfh", "computeLocalDescriptors"), ("spfh", "computeLocalDescriptors"), ("pfh", "computeLocalDescriptors"),
                   ("shot", "computeLocalDescriptors"), ("desc_knn", "estimateTransform: initial (k-NN + SAC-IA | RANSAC)"),
                   ("sacia", "estimateTransform: initial (k-NN + SAC-IA | RANSAC)"), ("ransac", "estimateTransform: initial (k-NN + SAC-IA | RANSAC)"),
                   ("icp", "estimateTransform: ICP"), ("score", "transformScore")]


def stage_of(kernel):
    for pre, st in STAGE_OF_PREFIX:
        if kernel.startswith(pre):
            return st
    return "search structures (grids, Hilbert order, scans, sorts)"


# The PMC / SQ counters under profiles/ are per-launch figures of ONE workload (scripts/profile_round.sh: the headline maps,
# 500 000 raw points each, FPFH + SAC_IA, 'independent' scenes, default resolution / window / hypotheses).  A launch on
# another workload does other work: the figures are only used when the running workload is the counted one (round 4 printed
# VALU "fractions" of 1.40 on 64 x 50 k by dividing the headline's instructions by a 50 k-point launch's time).
COUNTERS_WORKLOAD_DEFAULT = {"points": 500000, "descriptor": "FPFH", "method": "SAC_IA", "scenes": "independent", "window": 0.0,
                             "resolution": 0.0, "sac_iterations": 0}


def workload_signature(args):
    return {"points": int(args.points), "descriptor": args.descriptor, "method": args.method, "scenes": args.scenes,
            "window": float(args.window), "resolution": float(args.resolution), "sac_iterations": int(args.sac_iterations)}


# Which device functions a profile name stands for (the names MM3D_LAUNCH gives its kernels -> the kernels' symbols in the
# gfx950 code objects of libmm3d.so).  The staleness hash below covers these symbols' machine code.
KERNEL_SYMBOLS = {
    "sift_dog": r"k_sift_dog_lds", "sift_dog_exact": r"k_sift_dog_lds", "sift_dog_fast": r"k_sift_dog_fast", "sift_reject": r"k_sift_reject",
    "sift_extrema_one": r"k_sift_extrema_one", "normals_radius": r"k_normals_lds", "spfh": r"k_spfh", "fpfh_weight": r"k_fpfh_weight",
    "fpfh_mark": r"k_fpfh_mark", "icp_corr_reduce": r"k_nn_waveILi0", "score_nn_reduce": r"k_nn_waveILi1", "sacia_err": r"k_sacia_err",
    "sacia_seq_sum": r"k_sacia_exact", "sacia_select": r"k_sacia_select", "desc_knn_mfma": r"k_knn_(mfma|filter)", "desc_knn_mfma_bf16": r"k_knn_mfma_wide_bf", "desc_knn_rerank": r"k_knn_rerank",
    "radius_outlier_count": r"k_radius_count", "voxel_centroid": r"k_voxel_centroid",
}
_ISA_CACHE = {}


def _device_kernels(lib_path):
    """{symbol name: machine code bytes} of every kernel in the gfx950 code objects of a HIP shared library, read with nothing
    but struct: the .so carries one clang offload bundle per translation unit, each bundle a gfx950 ELF whose .symtab lists
    the kernels as FUNC symbols inside .text."""
    import struct
    if lib_path in _ISA_CACHE:
        return _ISA_CACHE[lib_path]
    out = {}
    try:
        data = open(lib_path, "rb").read()
    except OSError:
        _ISA_CACHE[lib_path] = out
        return out
    magic, pos = b"__CLANG_OFFLOAD_BUNDLE__", 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            break
        pos = i + len(magic)
        try:
            (n_ent,) = struct.unpack_from("<Q", data, i + 24)
            off = i + 32
            for _ in range(n_ent):
                o, sz, ts = struct.unpack_from("<QQQ", data, off)
                off += 24
                triple = data[off:off + ts].decode("ascii", "replace")
                off += ts
                if "gfx950" not in triple or sz == 0:
                    continue
                elf = data[i + o:i + o + sz]
                if elf[:4] != b"\x7fELF":
                    continue
                shoff, = struct.unpack_from("<Q", elf, 0x28)
                shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
                secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
                for sec in secs:
                    if sec[1] != 2:                    # SHT_SYMTAB
                        continue
                    strtab = secs[sec[6]]
                    for k in range(sec[5] // 24):
                        name_off, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, sec[4] + k * 24)
                        if (info & 0xF) != 2 or size == 0 or shndx == 0 or shndx >= shnum:    # STT_FUNC, defined
                            continue
                        end = elf.index(b"\0", strtab[4] + name_off)
                        name = elf[strtab[4] + name_off:end].decode("ascii", "replace")
                        tsec = secs[shndx]
                        start = tsec[4] + (value - tsec[3])
                        out[name] = elf[start:start + size]
        except (struct.error, ValueError, IndexError):
            continue
    _ISA_CACHE[lib_path] = out
    return out


def kernel_source_hash(kernel):
    """What makes a committed counter stale: sha256 over the MACHINE CODE of the kernel's device functions as libmm3d.so
    carries them (None for kernels without an entry in KERNEL_SYMBOLS, or when the library cannot be read).  Round 5 hashed
    the source files with their include closure, and a comment edited in include/mm3d.h turned every counter of the round
    stale; the code object does not change with a comment."""
    import hashlib
    import re
    pat = KERNEL_SYMBOLS.get(kernel)
    if not pat:
        return None
    lib = os.environ.get("MM3D_LIB") or os.path.join(ROOT, "map-merge_amd", "libmm3d.so")
    ks = _device_kernels(lib)
    rx = re.compile(pat)
    names = sorted(n for n in ks if rx.search(n))
    if not names:
        return None
    h = hashlib.sha256()
    for n in names:
        h.update(n.encode())
        h.update(ks[n])
    return h.hexdigest()[:16]


def cgroup_cpu_limit():
    """CPUs this process may use at a time (cgroup v2 cpu.max quota / period), None if unlimited or unknown."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(int(q) / int(p), 2)
    except Exception:
        return None


def cgroup_throttle():
    """Microseconds this cgroup's threads have spent throttled by the CPU quota so far (0 if unknown)."""
    try:
        for line in open("/sys/fs/cgroup/cpu.stat"):
            if line.startswith("throttled_usec"):
                return int(line.split()[1])
    except Exception:
        pass
    return 0


def make_workload_gt(n_maps, n_points, cache=True, scenes="independent", overlap_step=0.5, window=0.0):
    """The synthetic maps as packed records plus their ground-truth poses.  scenes: 'independent' = every map draws its
    own surface samples (synth.synth_map; the headline workload), 'lattice' = the maps share the samples of one
    world-anchored lattice (synth.lattice_map)."""
    from map_merge_amd import synth
    kw = {} if overlap_step == 0.5 else {"overlap_step": overlap_step}
    if window > 0:
        kw["window"] = window
    return synth.cached_maps(n_maps, n_points, cache_dir="/tmp" if cache else None, family=scenes, **kw)


def make_workload(n_maps, n_points, cache=True):
    """The maps of the headline scene family as packed records (the scripts under scripts/ use this)."""
    return make_workload_gt(n_maps, n_points, cache=cache)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cache", action="store_true")
    ap.add_argument("--streams", type=int, default=16, help="contexts (HIP stream + host thread) per GPU")
    ap.add_argument("--engine", choices=["library", "shard", "python", "devices"], default="library",
                    help="one GPU only: 'library' = one mm3d_estimate_maps_transforms call, streams inside libmm3d; "
                         "'shard' = the N > 1 driver (mm3d_shard_*: what several ranks always use) on one rank; "
                         "'python' = the shardable pieces driven from Python threads (diagnostic); "
                         "'devices' = ONE process (launch without torchrun), --gpus N devices behind the one mm3d_estimate_maps_transforms "
                         "call (mm3d_create_devices: sharded inside the library, pair records through an in-library RCCL all-gather) -- "
                         "what the reference's single-process callers get; MM3D_BENCH_DEVICES=0,0 overrides the list (test hook)")
    ap.add_argument("--feature-streams", type=int, default=6,
                    help="one GPU only: pipeline the stages, this many streams extract features (0 = two barriered stages)")
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="diagnostic: do not bracket kernels with HIP events in the timed region (no roofline then)")
    ap.add_argument("--descriptor", choices=["FPFH", "PFH", "SHOT"], default="FPFH")
    ap.add_argument("--method", choices=["SAC_IA", "MATCHING"], default="SAC_IA")
    ap.add_argument("--host-input", choices=["none", "pcl32"], default="none",
                    help="diagnostic (one GPU, library engine): hand the clouds over as HOST arrays of pcl::PointXYZRGB records "
                         "(stride 32, rgba at 16) like the reference's callers do, so that the step includes the upload; "
                         "never the reported configuration (inputs are HBM-resident for `value`)")
    ap.add_argument("--kernel-table", default=None, help="write rank 0's full per-kernel HIP-event table (CSV) here (implies --full)")
    ap.add_argument("--scenes", choices=["independent", "lattice"], default="independent",
                    help="synthetic scene family: 'independent' (default, the headline workload: every map samples the world on its own) "
                         "or 'lattice' (overlapping maps share the samples of one world-anchored lattice: repeatable keypoints)")
    ap.add_argument("--overlap-step", type=float, default=0.5,
                    help="distance between consecutive map windows in window sides (0.5 = about half of a window shared)")
    ap.add_argument("--sac-iterations", type=int, default=0, help="MapMergingParams.max_iterations (0 = the reference's default, 500)")
    ap.add_argument("--window", type=float, default=0.0, help="side of a map's window in metres (0 = 60 m at 500 k points, constant raw density)")
    ap.add_argument("--resolution", type=float, default=0.0, help="MapMergingParams.resolution (0 = the reference's default 0.1; the radii keep their defaults, "
                    "as with the reference's --resolution option)")
    ap.add_argument("--no-pair-stage", action="store_true", help="skip the untimed pair-loop-alone pass (pair_stage_pairs_per_s) at N = 1")
    ap.add_argument("--no-pcie", action="store_true", help="skip the extra PCIe-inclusive step (host pcl::PointXYZRGB input) at N = 1")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: kernel events in the timed steps (roofline, per-kernel and per-stage figures), the "
                         "isolated per-kernel pass, the pair stage alone, the PCIe-inclusive steps, the ground-truth error and the CPU "
                         "baselines with their parity check (the --no-* options above switch single ones off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (global transforms, pair records) as DIR/<name>.npy")
    args = ap.parse_args()
    args.full = args.full or bool(args.kernel_table)
    if args.dump_outputs and args.steps < 1:
        ap.error("--dump-outputs writes what the last timed step computed: it needs --steps 1 or more")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("MM3D_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    backend = os.environ.get("MM3D_BENCH_BACKEND", "nccl")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (test knobs: MM3D_BENCH_BACKEND=gloo MM3D_BENCH_DEVICE=0 run several ranks on ONE GPU to exercise
        # the exchange / gather code where only a single-GPU box is available)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)
    if world == 1 and args.gpus > 1 and args.engine != "devices":
        # `python bench.py --gpus N` WITHOUT torchrun: one process, N devices -- the library's own multi-device driver
        # (mm3d_create_devices: maps by owner, peer copies, pairs by target owner, ONE in-library ncclAllGather), never a silent
        # one-GPU run under an N-GPU label.  (Under torchrun -- WORLD_SIZE = N -- the ranks use the shard engine as before.)
        have = torch.cuda.device_count()
        if have < args.gpus and not os.environ.get("MM3D_BENCH_DEVICES"):
            raise SystemExit(f"bench.py: --gpus {args.gpus} without torchrun needs {args.gpus} visible GPUs, this box has {have} "
                             "(launch with torch.distributed.run for one rank per GPU, or lower --gpus)")
        if args.engine != "library":
            raise SystemExit(f"bench.py: --gpus {args.gpus} without torchrun runs the one-process device-list engine; --engine {args.engine} is a one-GPU engine")
        print(f"note: --gpus {args.gpus} without torchrun: using --engine devices (one process over {args.gpus} GPUs)", file=sys.stderr)
        args.engine = "devices"
    elif args.gpus != world and args.engine != "devices":
        if rank == 0:
            print(f"note: --gpus {args.gpus} but WORLD_SIZE {world} (torchrun): one rank per GPU, {world} GPUs", file=sys.stderr)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    mm = ge.load()
    from map_merge_amd import sharding
    dev_list = None
    if args.engine == "devices":
        if world != 1:
            raise SystemExit("--engine devices is ONE process over --gpus N devices: launch it without torchrun")
        dev_list = [int(x) for x in os.environ["MM3D_BENCH_DEVICES"].split(",")] if os.environ.get("MM3D_BENCH_DEVICES") else list(range(max(1, args.gpus)))
        ctx = mm.Context(devices=dev_list)                 # (creates the RCCL communicators: seconds, once, outside the timed region)
    else:
        ctx = mm.Context(local_rank)
    n_gpus = len(dev_list) if dev_list else world
    # BASELINE.json's configuration is FPFH + SAC_IA; the other combinations (PFH is the reference's default
    # descriptor, MATCHING its default method) can be timed with the flags
    desc_type = mm.Descriptor[args.descriptor]
    desc_dim = {"FPFH": 33, "PFH": 125, "SHOT": 1344}[args.descriptor]
    params = mm.MapMergingParams(descriptor_type=desc_type, estimation_method=mm.EstimationMethod[args.method],
                                 refine_transform=1)
    if args.sac_iterations > 0:
        params.max_iterations = args.sac_iterations
    if args.resolution > 0:
        params.resolution = args.resolution

    # ---- synthetic workload, resident in HBM before timing ---------------------------------
    n_maps, n_pts = args.maps, args.points
    host, T_gt, _ = make_workload_gt(n_maps, n_pts, cache=not args.no_cache, scenes=args.scenes, overlap_step=args.overlap_step, window=args.window)
    dev_raw = [torch.from_numpy(h.view(np.uint8).reshape(-1, 16)).to(dev) for h in host]
    torch.cuda.synchronize()
    pairs_idx = [(i, j) for i in range(n_maps - 1) for j in range(i + 1, n_maps)]
    host_pcl = []
    want_pcie = args.full and world == 1 and args.engine == "library" and not args.no_pcie and args.host_input == "none"
    if args.host_input == "pcl32" or want_pcie:           # pcl::PointXYZRGB as it lies in memory: x y z 1 | rgba pad pad pad
        PCL = np.dtype({"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16],
                        "itemsize": 32})
        for h in host:
            a = np.zeros(len(h), dtype=PCL)
            a["x"], a["y"], a["z"], a["w"], a["rgba"] = h["x"], h["y"], h["z"], 1.0, h["rgba"]
            host_pcl.append(a)

    stats = {}
    last = {}                                              # what the latest step returned to its caller (--dump-outputs)

    # Within a rank the maps and pairs are dealt once more over S contexts (one HIP stream, one host
    # thread each): a pair is a chain of dependent launches with a few host round trips, so one
    # stream leaves SIMDs idle that another stream's kernels can use.
    # A stream's host thread does not spin while it waits (stream_wait in csrc/grid.hip polls and naps), but it is not free
    # either: measured 3.2 busy cores for 16 streams on one rank = 0.2 of a core per stream.  The ranks of one node share the
    # container's CPU quota (16 CPUs on the single-GPU boxes), and a group over its quota gets EVERY rank throttled, so a
    # rank's streams are clamped to its share of the quota at that price (8 ranks on 16 CPUs: 10 streams each; up to 4 ranks
    # keep all 16).  A spinning thread (MM3D_WAIT=spin) holds a whole core.  `host_cpu.throttled_ms_per_step` in the line
    # shows whether the clamp was enough.
    S = max(1, args.streams)
    quota = cgroup_cpu_limit()
    cpus = quota if quota is not None else float(os.cpu_count() or 16)
    if os.environ.get("MM3D_WAIT") == "spin":
        S = max(1, min(S, max(2, int(cpus // max(world, 1)) - (1 if world > 1 else 0))))
    else:
        S = max(1, min(S, max(2, int(cpus / (0.2 * max(n_gpus, 1))))))
    library_streams = world > 1 or args.engine in ("library", "shard", "devices")
    # (the library engines deal the work to S streams inside libmm3d: only the Python-threaded one needs contexts of its own)
    ctxs = [ctx] + ([] if library_streams else [mm.Context(local_rank) for _ in range(S - 1)])
    tpool = ThreadPoolExecutor(S) if S > 1 and not library_streams else None

    def run_streams(fn):
        if tpool is None:
            fn(0)
        else:
            list(tpool.map(fn, range(S)))                  # re-raises a worker's exception

    def step_sharded():
        """N > 1 (and `--engine shard` on one GPU): the driver is the library's (mm3d_shard_*): this rank's maps on the
        context's streams, ONE all-gather of the packed feature bundles (RCCL), the pairs whose target this rank
        owns, one all-gather of the pair records (RCCL), the pose graph on every rank."""
        t0 = time.perf_counter()
        ctx.srand(1)                                       # the reference's process starts at glibc seed 1
        views = [(dev_raw[i].data_ptr(), len(host[i])) for i in range(n_maps)]
        sh = ctx.shardBegin(views, params, rank, world)
        t1 = time.perf_counter()
        npts, nkp = sharding.exchange_bundles(sh, world, rank, dist if world > 1 else None, dev if backend == "nccl" else None)
        t2 = time.perf_counter()
        mine, is_mine = sh.pairs()
        t3 = time.perf_counter()
        owners = [sharding.pair_owner(int(r["source_idx"]), int(r["target_idx"]), world) for r in mine]
        mine = sharding.gather_pair_records(mine, owners, world, rank, dist if world > 1 else None, dev if backend == "nccl" else None)
        T = mm.globalTransforms(mine, params.confidence_threshold, n_maps)
        t4 = time.perf_counter()
        sh.end()
        stats.update(dict(n_pairs=len(mine), t_features=t1 - t0, t_exchange=t2 - t1, t_pairs=t3 - t2, t_gather_graph=t4 - t3,
                          pts_filtered=[int(v) for v in npts], keypoints=[int(v) for v in nkp],
                          icp_iters=[int(x) for x in mine["icp_iterations"]], pairs_here=int(is_mine.sum()),
                          n_estimated=int(sum(1 for t in T if np.any(t))),
                          crc=zlib.crc32(np.ascontiguousarray(mine["transform"]).tobytes()) & 0xffffffff))
        last.update(transforms=T, pairs=mine)
        return T

    def step_pipelined():
        """One GPU: no exchange separates the stages, so a pair starts as soon as its two maps exist.  Only
        `--feature-streams` of the streams extract features (maps finish earlier that way), the others -- and
        the feature streams once the maps are handed out -- claim pairs in order and wait for their maps."""
        t0 = time.perf_counter()
        maps, kn = [None] * n_maps, [0] * n_maps
        ready = [threading.Event() for _ in range(n_maps)]
        lock = threading.Lock()
        next_map, next_pair = iter(range(n_maps)), iter(range(len(pairs_idx)))
        recs = np.zeros(len(pairs_idx), dtype=mm.PAIR)
        is_live = np.zeros(len(pairs_idx), dtype=bool)
        t_last_map = [t0]
        F = max(1, min(S, args.feature_streams))

        def live(q):
            i, j = pairs_idx[q]
            for e in (ready[i], ready[j]):
                if not e.wait(timeout=300):
                    raise RuntimeError("a map never became ready")
            return kn[i] > 0 and kn[j] > 0

        def worker(s):
            c = ctxs[s]
            c.srand(1)                                     # the reference's process starts at glibc seed 1
            try:
                while s < F:
                    with lock:
                        i = next(next_map, None)
                    if i is None:
                        break
                    raw = c.cloud_from_ptr(dev_raw[i].data_ptr(), len(host[i]))
                    m = c.mapFeatures(raw, params)
                    raw.free()
                    c.mapPrepare(m, params)
                    maps[i], kn[i] = m, len(m.keypoints)
                    with lock:
                        t_last_map[0] = max(t_last_map[0], time.perf_counter())
                    ready[i].set()
            except BaseException:
                for e in ready:                            # do not leave the other streams waiting
                    e.set()
                raise
            pos = 0
            while True:
                with lock:
                    p = next(next_pair, None)
                if p is None:
                    break
                for q in range(pos, p):                    # replay the draws of the pairs other streams execute
                    if live(q):
                        c.pairEstimate(maps[pairs_idx[q][0]], maps[pairs_idx[q][1]], params, execute=False)
                if live(p):
                    recs[p] = c.pairEstimate(maps[pairs_idx[p][0]], maps[pairs_idx[p][1]], params, execute=True)
                    is_live[p] = True
                pos = p + 1
            c.synchronize()

        run_streams(worker)
        t3 = time.perf_counter()
        recs["source_idx"] = [i for i, _ in pairs_idx]
        recs["target_idx"] = [j for _, j in pairs_idx]
        mine = recs[is_live]
        T = mm.globalTransforms(mine, params.confidence_threshold, n_maps)
        t4 = time.perf_counter()
        stats.update(dict(n_pairs=len(mine), t_features=t_last_map[0] - t0, t_exchange=0.0, t_pairs=t3 - t_last_map[0],
                          t_gather_graph=t4 - t3, pts_filtered=[len(m.points) for m in maps], keypoints=kn,
                          icp_iters=[int(x) for x in mine["icp_iterations"]],
                          n_estimated=int(sum(1 for t in T if np.any(t))),
                          crc=zlib.crc32(np.ascontiguousarray(mine["transform"]).tobytes()) & 0xffffffff))
        for m in maps:
            m.free()
        last.update(transforms=T, pairs=mine)
        return T

    def step_library():
        """One GPU, default: the whole job is ONE call of the reference's own entry point on HBM-resident
        clouds; the library deals the two loops to its streams itself (mm3d_set_streams: C++ threads and
        helper contexts inside libmm3d, the same pipelined scheme as step_pipelined without the Python
        in between)."""
        ctx.srand(1)                                       # the reference's process starts at glibc seed 1
        if args.host_input == "pcl32":
            views = [(host_pcl[i].ctypes.data, len(host[i]), 32, 16) for i in range(n_maps)]
        else:
            views = [(dev_raw[i].data_ptr(), len(host[i])) for i in range(n_maps)]
        T, mine = ctx.estimateMapsTransforms(views, params, return_pairs=True)
        L = mm.lib()
        f_s, tot_s = C.c_double(), C.c_double()
        L.mm3d_last_run_stage_seconds(ctx._h, C.byref(f_s), C.byref(tot_s))
        pts, kps = (C.c_size_t * n_maps)(), (C.c_size_t * n_maps)()
        L.mm3d_last_run_map_sizes.restype = C.c_size_t
        L.mm3d_last_run_map_sizes(ctx._h, pts, kps, C.c_size_t(n_maps))
        t_exchange, t_pairs, t_gather = 0.0, tot_s.value - f_s.value, 0.0
        if dev_list:                                       # per-stage seconds of the slowest device, and the RCCL gather alone
            ex_s, pr_s, g_s = ctx.lastRunDeviceSeconds()
            t_exchange, t_pairs, t_gather = ex_s - f_s.value, pr_s - ex_s, tot_s.value - pr_s
            stats["rccl_gather_us"] = round(1e6 * g_s, 1)
        stats.update(dict(n_pairs=len(mine), t_features=f_s.value, t_exchange=t_exchange, t_pairs=t_pairs,
                          t_gather_graph=t_gather, pts_filtered=list(pts), keypoints=list(kps),
                          icp_iters=[int(x) for x in mine["icp_iterations"]],
                          n_estimated=int(sum(1 for t in T if np.any(t))),
                          crc=zlib.crc32(np.ascontiguousarray(mine["transform"]).tobytes()) & 0xffffffff, records=mine))
        last.update(transforms=T, pairs=mine)
        return T

    if library_streams:
        ctx.setStreams(S)
        step = step_library if (world == 1 and args.engine in ("library", "devices")) else step_sharded
    else:
        step = step_pipelined

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        for c in ctxs:
            c.synchronize()
        torch.cuda.synchronize()

    # HIP events around every kernel of the timed steps feed the per-kernel figures of --full only
    kernel_events = args.full and not args.no_kernel_events
    for _ in range(args.warmup):
        step()
    for c in ctxs:
        c.profile_reset()
        c.profile(kernel_events)
    barrier()
    def host_waits():
        # (host waits for a stream, summed over the library's worker contexts: mm3d_debug_waits)
        import ctypes as C
        tot = [0, 0]
        for c in ctxs:
            w = (C.c_longlong * 2)()
            try:
                mm.lib().mm3d_debug_waits(c._h, w)
            except Exception:
                return None
            tot[0] += w[0]; tot[1] += w[1]
        return tot
    w0 = host_waits()
    cpu0, thr0 = time.process_time(), cgroup_throttle()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    w1 = host_waits()
    host_cpu = {"cores_busy": round((time.process_time() - cpu0) / max(elapsed, 1e-9), 2), "cgroup_cpu_limit": cgroup_cpu_limit(),
                "cgroup_throttled_ms_per_step": round((cgroup_throttle() - thr0) / 1e3 / max(args.steps, 1), 2)}
    if w0 and w1:
        host_cpu["stream_waits_per_step"] = round((w1[0] - w0[0]) / max(args.steps, 1), 1)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last["transforms"], last["pairs"])
    sacia_certified = None
    if os.environ.get("MM3D_SACIA_STATS"):                 # (a study run: the collection costs a wait per batch of pairs)
        st = mm.sacia_stats()
        sacia_certified = {"pairs": st[0], "decided_without_a_chain": st[1], "candidates_left": st[2], "float_chains_run": st[3],
                           "what": "SAC-IA's pick certified from the error sums in double (csrc/registration.hip::k_sacia_select), all steps of this run"}
    for c in ctxs:
        c.profile(False)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    def headline():
        """The contract's fields: the figure, its unit and sense, and the job it was measured on."""
        n_pairs = stats["n_pairs"]
        return {
            "metric": "map-pairs/sec (normals+%s+%s+ICP, end to end incl. per-map features)"
                      % (args.descriptor, "SAC-IA" if args.method == "SAC_IA" else "matching+RANSAC"),
            "value": round(n_pairs * args.steps / elapsed, 4), "unit": "map-pairs/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / max(args.steps, 1), 3), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{n_maps} maps x {n_pts} raw pts, {args.descriptor} + {args.method} + ICP refine, {n_pairs} pairs"
                                   + (f", {args.window:g} m windows" if args.window > 0 else "") + (f", resolution {args.resolution:g}" if args.resolution > 0 else "")
                                   + (f", '{args.scenes}' scenes, windows {args.overlap_step:g} of a side apart" if args.scenes != "independent" or args.overlap_step != 0.5 else "")
                                   + (f", {args.sac_iterations} SAC-IA hypotheses" if args.sac_iterations > 0 else "")
                                   + (" [DIAGNOSTIC: host pcl::PointXYZRGB input, upload inside the step]" if args.host_input != "none" else ""),
                       "parallelism": (f"ONE process, one mm3d_estimate_maps_transforms call on the device list {dev_list} (mm3d_create_devices): maps by owner, "
                                       f"bundles pulled with hipMemcpyPeerAsync, pairs by target owner, {S} streams per device, pair records through "
                                       + ("one in-library ncclAllGather" if ctx.uses_rccl else "host memory (duplicate-device test hook: no RCCL)")
                                       if dev_list else
                                       f"one mm3d_estimate_maps_transforms call, {S} streams inside the library"
                                       if world == 1 and args.engine == "library" else
                                       f"mm3d_shard_*: maps by owner, pairs by target owner over {world} GPU(s) x {S} streams inside the library"
                                       if step is step_sharded else
                                       f"maps and pairs dealt over {S} streams (Python threads)"),
                       "points_after_filter_mean": int(np.mean(stats["pts_filtered"])), "keypoints_mean": int(np.mean(stats["keypoints"]))},
        }

    def step_report():
        """What the timed steps themselves report, at no cost beyond them."""
        return {
            "stage_seconds_last_step": {k: round(stats[k], 4) for k in ("t_features", "t_exchange", "t_pairs", "t_gather_graph")},
            "maps_estimated": stats["n_estimated"],
            "icp_iterations_histogram": {str(k): int(v) for k, v in zip(*np.unique(stats["icp_iters"], return_counts=True))},
            "host_cpu": host_cpu,                           # the box's CPU quota bounds how many host threads can wait at once
            **({"sacia_certified": sacia_certified} if sacia_certified else {}),
            "pair_transforms_crc32": stats["crc"],          # same job, same bits: independent of --gpus / --streams
            **({"rccl_gather_us": stats["rccl_gather_us"]} if "rccl_gather_us" in stats else {}),
        }

    def print_line(out):
        # Every rank empties its C stdio buffer now (RCCL's banner sits there on each of them, and torchrun merges the ranks'
        # stdout into one pipe), and rank 0 prints behind a barrier: the JSON line is the LAST line of the job's output.
        try:
            C.CDLL(None).fflush(None)
            sys.stdout.flush()
        except Exception:
            pass
        if world > 1:
            dist.barrier()
        if rank == 0:
            print(json.dumps(out()), flush=True)

    def close():
        if tpool is not None:
            tpool.shutdown()
        for c in ctxs:
            c.close()
        if world > 1:
            dist.destroy_process_group()

    if not args.full:
        # a plain run: the headline and what the timed steps report; nothing more runs on the GPU
        print_line(lambda: {**headline(), **step_report()})
        close()
        return

    # N = 1: the same step with the clouds handed over the way the reference's callers hold them -- host arrays of
    # pcl::PointXYZRGB (stride 32) in pageable memory, uploaded inside the step.  A secondary figure, never `value`.
    pcie = None
    if want_pcie and rank == 0:
        saved = dict(stats)
        args.host_input = "pcl32"
        step()                                             # (untimed: first touch of the host arrays)
        barrier()
        tp0 = time.perf_counter()
        for _ in range(2):
            step()
        barrier()
        tp = (time.perf_counter() - tp0) / 2
        pcie = {"value": round(saved["n_pairs"] / tp, 4), "unit": "map-pairs/s", "ms_per_step": round(1e3 * tp, 3), "steps": 2,
                "input": "host pcl::PointXYZRGB arrays (stride 32, pageable), %d MB uploaded inside the step" % (sum(len(h) for h in host) * 32 // 1000000),
                "pair_transforms_crc32": stats["crc"]}
        args.host_input = "none"
        stats.clear(); stats.update(saved)
    prof = {}
    for c in ctxs:                                         # per-kernel HIP-event times, summed over the rank's streams
        for k, v in c.profile_entries().items():
            e = prof.setdefault(k, {"ms": 0.0, "launches": 0, "bytes": 0.0})
            for f in ("ms", "launches", "bytes"):
                e[f] += v[f]

    # untimed: the same kernels alone on the GPU (one stream, maps 0 and 1 and their pair).  In the
    # timed region several streams share the CUs, so a kernel's HIP-event duration there includes the
    # time it spent sharing; the isolated figure is what speaks about the kernel itself.
    iso, gpu_sample = {}, None
    normals_alone = None
    # (MM3D_BENCH_NO_ISOLATED=1: a kernel-trace run wants nothing behind the timed steps -- scripts/profile_round.sh)
    if rank == 0 and not os.environ.get("MM3D_BENCH_NO_ISOLATED"):
        ctx.profile_reset()
        ctx.profile(True)
        ctx.srand(1)
        two = []
        sift_fused_ms_map0 = None
        for i in (0, 1):
            raw = ctx.cloud_from_ptr(dev_raw[i].data_ptr(), len(host[i]))
            two.append(ctx.mapFeatures(raw, params))
            raw.free()
            if i == 0:
                ctx.synchronize()
                sift_fused_ms_map0 = ctx.profile_entries().get("sift_dog", {}).get("ms")
        rec01 = ctx.pairEstimate(two[0], two[1], params)
        ctx.synchronize()
        ctx.profile(False)
        iso = ctx.profile_entries()
        # computeSurfaceNormals as a launch of its own (in the whole-map path with SIFT keypoints the normals ride on the first
        # octave's sorted lists and have no launch to time): map 0's filtered points through the stand-alone entry point, and
        # detectKeypoints stand-alone (no fused normals) to price what the fusion adds to the first octave
        try:
            ctx.profile_reset(); ctx.profile(True)
            nrm0 = ctx.computeSurfaceNormals(two[0].points, params.normal_radius)
            ctx.synchronize(); ctx.profile(False)
            e_n = ctx.profile_entries()
            ctx.profile_reset(); ctx.profile(True)
            kp0 = ctx.detectKeypoints(two[0].points, nrm0, int(params.keypoint_type), params.keypoint_threshold, params.normal_radius, params.resolution)
            ctx.synchronize(); ctx.profile(False)
            e_k = ctx.profile_entries()
            n0 = len(two[0].points)
            t_n = sum(v["ms"] for k, v in e_n.items() if k.startswith("normals")) / 1e3
            normals_alone = {"mpoints_per_s": round(n0 / 1e6 / max(t_n, 1e-9), 2), "points": n0, "kernel_ms": round(1e3 * t_n, 3),
                             "hbm_frac": round(n0 * 28.0 / max(t_n, 1e-9) / (HBM_PEAK_GBS * 1e9), 5),
                             "what": "mm3d_compute_normals on map 0's filtered points, alone on the GPU (the launch the fused path no longer has)"}
            if "sift_dog" in e_k and sift_fused_ms_map0:
                normals_alone["sift_dog_unfused_ms_map0"] = round(e_k["sift_dog"]["ms"], 3)
                normals_alone["sift_dog_fused_ms_map0"] = round(sift_fused_ms_map0, 3)
                normals_alone["fused_marginal_ms_map0"] = round(sift_fused_ms_map0 - e_k["sift_dog"]["ms"], 3)
            del nrm0, kp0
        except Exception as exc:                            # (a diagnostic: never fails the bench line)
            normals_alone = {"error": str(exc)[:200]}
        # what the device computed for maps 0 and 1 and pair (0, 1): bench's parity_check holds it against the oracle
        gpu_sample = {"maps": [dict(points=m.points.numpy(), keypoints=m.keypoints.numpy(), descriptors=m.descriptors.numpy())
                               for m in two], "pair": rec01}
        for m in two:
            m.free()
    # map-pairs/sec = surviving pairs / wall time of the PER-PAIR stage (R/src/map_merging.cpp:256-269) -- the pair
    # loop alone, on maps whose features and search structures already exist.  Untimed extra after the step loop: every map
    # prepared once (mm3d_shard_begin as the only rank), then the whole pair loop (mm3d_shard_pairs: all pairs, same-target
    # batches on the context's streams) three times.  The pipelined step overlaps this stage with the features, so
    # "step time minus the time the last map was ready" says nothing about it.
    pair_stage = None
    if rank == 0 and world == 1 and args.engine in ("library", "devices") and not dev_list and not args.no_pair_stage:
        try:
            views = [(dev_raw[i].data_ptr(), len(host[i])) for i in range(n_maps)]
            ctx.srand(1)
            sh = ctx.shardBegin(views, params, 0, 1)
            ctx.srand(1)
            sh.pairs()                                     # (untimed: first touch)
            reps = 3
            tq0 = time.perf_counter()
            for _ in range(reps):
                ctx.srand(1)
                recs_ps, _ = sh.pairs()
            tq = (time.perf_counter() - tq0) / reps
            sh.end()
            pair_stage = {"pairs_per_s": round(len(recs_ps) / max(tq, 1e-9), 2), "ms_per_pair_loop": round(1e3 * tq, 3), "pairs": int(len(recs_ps)), "repeats": reps,
                          "pair_transforms_crc32": zlib.crc32(np.ascontiguousarray(recs_ps["transform"]).tobytes()) & 0xffffffff,
                          "what": "the pair loop alone (estimateTransform + transformScore of every live pair, map_merging.cpp:256-269) on prepared maps, "
                                  "%d streams, features excluded" % S}
        except Exception as exc:                            # (a secondary figure: never fails the bench line)
            pair_stage = {"error": str(exc)[:200]}
    # HBM-side traffic per launch from the most recent committed PMC passes (scripts/profile_round.sh)
    pmc_traffic, pmc_source, pmc_hashes = {}, None, {}
    try:
        latest = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))[-1]
        with open(latest) as f:
            doc = json.load(f)
        pmc_traffic, pmc_hashes = doc["bytes_per_launch"], doc.get("source_sha256", {})
        pmc_source = "profiles/" + os.path.basename(latest).replace("traffic.json", "pmc_hbm_traffic.csv")
        counters_workload = doc.get("workload", COUNTERS_WORKLOAD_DEFAULT)
    except Exception:
        counters_workload = None
    # per-launch counters only speak about the workload they were counted on
    counters_apply = counters_workload is not None and counters_workload == workload_signature(args)
    if not counters_apply:
        pmc_traffic = {}

    def stale(kernel):
        """True when the kernel's sources are not the ones the committed counters were collected on (or that is unknown)."""
        now = kernel_source_hash(kernel)
        return not (now and pmc_hashes.get(kernel) == now)

    # VALU instructions per launch from the most recent committed SQ-counter pass (same maps 0 and 1, one stream)
    valu_insts, valu_source, sq_ratios = {}, None, {}
    try:
        latest = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_sq_counters.csv")))[-1]
        import csv
        with open(latest) as f:
            for row in csv.DictReader(f):
                d = float(row.get("dispatches") or 0)
                if d > 0 and row.get("SQ_INSTS_VALU") not in (None, "", "nan"):
                    name = KERNEL_OF_SYMBOL.get(row["kernel"], row["kernel"])
                    valu_insts[name] = float(row["SQ_INSTS_VALU"]) / d

                    def ratio(a, b):
                        try:
                            return round(float(row[a]) / float(row[b]), 4) if float(row[b]) > 0 else None
                        except (KeyError, ValueError, TypeError):
                            return None
                    # share of the wave cycles spent waiting, share of the LDS cycles lost to bank conflicts, VALU busy share
                    # (SQ_ACTIVE_INST_VALU and SQ_WAVE_CYCLES both count quad-cycles; divided by the waves per SIMD it is the SIMD's)
                    sq_ratios[name] = {"stall": ratio("SQ_WAIT_ANY", "SQ_WAVE_CYCLES"), "lds_conflict": ratio("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"),
                                       "valu_active_per_wave_cycle": ratio("SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES")}
        valu_source = "profiles/" + os.path.basename(latest)
    except Exception:
        pass
    if not counters_apply:
        valu_insts, sq_ratios = {}, {}
        # another workload than the headline: its own SQ counters, if a pass was made for it (scripts/profile_counters.sh +
        # assemble_counters.py write one profiles/r*_counters_<name>.json per workload, with the kernels' machine-code hashes)
        try:
            for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_counters_*.json")), reverse=True):
                with open(path) as f:
                    doc = json.load(f)
                if doc.get("workload") != workload_signature(args):
                    continue
                pmc_hashes = doc.get("source_sha256", {})
                for name, v in doc.get("kernels", {}).items():
                    valu_insts[name] = v["valu_wave_instructions_per_dispatch"]
                    sq_ratios[name] = {"stall": v.get("stall"), "lds_conflict": v.get("lds_conflict"),
                                       "valu_active_per_wave_cycle": v.get("valu_active_per_wave_cycle")}
                valu_source = doc.get("source")
                counters_workload = doc["workload"]
                counters_apply = True
                break
        except Exception:
            pass

    def bound_of(name, launch_ms, work):
        """Which ceiling the kernel is nearest to, from what can be known here: algorithmic bytes (or flops) per launch
        against HBM (or MFMA) peak, and -- where the committed SQ counters cover the kernel -- VALU wave-instructions per
        launch against the measured issue peak (VALU_PEAK_WINSTR_S above)."""
        out = {}
        if launch_ms <= 0:
            return out
        if name in MFMA_KERNELS:
            out["mfma_frac"] = round(work / (launch_ms * 1e-3) / (MFMA_KERNELS[name] * 1e12), 5)
        else:
            out["hbm_frac"] = round(work / (launch_ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 5)
        if name in valu_insts and not stale(name):
            vf = valu_insts[name] / (launch_ms * 1e-3) / VALU_PEAK_WINSTR_S
            if vf <= 1.0:                                  # (above 1: the counted launch was not this launch's work -- not evidence)
                out["valu_frac"] = round(vf, 4)
        out["nearest"] = max(((v, k[:-5]) for k, v in out.items()), default=(0, None))[1]
        return out

    # Every rank empties its C stdio buffer now (RCCL's banner sits there on each of them, and torchrun merges the ranks'
    # stdout into one pipe), and rank 0 prints behind a barrier: the JSON line is the LAST line of the job's output.
    try:
        C.CDLL(None).fflush(None)
        sys.stdout.flush()
    except Exception:
        pass
    if world > 1:
        dist.barrier()
    if rank == 0:
        n_pairs = stats["n_pairs"]
        # dominant kernel of this rank, by device time
        dom = max(prof.items(), key=lambda kv: kv[1]["ms"]) if prof else (None, None)
        roofline = None
        if dom[0]:
            k = dom[1]
            avg_ms = k["ms"] / max(k["launches"], 1)
            work_per_launch = k["bytes"] / max(k["launches"], 1)   # bytes, or FLOPs for the MFMA kernel
            rate = work_per_launch / (avg_ms * 1e-3) if avg_ms > 0 else 0.0
            if dom[0] in MFMA_KERNELS:
                roofline = {"kernel": dom[0], "bound": "mfma", "achieved": round(rate / 1e12, 4), "peak": MFMA_KERNELS[dom[0]],
                            "unit": "TFLOP/s", "frac": round(rate / 1e12 / MFMA_KERNELS[dom[0]], 6), "traffic": None,
                            "mfma_dtype": "bf16 (split: three products per f32 product)" if dom[0].endswith("_bf16") else "f32",
                            "avg_launch_us": round(avg_ms * 1e3, 3), "launches_per_step": k["launches"] / max(args.steps, 1),
                            "algorithmic_flops_per_launch": round(work_per_launch, 1)}
            else:
                roofline = {"kernel": dom[0], "bound": "hbm", "achieved": round(rate / 1e9, 3), "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": round(rate / 1e9 / HBM_PEAK_GBS, 6), "traffic": None,
                            "avg_launch_us": round(avg_ms * 1e3, 3), "launches_per_step": k["launches"] / max(args.steps, 1),
                            "algorithmic_bytes_per_launch": round(work_per_launch, 1)}
            # HBM-side bytes per launch from the rocprofv3 PMC passes committed under profiles/ (FETCH_SIZE x2 per
            # the gfx950 note + WRITE_SIZE); null when that kernel was not in the counted run
            roofline["counters_workload"] = counters_workload
            roofline["counters_apply_to_this_workload"] = bool(counters_apply)
            roofline["traffic"] = pmc_traffic.get(dom[0])
            roofline["traffic_source"] = pmc_source if dom[0] in pmc_traffic else None
            # the counters under profiles/ were collected on some commit: "stale" says whether the kernel's sources have
            # changed since (hashes in the traffic file against the files of this tree)
            roofline["traffic_stale"] = stale(dom[0]) if dom[0] in pmc_traffic else None
            if dom[0] in iso and iso[dom[0]]["launches"]:
                iso_ms = iso[dom[0]]["ms"] / iso[dom[0]]["launches"]
                iso_work = iso[dom[0]]["bytes"] / iso[dom[0]]["launches"]
                peak = MFMA_KERNELS[dom[0]] * 1e12 if dom[0] in MFMA_KERNELS else HBM_PEAK_GBS * 1e9
                roofline["isolated_avg_launch_us"] = round(iso_ms * 1e3, 3)
                roofline["isolated_frac"] = round(iso_work / (iso_ms * 1e-3) / peak, 6) if iso_ms > 0 else None
            iso_us = roofline.get("isolated_avg_launch_us")
            if roofline["traffic"] and iso_us and not roofline["traffic_stale"]:
                # what the memory side actually moved per launch (PMC) against the same peak: far above the algorithmic
                # bytes where a kernel keeps scratch lists in global memory (sift_dog, normals_radius)
                roofline["traffic_gbs"] = round(roofline["traffic"] / (iso_us * 1e-6) / 1e9, 1)
                roofline["traffic_frac"] = round(roofline["traffic"] / (iso_us * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
            if dom[0] in valu_insts and iso_us and valu_insts[dom[0]] / (iso_us * 1e-6) <= VALU_PEAK_NOMINAL_WINSTR_S:
                v = valu_insts[dom[0]] / (iso_us * 1e-6)
                roofline["valu"] = {"wave_instructions_per_launch": round(valu_insts[dom[0]]), "achieved": round(v / 1e9, 2),
                                    "peak": round(VALU_PEAK_WINSTR_S / 1e9, 1), "peak_source": "measured: scripts/micro/valu_rate.hip, profiles/r04_valu_rate.txt",
                                    "peak_nominal": round(VALU_PEAK_NOMINAL_WINSTR_S / 1e9, 1), "unit": "G wave-instr/s",
                                    "frac": round(v / VALU_PEAK_WINSTR_S, 4), "frac_of_nominal": round(v / VALU_PEAK_NOMINAL_WINSTR_S, 4),
                                    "source": valu_source, "timed": "isolated_avg_launch_us", "stale": stale(dom[0])}
            if dom[0] in sq_ratios:
                # from the same committed SQ-counter CSV (one stream): SQ_WAIT_ANY / SQ_WAVE_CYCLES and SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE
                roofline["stall"] = sq_ratios[dom[0]]["stall"]
                roofline["lds_conflict"] = sq_ratios[dom[0]]["lds_conflict"]
                roofline["valu_active_per_wave_cycle"] = sq_ratios[dom[0]]["valu_active_per_wave_cycle"]
                roofline["sq_counters_source"] = valu_source
                roofline["sq_counters_stale"] = stale(dom[0])
            # `bound`: the ceiling the kernel is nearest to alone on the GPU -- "hbm" by algorithmic or by measured memory-side
            # bytes, "valu" by issued wave-instructions, "mfma" by flops -- the fractions beside it say how near
            cand = {"hbm": max(roofline.get("isolated_frac") or 0.0, roofline.get("traffic_frac") or 0.0) if dom[0] not in MFMA_KERNELS else 0.0,
                    "mfma": (roofline.get("isolated_frac") or 0.0) if dom[0] in MFMA_KERNELS else 0.0,
                    "valu": (roofline.get("valu") or {}).get("frac", 0.0) if not (roofline.get("valu") or {}).get("stale") else 0.0}
            roofline["bound"] = max(cand.items(), key=lambda kv: kv[1])[0] if any(cand.values()) else roofline["bound"]
            roofline["bound_fractions"] = {k: round(v, 5) for k, v in cand.items()}
            if roofline["bound"] == "valu":
                # The kernel is nearest to the VALU issue ceiling: achieved / peak / unit / frac at the top level speak about THAT
                # ceiling -- against the guide's NOMINAL peak (MI355X_MICROARCH.md: 2 cycles per wave64 v_fma_f32 -> 1.23e12 /s),
                # with the measured peak beside it -- and the HBM figures (the contract's default reading) move to "hbm".
                # Both VALU figures use the kernel's launch time alone on the GPU (the counters were collected that way);
                # frac_in_step divides the same instructions by the launch's duration inside the timed 16-stream region.
                v = roofline["valu"]
                hbm = {k: roofline.get(k) for k in ("achieved", "peak", "unit", "frac", "isolated_frac", "traffic_gbs", "traffic_frac")}
                roofline["hbm"] = hbm
                roofline["achieved"], roofline["peak"], roofline["unit"] = v["achieved"], v["peak_nominal"], v["unit"]
                roofline["frac"] = v["frac_of_nominal"]
                roofline["frac_of_measured_peak"] = v["frac"]
                roofline["frac_in_step"] = round(v["wave_instructions_per_launch"] / (avg_ms * 1e-3) / VALU_PEAK_NOMINAL_WINSTR_S, 4) if avg_ms > 0 else None
                roofline["frac_timed_on"] = "isolated_avg_launch_us (the kernel alone on the GPU, as the SQ counters were collected)"
            roofline["note"] = ("timed region runs %d streams per GPU, so avg_launch_us includes time shared with other kernels; "
                                "neighbourhood kernels (sift_dog, spfh, sacia_err, *_nn_reduce) are bound by VALU instruction issue on "
                                "in-radius pair work, not by HBM: see DESIGN.md sections 5 and 6" % S)
        ranked = sorted(prof.items(), key=lambda kv: -kv[1]["ms"])
        top = ranked[:8]
        if args.kernel_table:
            with open(args.kernel_table, "w") as f:
                f.write("kernel,launches_per_step,ms_per_step,avg_launch_us,algorithmic_bytes_or_flops_per_launch\n")
                for k, v in ranked:
                    f.write("%s,%.1f,%.3f,%.2f,%.0f\n" % (k, v["launches"] / max(args.steps, 1), v["ms"] / max(args.steps, 1),
                                                         1e3 * v["ms"] / max(v["launches"], 1), v["bytes"] / max(v["launches"], 1)))
                f.write("TOTAL,%.1f,%.3f,,\n" % (sum(v["launches"] for _, v in ranked) / max(args.steps, 1),
                                                 sum(v["ms"] for _, v in ranked) / max(args.steps, 1)))
        npts_f = stats["pts_filtered"]
        icp_pts = sum(npts_f[i] * it for (i, j), it in zip([(i, j) for (i, j) in pairs_idx], stats["icp_iters"]))
        out = {
            **headline(),
            # pairs / wall time of the per-pair stage alone, on prepared maps (measured after the step loop; null when
            # that pass did not run).  NOT n_pairs / (step - features): in the pipelined step most pairs run beside the features.
            "pair_stage_pairs_per_s": (pair_stage or {}).get("pairs_per_s"),
            "pair_stage": pair_stage,
            "pair_tail_after_last_map_ms": round(1e3 * stats["t_pairs"], 3),
            "mpoints_per_s": {
                # (FPFH + SIFT: the normals come out of the first octave's scale-space launch, sift.hip k_sift_dog_lds<., true>; there is
                # no launch of their own to time, see "normals_fused" below)
                "normals": round(sum(npts_f) / 1e6 / max(prof.get("normals_radius", {}).get("ms", 0) / 1e3 / max(args.steps, 1), 1e-9), 2)
                if "normals_radius" in prof else ((normals_alone or {}).get("mpoints_per_s")),
                "normals_alone": normals_alone,
                "normals_fused": "computeSurfaceNormals rides on detectKeypoints' first octave (same sorted neighbour lists, same bits)"
                if "normals_radius" not in prof and "sift_dog" in prof else None,
                # FPFH: support points per second of the SPFH kernel (|S| = its algorithmic bytes / 156 B) and
                # keypoints per second of the weighting kernel
                "fpfh_spfh": round(prof["spfh"]["bytes"] / 156.0 / 1e6 / max(prof["spfh"]["ms"] / 1e3, 1e-9), 2) if "spfh" in prof else None,
                "fpfh_weight": round(sum(stats["keypoints"]) / 1e6 / max(prof["fpfh_weight"]["ms"] / 1e3 / max(args.steps, 1), 1e-9), 3)
                if "fpfh_weight" in prof else None,
                "icp": round(icp_pts / 1e6 / max(prof.get("icp_corr_reduce", {}).get("ms", 0) / 1e3 / max(args.steps, 1), 1e-9), 2)
                if "icp_corr_reduce" in prof else None,
            },
            # per kernel, alone on the GPU (the untimed one-stream pass): launch time and the ceiling it is nearest to
            "kernel_bounds_isolated": {k: dict(avg_launch_us=round(1e3 * v["ms"] / max(v["launches"], 1), 1),
                                               **bound_of(k, v["ms"] / max(v["launches"], 1), v["bytes"] / max(v["launches"], 1)))
                                       for k, v in [kv for n_, kv in enumerate(sorted(iso.items(), key=lambda kv: -kv[1]["ms"]))
                                                    if n_ < 10 or kv[0] in ("desc_knn_mfma", "normals_radius", "icp_corr_reduce", "score_nn_reduce")]},
            "top_kernels_ms_per_step": {k: round(v["ms"] / max(args.steps, 1), 3) for k, v in top},
            **step_report(),
            "roofline": roofline,
        }
        # ground truth: the generator knows every map's pose.  Error of the estimated pair transforms (source -> target)
        # against it, over the pairs whose windows overlap by at least 30 %
        from map_merge_amd import synth
        errs = []
        for rec in stats.get("records", []):
            i, j = int(rec["source_idx"]), int(rec["target_idx"])
            if synth.window_overlap(n_maps, n_pts, i, j, overlap_step=args.overlap_step, window=args.window or None) >= 0.3:
                errs.append(float(np.linalg.norm(np.asarray(rec["transform"], dtype=np.float64).reshape(4, 4).T - synth.relative_gt(T_gt[i], T_gt[j]))))
        out["gt_error"] = {"pairs_with_overlap_ge_0.3": len(errs),
                           "median_frobenius": round(float(np.median(errs)), 4) if errs else None,
                           "max_frobenius": round(float(np.max(errs)), 4) if errs else None,
                           "recovered_within_0.5": int(sum(e <= 0.5 for e in errs)),
                           "scenes": args.scenes, "overlap_step": args.overlap_step,
                           "note": "||T_pair - T_gt||_F; the reference's FPFH + SAC-IA (500 hypotheses) does not find the basin on the "
                                   "'independent' scenes, on the device or on the CPU path alike (DESIGN.md section 6)"}
        # GPU seconds per step at registration_visualisation's stage boundaries: kernel time summed over the streams
        gpu_stage = {}
        for k, v in prof.items():
            gpu_stage[stage_of(k)] = gpu_stage.get(stage_of(k), 0.0) + v["ms"] / 1e3 / max(args.steps, 1)
        out["stage_seconds"] = {"gpu_kernel_time_per_step": {k: round(v, 4) for k, v in sorted(gpu_stage.items(), key=lambda kv: -kv[1])}}
        if pcie is not None:
            out["pcie_inclusive"] = pcie
        if world == 1 and not args.no_cpu_baseline:
            b1, b2, parity, cpu_stages = cpu_baseline(host, n_maps, n_pairs, gpu_sample, True, args.descriptor, args.method, params)
            out["cpu_baseline"] = b1
            out["cpu_baseline_all_cores"] = b2
            out["parity_check"] = parity
            out["stage_seconds"].update(cpu_stages)
        # RCCL writes its version banner through C stdio when a communicator is made, and a redirected stdout only flushes
        # that buffer at exit -- after our line.  The contract is ONE JSON line, last: empty C's buffer first.
        try:
            C.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    close()


def dump_outputs(path, transforms, pairs):
    """What the last timed step handed its caller, as <path>/<name>.npy (float32 as computed, integer fields as float64):
    the global transform of every map and every field of the pair records, in the order the step returned them."""
    os.makedirs(path, exist_ok=True)
    arrays = {"global_transforms": np.asarray(np.stack(transforms) if len(transforms) else np.zeros((0, 4, 4)), dtype=np.float32),
              "pair_transform": np.asarray(pairs["transform"], dtype=np.float32),
              "pair_confidence": np.asarray(pairs["confidence"], dtype=np.float64)}
    for f in ("source_idx", "target_idx", "icp_iterations", "n_correspondences", "n_inliers", "icp_correspondences"):
        arrays["pair_" + f] = np.asarray(pairs[f], dtype=np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def cpu_baseline(host, n_maps, n_pairs, gpu_sample, check, descriptor="FPFH", method="SAC_IA", params=None):
    """The CPU oracle (kind "port": our restatement of the reference's PCL path) on a bounded sample of the
    workload, extrapolated to the whole job as n_maps * t_map + n_pairs * t_pair (means over the sample):
      B2 `cpu_baseline_all_cores`: the features of maps 0, 1, 2 and the pairs (0,1), (0,2), (1,2) with the oracle's
          loops over points on every host core (OpenMP; results identical, tests/test_oracle_cpu.py).
      B1 `cpu_baseline`: one thread, like the reference's hot path: the features of maps 0 and 1 and the same three
          pairs (map 2's features are B2's: the same bits).
    Both report the seconds per stage at registration_visualisation's boundaries.  The oracle's results for maps 0, 1
    and pair (0, 1) are then held against what the device computed for them in this very run (`parity_check`)."""
    po = ge.load_oracle()
    p = params if params is not None else po.params_default()   # the same parameter values the device ran with
    describe = {"FPFH": po.descriptors_fpfh, "PFH": po.descriptors_pfh, "SHOT": po.descriptors_shot}[descriptor]
    # B2's threads: the physical cores (SMT siblings do not help these loops), at most 64 -- and not more than the
    # container's CPU quota lets run at once (the GPU boxes show 256 CPUs and grant 16: threads beyond the quota
    # only get the whole group throttled)
    cores = max(1, min(64, (os.cpu_count() or 2) // 2))
    quota = cgroup_cpu_limit()
    if quota is not None:
        cores = max(1, min(cores, int(quota)))
    try:
        with open("/proc/cpuinfo") as f:
            model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "?")
    except Exception:
        model = "?"

    def timed(acc, key, fn, *a):
        t0 = time.perf_counter()
        r = fn(*a)
        acc[key] = acc.get(key, 0.0) + time.perf_counter() - t0
        return r

    def features(cloud, acc):
        d = timed(acc, "downSample", po.downsample, cloud, p.resolution)
        f = timed(acc, "removeOutliers", po.remove_outliers, d, p.descriptor_radius, p.outliers_min_neighbours)
        n = timed(acc, "computeSurfaceNormals", po.normals, f, p.normal_radius)
        kp, _ = timed(acc, "detectKeypoints", po.keypoints_sift, f, p.resolution, 3, 3, p.keypoint_threshold)
        kp, desc = timed(acc, "computeLocalDescriptors", describe, f, n, kp, p.descriptor_radius)
        return f, kp, desc

    def pair(A, B, acc):
        (f0, k0, d0), (f1, k1, d1) = A, B
        po.srand(1)
        if method == "SAC_IA":
            T, _, _ = timed(acc, "estimateTransform: initial (k-NN + SAC-IA | RANSAC)", po.sac_ia, k0, d0, k1, d1, p.inlier_threshold,
                            p.max_correspondence_distance, p.max_iterations)
        else:
            def initial():
                corr = po.find_correspondences(d0, d1, int(p.matching_k))
                return po.ransac(k0, k1, corr, p.inlier_threshold)[0]
            T = timed(acc, "estimateTransform: initial (k-NN + SAC-IA | RANSAC)", initial)
        T_init = T
        T, it = timed(acc, "estimateTransform: ICP", po.icp, f0, f1, T, p.max_correspondence_distance, p.inlier_threshold, p.max_iterations,
                      p.transform_epsilon)
        score = timed(acc, "transformScore", po.transform_score, f0, f1, T, p.max_correspondence_distance)
        pair.last_init = T_init
        return T, it, score

    # (many SAC-IA hypotheses, the 'lattice' rows' 20 000: a pair costs 40 x the default's, so the sample is two maps and
    # ONE pair, and B1 extracts the features of one map only -- still the same code on the same workload, still bounded)
    heavy_pairs = method == "SAC_IA" and int(p.max_iterations) > 2000
    n_sample = min(2 if heavy_pairs else 3, len(host))
    sample_pairs = [(i, j) for i in range(n_sample - 1) for j in range(i + 1, n_sample)]
    # B2 (fast): all cores; it also provides map 2's features for B1's pairs
    po.set_threads(cores)
    st2 = {}
    t0 = time.perf_counter()
    F2 = [features(host[i], st2) for i in range(n_sample)]
    t_maps2 = time.perf_counter() - t0
    t0 = time.perf_counter()
    R2 = [pair(F2[i], F2[j], st2) for i, j in sample_pairs]
    t_pairs2 = time.perf_counter() - t0
    # yardstick for the check below (untimed): pair (0, 1)'s ICP once more from the same initial estimate with its sums in
    # double over the original points -- what exact arithmetic gives, not the reference's float sums (oracle/o_matching.c)
    pair(F2[0], F2[1], {})
    corr_oracle = int(po.last_pair_trace()["icp_correspondences"])
    T_dbl, it_dbl = po.icp_double_sums(F2[0][0], F2[1][0], pair.last_init, p.max_correspondence_distance, p.max_iterations, p.transform_epsilon)
    corr_dbl = int(po.lib().mo_last_double_sums_correspondences())
    t_map2, t_pair2 = t_maps2 / n_sample, t_pairs2 / max(len(sample_pairs), 1)
    job2 = n_maps * t_map2 + n_pairs * t_pair2
    b2 = {"value": round(n_pairs / job2, 6), "unit": "map-pairs/s", "cores": cores, "kind": "port", "cpu": model,
          "sample": f"{n_sample} of {n_maps} maps' features ({t_map2:.2f} s each) + {len(sample_pairs)} of {n_pairs} pairs ({t_pair2:.2f} s each) on "
                    f"{cores} OpenMP threads, extrapolated to the job as {n_maps}*t_map + {n_pairs}*t_pair = {job2:.0f} s"}
    # B1: one thread; maps 0 and 1 (map 2's features are B2's, the same bits), the same pairs
    po.set_threads(1)
    st1 = {}
    n_b1 = min(1 if heavy_pairs else 2, n_sample)
    t0 = time.perf_counter()
    F1 = [features(host[i], st1) for i in range(n_b1)] + F2[n_b1:]
    t_map = (time.perf_counter() - t0) / n_b1
    t0 = time.perf_counter()
    R1 = [pair(F1[i], F1[j], st1) for i, j in sample_pairs]
    t_pair = (time.perf_counter() - t0) / max(len(sample_pairs), 1)
    job = n_maps * t_map + n_pairs * t_pair
    b1 = {"value": round(n_pairs / job, 6), "unit": "map-pairs/s", "cores": 1, "kind": "port", "cpu": model,
          "sample": f"{n_b1} of {n_maps} maps' features ({t_map:.1f} s each) + {len(sample_pairs)} of {n_pairs} pairs ({t_pair:.1f} s each), "
                    f"extrapolated to the job as {n_maps}*t_map + {n_pairs}*t_pair = {job:.0f} s"}
    # seconds per map (feature stages) / per pair (pair stages), means over the sample
    feat_keys = ("downSample", "removeOutliers", "computeSurfaceNormals", "detectKeypoints", "computeLocalDescriptors")
    per_unit = lambda st, nm: {k: round(v / (nm if k in feat_keys else max(len(sample_pairs), 1)), 4) for k, v in st.items()}   # noqa: E731
    cpu_stages = {"cpu_1_thread_per_map_or_pair": per_unit(st1, n_b1), "cpu_all_cores_per_map_or_pair": per_unit(st2, n_sample)}
    (f0, k0, d0), (f1, k1, d1) = F2[0], F2[1]
    (g0, h0, e0) = F1[0]
    T, it, score = R2[0]
    T1, it1, score1 = R1[0]
    threads_agree = (g0.tobytes() == f0.tobytes() and h0.tobytes() == k0.tobytes() and e0.tobytes() == d0.tobytes()
                     and T1.tobytes() == T.tobytes() and it1 == it and score1 == score)
    parity = None
    if check and gpu_sample is not None:
        def same(a, b):
            return a.shape == b.shape and a.tobytes() == b.tobytes()
        xyz = lambda a: np.stack([a["x"], a["y"], a["z"]], axis=1)           # noqa: E731
        g = gpu_sample["maps"]
        rec = gpu_sample["pair"]
        T_dev = np.asarray(rec["transform"], dtype=np.float32).reshape(4, 4).T
        fro = float(np.linalg.norm(T_dev - T))
        fro_dbl = float(np.linalg.norm(T_dev - T_dbl))
        cpu_noise = float(np.linalg.norm(T - T_dbl))
        conf_rel = abs(float(rec["confidence"]) * score - 1.0)
        # The confidence is 1 / transformScore(T): against the oracle's own value it inherits the CPU path's noise in T (at 1.6 M
        # points T_oracle is 2e-3 from exact arithmetic and the score moves with it), which says nothing about the score kernel.
        # The kernel is held to the CPU path's transformScore evaluated AT THE DEVICE'S TRANSFORM (1e-4 relative, measured ~1e-6);
        # the raw difference is reported and bounded like the all-pairs test bounds it (1e-3).
        score_at_dev_T = po.transform_score(f0, f1, T_dev, p.max_correspondence_distance)
        conf_rel_same_T = abs(float(rec["confidence"]) * score_at_dev_T - 1.0)
        # THE stated pair-transform tolerance (oracle/pyoracle.py, BASELINE.md "Reported metrics"): BOTH
        # clauses must hold.  exact: within TOL_T_EXACT of the same ICP with its sums in double, equal iteration counts;
        # oracle: within transform_tolerance(n_src) of the CPU path, whose sequential float sums carry their own summation
        # noise (reported as cpu_path_own_noise_vs_double_sums), equal iteration counts.
        t_tol = po.transform_tolerance(len(f0), cpu_noise)        # min(per-point slope, this pair's own CPU noise + TOL_T_EXACT)
        it_dev = int(rec["icp_iterations"])
        exact_ok = fro_dbl <= po.TOL_T_EXACT and it_dev == int(it_dbl)
        oracle_ok = fro <= t_tol and cpu_noise <= po.transform_tolerance(len(f0)) and it_dev == int(it)
        parity = {
            "sample": "maps 0 and 1 and pair (0, 1) of the timed workload: device (this run) vs CPU oracle",
            "filtered_points_bit_equal": bool(same(g[0]["points"], f0) and same(g[1]["points"], f1)),
            "keypoints_bit_equal": bool(same(xyz(g[0]["keypoints"]), xyz(k0)) and same(xyz(g[1]["keypoints"]), xyz(k1))),
            "descriptors_bit_equal": bool(same(g[0]["descriptors"], d0) and same(g[1]["descriptors"], d1)),
            "n_points": [int(len(f0)), int(len(f1))], "n_keypoints": [int(len(k0)), int(len(k1))],
            "pair_transform_frobenius": round(fro, 9), "pair_transform_tolerance": t_tol,
            "pair_transform_frobenius_vs_double_sums": round(fro_dbl, 9), "pair_transform_tolerance_vs_double_sums": po.TOL_T_EXACT,
            "cpu_path_own_noise_vs_double_sums": round(cpu_noise, 9),
            "clause_oracle_ok": bool(oracle_ok), "clause_exact_ok": bool(exact_ok),
            "confidence_rel_err_at_the_device_transform": round(conf_rel_same_T, 9), "confidence_tolerance_at_the_device_transform": 1e-4,
            "confidence_rel_err": round(conf_rel, 9), "confidence_tolerance": 1e-3,
            "icp_iterations": {"device": it_dev, "oracle": int(it), "double_sums": int(it_dbl)},
            "icp_last_iteration_correspondences": {"device": int(rec["icp_correspondences"]), "oracle": int(corr_oracle),
                                                   "double_sums": int(corr_dbl)},
            "all_pairs": "tests/test_gpu_baseline_configs.py::test_16x500k_all_120_pairs_within_the_stated_tolerance holds every pair of the "
                         "headline job to the same two clauses (profiles/r05_all_pairs_tolerance.txt)",
            "oracle_threads_agree": bool(threads_agree),
        }
        parity["ok"] = bool(parity["filtered_points_bit_equal"] and parity["keypoints_bit_equal"] and parity["descriptors_bit_equal"]
                            and oracle_ok and exact_ok and conf_rel_same_T <= 1e-4 and conf_rel <= 1e-3 and threads_agree)
    return b1, b2, parity, cpu_stages


if __name__ == "__main__":
    main()
