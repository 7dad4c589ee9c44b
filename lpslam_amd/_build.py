"""Builds the HIP/C-ABI shared library in-tree for gfx950 (no JIT cache: the .so travels with the repo snapshot)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "liblpslam_hip.so")
HIP_SOURCES = ["api.hip", "frontend.hip", "match.hip", "ba.hip", "pose_opt.hip", "sim3.hip", "bow.hip", "share.hip", "occupancy.hip", "jpeg.hip", "jpeg_dec.hip", "intensity.hip", "ingest.hip", "triangulate.hip", "pnp.hip", "two_view.hip", "pose_cov.hip"]
# -ffp-contract=off: parity with the CPU definition forbids FMA contraction ("Numerics").
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


OBJ_DIR = os.path.join(CSRC, "_obj")
# What each translation unit includes, directly or through another include, beyond itself and COMMON_DEPS: a change there recompiles
# only the units that list it.  tests/test_abi_cpu.py follows the #include lines and fails when an entry is missing.
_HOST = os.path.join("..", "host")
UNIT_DEPS = {
    "api.hip": ["fisheye_math.h", "radtan_math.h"],
    "frontend.hip": ["orb_pattern.inc", "fisheye_math.h", "radtan_math.h"],
    "match.hip": ["desc_wave.h"],
    "ba.hip": ["ba_common.h", "chol_panel.inl", "ba_build.inl", "ba_solve.inl", "ba_band.inl", "ba_update.inl", "ba_host.inl", "ba_partitioned.inl"],
    "pose_opt.hip": ["ba_common.h"],
    "sim3.hip": ["ba_common.h", "epnp_math.h", "jacobi_math.h", "ransac_sample.h", "sim3_math.h"],
    "bow.hip": ["desc_wave.h"],
    "share.hip": [],
    "occupancy.hip": [],
    "intensity.hip": [],
    "ingest.hip": ["ingest_math.h"],
    "triangulate.hip": ["desc_wave.h", "triangulate_math.h", "jacobi_math.h"],
    "pnp.hip": ["epnp_math.h", "jacobi_math.h", "ransac_sample.h", "sim3_math.h", os.path.join(_HOST, "pose_math.h")],
    "two_view.hip": ["two_view_math.h", "triangulate_math.h", "jacobi_math.h", "ransac_sample.h"],
    "pose_cov.hip": ["pose_cov_math.h", "jacobi_math.h"],
    "jpeg.hip": ["jpeg_scan.inl", os.path.join(_HOST, "jpeg_tables.h")],
    "jpeg_dec.hip": ["jpeg_scan.inl", os.path.join(_HOST, "jpeg_header.h"), os.path.join(_HOST, "jpeg_tables.h")],
}
COMMON_DEPS = ["internal.h", os.path.join("..", "..", "include", "lpslam_hip.h")]


def hip_library(force=False, verbose=False):
    """One object per translation unit (compiled in parallel, rebuilt only when its sources changed), then the link."""
    srcs = [s for s in HIP_SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ_DIR, exist_ok=True)
    compile_flags = [f for f in FLAGS if f != "-shared"] + os.environ.get("LPSLAM_HIP_EXTRA_FLAGS", "").split()
    # objects compiled with other flags (a development build with -DLPSLAM_..._STAMPS) are stale whatever their age
    flags_file = os.path.join(OBJ_DIR, "flags.txt")
    flags_now = " ".join(compile_flags)
    if not os.path.exists(flags_file) or open(flags_file).read() != flags_now:
        force = True
    # a tree that travelled with its library but without the per-unit objects (they are not part of a snapshot): the library stands
    # when it is newer than everything it is made from
    if not force and os.path.exists(LIB) and not any(os.path.exists(os.path.join(OBJ_DIR, s.replace(".hip", ".o"))) for s in srcs):
        made_from = [os.path.join(CSRC, d) for s in srcs for d in [s] + UNIT_DEPS.get(s, []) + COMMON_DEPS] + [os.path.abspath(__file__)]
        if all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in made_from if os.path.exists(d)):
            return LIB
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        objs.append(obj)
        deps = [os.path.join(CSRC, d) for d in [src] + UNIT_DEPS.get(src, []) + COMMON_DEPS]
        deps = [d for d in deps if os.path.exists(d)] + [os.path.abspath(__file__)]
        if force or not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in deps):
            cmd = [hipcc] + compile_flags + ["-c", "-o", obj, os.path.join(CSRC, src)]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            jobs.append((cmd, subprocess.Popen(cmd)))
    failed = [cmd for cmd, p in jobs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    with open(flags_file, "w") as f:
        f.write(flags_now)
    if jobs or not os.path.exists(LIB) or any(os.path.getmtime(o) > os.path.getmtime(LIB) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return LIB


HOST_LIB = os.path.join(HERE, "liblpslam.so")
HOST_SOURCES = ["slam_manager.cpp", "hip_tracker.cpp", "interface.cpp", "rectify.cpp", "replay.cpp", "two_view.cpp", "bow.cpp", "jpeg.cpp", "jpeg_device.cpp", "map_file.cpp", "record.cpp", "intensity.cpp", "ingest.cpp", "pnp_batch.cpp", "two_view_batch.cpp", "sim3_batch.cpp", "pose_cov_batch.cpp"]


def host_library(force=False, verbose=False):
    """C++ host mirror of the reference interface (g++), linked against the HIP C-ABI library next to it."""
    hdir = os.path.join(HERE, "host")
    srcs = [os.path.join(hdir, s) for s in HOST_SOURCES]
    deps = srcs + [os.path.join(hdir, h) for h in ("core.h", "json_min.h", "hip_tracker.h", "slam_manager.h", "rectify.h", "replay.h", "two_view.h", "pose_math.h", "bow.h", "jpeg.h", "jpeg_header.h", "jpeg_device.h", "jpeg_tables.h", "map_file.h", "occupancy.h", "record.h", "intensity.h", "ingest.h", os.path.join("..", "csrc", "ingest_math.h"), os.path.join("..", "csrc", "fisheye_math.h"), os.path.join("..", "csrc", "radtan_math.h"), os.path.join("..", "csrc", "triangulate_math.h"), os.path.join("..", "csrc", "epnp_math.h"), os.path.join("..", "csrc", "jacobi_math.h"), os.path.join("..", "csrc", "two_view_math.h"), os.path.join("..", "csrc", "ransac_sample.h"), os.path.join("..", "csrc", "sim3_math.h"), os.path.join("..", "csrc", "pose_cov_math.h"))] + \
        [os.path.join(HERE, "..", "include", h) for h in ("lpslam_types.h", "lpslam_manager.h", "lpslam_hip.h")] + [LIB]
    if not force and os.path.exists(HOST_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(HOST_LIB) for d in deps if os.path.exists(d)):
        return HOST_LIB
    hip_library(force=False, verbose=verbose)
    # -ffp-contract=off: the intensity table's product and sum stay unfused on every target
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-ffp-contract=off", "-Wall", "-Wextra",
           "-Wno-unused-parameter", "-pthread", "-o", HOST_LIB] + srcs + ["-L" + HERE, "-llpslam_hip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return HOST_LIB


if __name__ == "__main__":
    print(hip_library(force="-f" in sys.argv, verbose=True))
    print(host_library(force="-f" in sys.argv, verbose=True))
