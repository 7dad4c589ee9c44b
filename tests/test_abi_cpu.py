"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports exactly what
include/lpslam_hip.h declares; without a GPU the product fails loudly instead of falling back."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "lpslam_hip.h")).read()
    return sorted(set(re.findall(r"\b(lpslam_hip_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(hiplib):
    lib = hiplib.load()
    declared = _declared()
    assert len(declared) >= 40
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(hiplib.SYMBOLS) == declared


def test_code_object_targets_gfx950(hiplib):
    data = open(hiplib.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"gfx942" not in data and b"sm_" not in data


def test_no_cpu_fallback_without_device(hiplib):
    if hiplib.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(hiplib.LpslamHipError) as e:
        hiplib.Context(640, 480)
    assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)


def test_product_does_not_reference_the_oracle():
    bad = []
    for d in ("lpslam_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp", ".inc")):
                    t = open(os.path.join(dp, f), errors="ignore").read()
                    if re.search(r"(from|import)\s+oracle|oracle/|liblpslam_oracle|ora_[a-z]+\(", t):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_keypoint_layout_matches_cv_keypoint(hiplib):
    assert hiplib.KP_DTYPE.itemsize == 28 and hiplib.KP_DTYPE.names == ("x", "y", "size", "angle", "response", "octave", "class_id")
    assert hiplib.BA_OBS_DTYPE.itemsize == 40


def test_reference_header_client_links():
    """tests/golden/abi_symbols.txt holds the mangled names a client compiled against the REFERENCE's own interface headers
    (src/Interface/LpSlamManager.h:17-121, LpSlamConfiguration.h) leaves undefined -- made by tools/make_abi_symbols.py in the
    build container, where the same client is also linked and loaded against the product library.  Every one of them must be a
    defined dynamic symbol of lpslam_amd/liblpslam.so: that is what "existing clients relink unchanged" means."""
    import subprocess
    from lpslam_amd import _build
    lib = _build.host_library()
    want = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "abi_symbols.txt")) if l.strip()]
    assert len(want) == 37 and sum("LpSlamManager" in s for s in want) == 36
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    missing = [s for s in want if s not in have]
    assert not missing, missing


def test_unit_deps_cover_every_include():
    """Every file a translation unit reaches through its #include "..." lines (followed transitively, each resolved relative to the
    including file) is in that unit's UNIT_DEPS or in COMMON_DEPS: an entry missing there means an edit to the file leaves the
    unit's stale object in the library."""
    from lpslam_amd import _build

    def reached(path, seen):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
            f = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            assert os.path.exists(f), "%s includes %s, which does not exist" % (path, inc)
            if f not in seen:
                seen.add(f)
                reached(f, seen)
        return seen

    assert sorted(_build.UNIT_DEPS) == sorted(_build.HIP_SOURCES)
    for src in _build.HIP_SOURCES:
        listed = {os.path.normpath(os.path.join(_build.CSRC, d)) for d in _build.UNIT_DEPS[src] + _build.COMMON_DEPS}
        assert all(os.path.exists(d) for d in listed), (src, sorted(d for d in listed if not os.path.exists(d)))
        missing = sorted(reached(os.path.join(_build.CSRC, src), set()) - listed)
        assert not missing, "%s: not in UNIT_DEPS / COMMON_DEPS: %s" % (src, missing)


def test_environment_switches_are_the_documented_ones():
    """The LPSLAM_HIP_* variables the library and the host plugin read -- every name inside a getenv(...) call or given to
    env_us(...) under lpslam_amd/csrc and lpslam_amd/host -- are exactly those of the "environment switches" block of
    include/lpslam_hip.h, and the list stays short: at most 12 behaviour switches and 4 development traces."""
    read = set()
    for d in ("csrc", "host"):
        for dp, _, files in os.walk(os.path.join(ROOT, "lpslam_amd", d)):
            for f in files:
                if f.endswith((".hip", ".inl", ".inc", ".h", ".cpp")):
                    read |= set(re.findall(r'\b(?:getenv|env_us)\s*\(\s*"(LPSLAM_HIP_[A-Z0-9_]+)"', open(os.path.join(dp, f), errors="ignore").read()))
    header = open(os.path.join(ROOT, "include", "lpslam_hip.h")).read()
    block = re.search(r"/\* ---- environment switches -+\n(.*?)\*/", header, re.S)
    assert block, "include/lpslam_hip.h has no environment-switch block"
    behaviour, traces = block.group(1).split("Development traces")
    behaviour = re.findall(r"^ \*   (LPSLAM_HIP_[A-Z0-9_]+)\s", behaviour, re.M)
    traces = re.findall(r"^ \*   (LPSLAM_HIP_[A-Z0-9_]+)\s", traces, re.M)
    assert len(set(behaviour + traces)) == len(behaviour + traces), "a switch is listed twice"
    assert read == set(behaviour + traces), (sorted(read - set(behaviour + traces)), sorted(set(behaviour + traces) - read))
    assert len(behaviour) <= 12 and len(traces) <= 4, (len(behaviour), len(traces))
    assert all(t.endswith("_TRACE") for t in traces) and not any(b.endswith("_TRACE") for b in behaviour)
