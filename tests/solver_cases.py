"""The recorded solver cases of tests/golden/g20_solvers.npz (tools/make_golden_solvers.py writes it, tests/test_solvers_golden_cpu.py
replays it): how a case is run through the C shims of the host library and how cases are packed into the fixture.

A case is (fn, tag, args, arrays): fn names the shim (FUNCTIONS below), args are its scalar arguments, arrays its input arrays.  The
fixture holds three entries: `manifest` (JSON: per case fn, tag, args and for every input and output array its name, dtype, shape and
offset), `blob_in` and `blob_out` (the arrays' raw bytes one after the other)."""
import ctypes as C
import json

import numpy as np


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _sym_eigen(lib, args, a):
    n = args["n"]
    ev = np.zeros(n); vec = np.zeros((n, n))
    lib.lpslam_sym_eigen.restype = None
    lib.lpslam_sym_eigen.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.lpslam_sym_eigen(_p(a["A"]), n, _p(ev), _p(vec))
    return dict(eigval=ev, eigvec=vec)


def _epnp(lib, args, a):
    R = np.zeros(9); t = np.zeros(3)
    lib.lpslam_epnp_solve.restype = C.c_int
    lib.lpslam_epnp_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    ok = lib.lpslam_epnp_solve(_p(a["pw"]), _p(a["uv"]), args["n"], _p(a["cam"]), _p(R), _p(t))
    return dict(ok=np.array([ok], np.int32), R=R, t=t)


def _pnp_ransac(lib, args, a):
    n = args["n"]
    pose = np.zeros(7); pose[0] = 1.0
    inl = np.zeros(max(n, 1), np.uint8)
    f = lib.lpslam_pnp_solve_ransac
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    got = f(_p(a["pw"]), _p(a["obs"]), _p(a["w"]), n, _p(a["cam"]), args["iterations"], args["seed"], _p(pose), _p(inl))
    return dict(count=np.array([got], np.int32), pose7=pose, inlier=inl)


def _sim3_ransac(lib, args, a):
    n = args["n"]
    s12 = np.zeros(8); inl = np.zeros(max(n, 1), np.uint8)
    f = lib.lpslam_sim3_solve_ransac
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    got = f(_p(a["p1c"]), _p(a["p2c"]), _p(a["obs1"]), _p(a["obs2"]), _p(a["is1"]), _p(a["is2"]), n, _p(a["cam"]), _p(a["cam"]), args["fix_scale"],
            args["iterations"], args["seed"], _p(s12), _p(inl))
    return dict(count=np.array([got], np.int32), s12=s12, inlier=inl)


def _two_view(lib, args, a):
    n = args["n"]
    o = dict(ok=np.zeros(1, np.int32), R=np.zeros(9), t=np.zeros(3), H=np.zeros(9), F=np.zeros(9), scores=np.zeros(2), parallax_deg=np.zeros(1),
             model=np.zeros(1, np.int32), inlier=np.zeros(n, np.uint8), triangulated=np.zeros(n, np.uint8), points=np.zeros((n, 3)))
    f = lib.lpslam_two_view_initialize
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_uint32] + [C.c_void_p] * 10
    o["ok"][0] = f(_p(a["K"]), _p(a["kp_ref"]), _p(a["kp_cur"]), _p(a["matches"]), n, args["sigma"], args["iterations"], args["seed"], _p(o["R"]), _p(o["t"]),
                   _p(o["H"]), _p(o["F"]), _p(o["scores"]), _p(o["parallax_deg"]), _p(o["model"]), _p(o["inlier"]), _p(o["triangulated"]), _p(o["points"]))
    return o


FUNCTIONS = {"sym_eigen": _sym_eigen, "epnp": _epnp, "pnp_ransac": _pnp_ransac, "sim3_ransac": _sim3_ransac, "two_view": _two_view}


def run(lib, fn, args, arrays):
    """the outputs (name -> array) of one case; `arrays` are C-contiguous arrays of the dtypes the shim reads"""
    return FUNCTIONS[fn](lib, args, arrays)


def _pack(named, blob, seen):
    index = []
    for name, arr in named.items():
        arr = np.ascontiguousarray(arr)
        raw = arr.tobytes()
        if raw not in seen:                  # cases that share an input share its bytes
            seen[raw] = len(blob)
            blob += raw
        index.append([name, arr.dtype.str, list(arr.shape), seen[raw]])
    return index


def save(path, cases, outputs):
    """cases: list of (fn, tag, args, arrays); outputs: per case the dict run() returned"""
    blob_in, blob_out, seen_in, seen_out, manifest = bytearray(), bytearray(), {}, {}, []
    for (fn, tag, args, arrays), out in zip(cases, outputs):
        manifest.append({"fn": fn, "tag": tag, "args": args, "in": _pack(arrays, blob_in, seen_in), "out": _pack(out, blob_out, seen_out)})
    np.savez_compressed(path, manifest=np.frombuffer(json.dumps(manifest).encode(), np.uint8), blob_in=np.frombuffer(bytes(blob_in), np.uint8),
                        blob_out=np.frombuffer(bytes(blob_out), np.uint8))


def _unpack(index, blob):
    out = {}
    for name, dtype, shape, offset in index:
        dt = np.dtype(dtype)
        count = int(np.prod(shape))
        out[name] = np.frombuffer(blob, dt, count, offset).reshape(shape).copy()
    return out


def load(path):
    """list of (fn, tag, args, arrays, recorded outputs)"""
    z = np.load(path)
    blob_in, blob_out = z["blob_in"].tobytes(), z["blob_out"].tobytes()
    return [(m["fn"], m["tag"], m["args"], _unpack(m["in"], blob_in), _unpack(m["out"], blob_out)) for m in json.loads(z["manifest"].tobytes().decode())]
