"""CPU tests of the host's pose algebra (lpslam_amd/host/pose_math.h through its C shim in liblpslam.so) against a numpy float64
restatement: world -> camera poses as (quaternion w x y z, translation), x_c = R x_w + t.

Tolerance: 1e-12 absolute on unit-scale values.  An expression of at most about 20 double operations rounds within about
20 x 1.1e-16 = 2e-15; a swapped index, sign or transpose gives an error of order 0.1 to 1."""
import ctypes as C

import numpy as np
import pytest

TOL = 1e-12


@pytest.fixture(scope="module")
def lib():
    from lpslam_amd import _build
    l = C.CDLL(_build.host_library())
    for name, n_args in (("lpslam_pose_compose", 3), ("lpslam_pose_inverse", 2), ("lpslam_pose_relative", 3), ("lpslam_pose_centre", 2),
                         ("lpslam_quat_to_rot", 2), ("lpslam_rot_to_quat", 2)):
        getattr(l, name).restype = None
        getattr(l, name).argtypes = [C.c_void_p] * n_args
    return l


def _call(fn, n_out, *args):
    out = np.zeros(n_out)
    fn(*[np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p) for a in args], out.ctypes.data_as(C.c_void_p))
    return out


def np_rot(q):
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def np_quat(r):
    """Eigen::Quaterniond(R): the branch follows the trace, then the largest diagonal element."""
    tr = np.trace(r)
    if tr > 0:
        s = 2 * np.sqrt(tr + 1)
        return np.array([s / 4, (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s])
    i = int(np.argmax(np.diag(r)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = 2 * np.sqrt(1 + r[i, i] - r[j, j] - r[k, k])
    q = np.zeros(4)
    q[0] = (r[k, j] - r[j, k]) / s
    q[1 + i] = s / 4
    q[1 + j] = (r[j, i] + r[i, j]) / s
    q[1 + k] = (r[k, i] + r[i, k]) / s
    return q


def np_compose(a, b):
    """a after b, as (R, t)."""
    return a[0] @ b[0], a[0] @ b[1] + a[1]


def np_inverse(a):
    return a[0].T, -a[0].T @ a[1]


def _rt(p7):
    return np_rot(p7[:4]), np.asarray(p7[4:], float)


def _assert_pose(p7, r, t):
    """The pose's rotation and translation: compared as matrices, since a quaternion, its negative and (for the entry points
    that normalise on the way in) any positive multiple of it are the same rotation."""
    assert np.abs(np_rot(p7[:4]) - r).max() < TOL and np.abs(p7[4:] - t).max() < TOL


@pytest.fixture(scope="module")
def poses():
    rng = np.random.default_rng(20261019)
    q = rng.normal(size=(200, 4))
    q *= (rng.uniform(0.5, 2.0, 200) / np.linalg.norm(q, axis=1))[:, None]      # norms 0.5 .. 2: every entry point normalises
    return np.hstack([q, rng.uniform(-1, 1, (200, 3))])


def branch_rotations():
    """One rotation per branch of rotToQuat: trace > 0, then the x, y and z diagonal element largest (rotations by about 180
    degrees about an axis close to x, y, z)."""
    out = [("trace", np_rot([0.9, 0.2, -0.3, 0.1]))]
    for name, axis in (("x", [1.0, 0.05, -0.03]), ("y", [0.04, 1.0, 0.02]), ("z", [-0.02, 0.03, 1.0])):
        ang = np.pi - 0.05
        ax = np.asarray(axis) / np.linalg.norm(axis)
        out.append((name, np_rot(np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax]))))
    return out


def test_branch_rotations_reach_every_branch():
    rs = dict(branch_rotations())
    assert np.trace(rs["trace"]) > 0
    for i, name in enumerate("xyz"):
        assert np.trace(rs[name]) < 0 and int(np.argmax(np.diag(rs[name]))) == i


def test_quat_to_rot_matches_numpy(lib, poses):
    for p in poses:
        assert np.abs(_call(lib.lpslam_quat_to_rot, 9, p[:4]).reshape(3, 3) - np_rot(p[:4])).max() < TOL


def test_compose_with_inverse_is_identity(lib, poses):
    for p in poses:
        inv = _call(lib.lpslam_pose_inverse, 7, p)
        _assert_pose(inv, *np_inverse(_rt(p)))
        _assert_pose(_call(lib.lpslam_pose_compose, 7, p, inv), np.eye(3), np.zeros(3))
        _assert_pose(_call(lib.lpslam_pose_compose, 7, inv, p), np.eye(3), np.zeros(3))


def test_compose_matches_numpy(lib, poses):
    for a, b in zip(poses, np.roll(poses, 1, axis=0)):
        _assert_pose(_call(lib.lpslam_pose_compose, 7, a, b), *np_compose(_rt(a), _rt(b)))


def test_relative_is_compose_with_inverse(lib, poses):
    for a, b in zip(poses, np.roll(poses, 7, axis=0)):
        rel = _call(lib.lpslam_pose_relative, 7, a, b)
        via = _call(lib.lpslam_pose_compose, 7, a, _call(lib.lpslam_pose_inverse, 7, b))
        _assert_pose(rel, *_rt(via))
        _assert_pose(rel, *np_compose(_rt(a), np_inverse(_rt(b))))


def test_centre_is_minus_rt_t(lib, poses):
    for p in poses:
        r, t = _rt(p)
        assert np.abs(_call(lib.lpslam_pose_centre, 3, p) - (-r.T @ t)).max() < TOL


def test_rot_to_quat_round_trip_and_numpy(lib, poses):
    cases = [r for _, r in branch_rotations()] + [np_rot(p[:4]) for p in poses]
    for r in cases:
        q = _call(lib.lpslam_rot_to_quat, 4, r.ravel())
        assert np.abs(_call(lib.lpslam_quat_to_rot, 9, q).reshape(3, 3) - r).max() < TOL
        want = np_quat(r)
        assert min(np.abs(q - want).max(), np.abs(q + want).max()) < TOL
