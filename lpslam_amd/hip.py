"""ctypes binding of the C ABI in include/lpslam_hip.h (lpslam_amd/liblpslam_hip.so).

This is the thin Python face of the HIP library used by the tests and bench.py; the product's host side is the
C++ mirror of the reference interface in lpslam_amd/host/.  There is no CPU fallback: a missing library or a
missing GPU raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LPSLAM_HIP_LIB") or os.path.join(_HERE, "liblpslam_hip.so")      # the override: A/B timing of two builds on one box
MAX_LEVELS = 16

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CORNER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("score", "<i4")])
BA_OBS_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("u", "<f8"), ("v", "<f8"), ("ur", "<f8"),
                         ("inv_sigma2", "<f8")])
SIM3_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("meas", "<f8", (8,))])
SIM3_PAIR_DTYPE = np.dtype([("p1c", "<f8", (3,)), ("p2c", "<f8", (3,)), ("obs1", "<f8", (2,)), ("obs2", "<f8", (2,)),
                            ("inv_sigma2_1", "<f8"), ("inv_sigma2_2", "<f8")])
TRI_KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("x_right", "<f4"), ("depth", "<f4")])      # lpslam_hip_tri_keypoint
PROJ_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("x_right", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4")])
SCAN_POSE_DTYPE = np.dtype([("key", "<i4"), ("pad", "<i4"), ("origin", "<f8", (2,)), ("fwd", "<f8", (2,)), ("left", "<f8", (2,))])
BA_LOG_DTYPE = np.dtype([("chi2_before", "<f8"), ("chi2_after", "<f8"), ("lambda", "<f8"),
                         ("trials", "<i4"), ("status", "<i4")])

# every symbol include/lpslam_hip.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "lpslam_hip_last_error", "lpslam_hip_device_count", "lpslam_hip_create", "lpslam_hip_destroy",
    "lpslam_hip_stream", "lpslam_hip_set_mapping_reserve", "lpslam_hip_set_flat_priorities", "lpslam_hip_debug_occupy_unreserved", "lpslam_hip_sync", "lpslam_hip_timer_begin", "lpslam_hip_timer_end", "lpslam_hip_timer_read", "lpslam_hip_level_info", "lpslam_hip_max_keypoints_per_image",
    "lpslam_hip_image_ptr", "lpslam_hip_upload_image", "lpslam_hip_host_alloc", "lpslam_hip_host_free", "lpslam_hip_host_register", "lpslam_hip_host_unregister", "lpslam_hip_upload_images_async", "lpslam_hip_set_rectify_map", "lpslam_hip_set_mask", "lpslam_hip_upload_raw_image", "lpslam_hip_remap_staged", "lpslam_hip_extract", "lpslam_hip_extract_range", "lpslam_hip_stage_pyramid",
    "lpslam_hip_stage_fast", "lpslam_hip_stage_distribute", "lpslam_hip_stage_describe",
    "lpslam_hip_keypoint_count", "lpslam_hip_get_keypoints", "lpslam_hip_get_frame", "lpslam_hip_get_pyramid_level",
    "lpslam_hip_get_candidates", "lpslam_hip_keypoint_buffers", "lpslam_hip_match_bf", "lpslam_hip_get_bf_knn2",
    "lpslam_hip_get_bf_matches", "lpslam_hip_match_bf_strided", "lpslam_hip_set_descriptors",
    "lpslam_hip_match_stereo", "lpslam_hip_match_stereo_strided", "lpslam_hip_get_stereo",
    "lpslam_hip_vocab_create", "lpslam_hip_vocab_destroy", "lpslam_hip_vocab_info", "lpslam_hip_bow_transform", "lpslam_hip_bow_transform_host", "lpslam_hip_match_bow_tree", "lpslam_hip_match_bow_tree_multi",
    "lpslam_hip_match_projection", "lpslam_hip_match_fuse", "lpslam_hip_match_area", "lpslam_hip_window_match_rescans", "lpslam_hip_match_orientation_filter",
    "lpslam_hip_ba_create", "lpslam_hip_ba_prepare", "lpslam_hip_ba_build_batch", "lpslam_hip_ba_destroy", "lpslam_hip_ba_set_active", "lpslam_hip_ba_optimize", "lpslam_hip_ba_optimize_begin", "lpslam_hip_ba_optimize_end", "lpslam_hip_ba_graph_replays", "lpslam_hip_ba_wg_factorisations", "lpslam_hip_ba_debug_solve", "lpslam_hip_pose_optimize_passes", "lpslam_hip_match_bf_descriptors", "lpslam_hip_prefetch_frame", "lpslam_hip_get_frame_view", "lpslam_hip_desc_store_put", "lpslam_hip_desc_store_drop", "lpslam_hip_match_bf_stored", "lpslam_hip_desc_store_mask", "lpslam_hip_rank_stored", "lpslam_hip_ba_set_state_batch", "lpslam_hip_ba_get_batch", "lpslam_hip_ba_get_solver", "lpslam_hip_ba_get_schur_part", "lpslam_hip_ba_set_solver", "lpslam_hip_ba_timeouts", "lpslam_hip_ba_counters", "lpslam_hip_set_shared_launches", "lpslam_hip_shared_launch_counters", "lpslam_hip_create_session", "lpslam_hip_front_end", "lpslam_hip_frame_done", "lpslam_hip_front_end_images", "lpslam_hip_shared_front_end_counters", "lpslam_hip_shared_solve_counters", "lpslam_hip_ba_local_window",
    "lpslam_hip_ba_optimize_batch", "lpslam_hip_ba_reset_batch", "lpslam_hip_ba_optimize_profiled", "lpslam_hip_ba_optimize_partitioned", "lpslam_hip_ba_optimize_partitioned_with",
    "lpslam_hip_ba_local", "lpslam_hip_ba_set_points_fixed", "lpslam_hip_ba_pose_optimize", "lpslam_hip_pose_optimize", "lpslam_hip_ba_reset", "lpslam_hip_ba_set_state", "lpslam_hip_prefetch_begin", "lpslam_hip_prefetch_end", "lpslam_hip_prefetch_join", "lpslam_hip_ba_get", "lpslam_hip_ba_chi2", "lpslam_hip_ba_reduced_buffer",
    "lpslam_hip_ba_step_begin", "lpslam_hip_ba_step_lambda0", "lpslam_hip_ba_step_solve", "lpslam_hip_ba_scalar_buffer", "lpslam_hip_ba_step_end", "lpslam_hip_ba_status",
    "lpslam_hip_sim3_create", "lpslam_hip_sim3_destroy", "lpslam_hip_sim3_optimize", "lpslam_hip_sim3_get", "lpslam_hip_sim3_chi2", "lpslam_hip_sim3_transform_optimize",
    "lpslam_hip_sim3_ransac_batch", "lpslam_hip_sim3_verify_batch",
    "lpslam_hip_scan_geometry_put", "lpslam_hip_scan_store_put", "lpslam_hip_scan_store_drop", "lpslam_hip_occupancy_build",
    "lpslam_hip_jpeg_create", "lpslam_hip_jpeg_destroy", "lpslam_hip_jpeg_encode",
    "lpslam_hip_jpeg_dec_create", "lpslam_hip_jpeg_dec_create2", "lpslam_hip_jpeg_dec_destroy", "lpslam_hip_jpeg_decode", "lpslam_hip_jpeg_dec_last",
    "lpslam_hip_jpeg_dec_take_restart",
    "lpslam_hip_adjust_intensity", "lpslam_hip_upload_raw_image_adjusted", "lpslam_hip_front_end_images_adjusted", "lpslam_hip_adjust_intensity_last",
    "lpslam_hip_upload_pixels", "lpslam_hip_upload_raw_pixels", "lpslam_hip_front_end_pixels",
    "lpslam_hip_set_keypoint_camera", "lpslam_hip_stage_undistort", "lpslam_hip_undistort_dropped", "lpslam_hip_undistort_points",
    "lpslam_hip_set_keypoint_camera_radtan", "lpslam_hip_undistort_points_radtan",
    "lpslam_hip_triangulate_neighbours", "lpslam_hip_triangulate_pairs",
    "lpslam_hip_pnp_ransac_batch",
    "lpslam_hip_two_view_ransac_batch", "lpslam_hip_two_view_check_poses",
    "lpslam_hip_pose_covariance_batch",
]


class GridInfo(C.Structure):
    _fields_ = [("x0", C.c_int64), ("y0", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("rays", C.c_int64), ("cell_visits", C.c_int64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class LpslamHipError(RuntimeError):
    pass


class FrontendConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_keypoints", C.c_int32),
                ("scale_factor", C.c_float), ("num_levels", C.c_int32), ("ini_fast_threshold", C.c_int32),
                ("min_fast_threshold", C.c_int32), ("max_images", C.c_int32), ("device", C.c_int32)]


class Fisheye(C.Structure):
    """lpslam_hip_fisheye: intrinsics, k1 .. k4 and the angle limit in radians"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 4), ("max_angle", C.c_double)]

    def __init__(self, fx, fy, cx, cy, k=(0.0, 0.0, 0.0, 0.0), max_angle_deg=70.0):
        super().__init__(float(fx), float(fy), float(cx), float(cy), (C.c_double * 4)(*[float(v) for v in k]), float(np.deg2rad(max_angle_deg)))


class Radtan(C.Structure):
    """lpslam_hip_radtan: intrinsics and the radial-tangential coefficients k1, k2, p1, p2, k3"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double)]

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        super().__init__(float(fx), float(fy), float(cx), float(cy), float(k1), float(k2), float(p1), float(p2), float(k3))


class TriCamera(C.Structure):
    """lpslam_hip_tri_camera: focal_x_baseline 0 = a monocular camera"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("focal_x_baseline", C.c_double), ("scale_factor", C.c_double)]

    def __init__(self, fx, fy, cx, cy, focal_x_baseline=0.0, scale_factor=1.2):
        super().__init__(float(fx), float(fy), float(cx), float(cy), float(focal_x_baseline), float(scale_factor))


class TriSet(C.Structure):
    """lpslam_hip_tri_set: one neighbour keyframe in host memory"""
    _fields_ = [("kpts", C.c_void_p), ("desc32", C.c_void_p), ("group", C.c_void_p), ("x_right", C.c_void_p), ("depth", C.c_void_p), ("n", C.c_int32),
                ("pose", C.c_double * 7), ("F", C.c_double * 9), ("epipole", C.c_double * 2), ("has_epipole", C.c_int32)]


class BaCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("focal_x_baseline", C.c_double), ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


class AdjustParams(C.Structure):
    """lpslam_hip_adjust_params; the defaults are the reference's constants"""
    _fields_ = [("low_out", C.c_double), ("high_out", C.c_double), ("low_fraction", C.c_double), ("high_fraction", C.c_double)]

    def __init__(self, low_out=-0.3, high_out=1.4, low_fraction=0.01, high_fraction=0.99):
        super().__init__(float(low_out), float(high_out), float(low_fraction), float(high_fraction))


PIXEL_GRAY8, PIXEL_RGB8, PIXEL_BGR8, PIXEL_NV12, PIXEL_UYVY = range(5)          # LPSLAM_HIP_PIXEL_*


class Pixels(C.Structure):
    """lpslam_hip_pixels: one frame as it came.  `arr` (kept alive by the object) holds the bytes: (h, w) for GRAY8, (h, w, 3) for
    RGB8 / BGR8, (h, 2 w) for UYVY, (3 h / 2, w) for NV12 (the chroma rows right behind the Y plane) -- or, with `chroma`, (h, w)
    and an array of (h / 2, w) chroma rows of its own.  Rows may be strided (a view of a wider array)."""
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int32), ("chroma", C.c_void_p), ("chroma_stride", C.c_int32), ("format", C.c_int32)]

    def __init__(self, arr, fmt, chroma=None, stride=None):
        assert arr.dtype == np.uint8
        self.arr, self.chroma_arr = arr, chroma
        super().__init__(arr.ctypes.data, int(arr.strides[0]) if stride is None else int(stride),
                         None if chroma is None else chroma.ctypes.data, 0 if chroma is None else int(chroma.strides[0]), int(fmt))


class BaKernelTimes(C.Structure):
    _fields_ = [("ms", C.c_float * 8), ("launches", C.c_int32 * 8), ("launches_per_mark", C.c_int32 * 8), ("iterations", C.c_int32), ("dim", C.c_int32)]


_lib = None


def load():
    """Loads the in-tree HIP library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LpslamHipError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(hipcc --offload-arch=gfx950); the lpslam hot path has no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.lpslam_hip_last_error.restype = C.c_char_p
        _lib.lpslam_hip_stream.restype = C.c_void_p
        _lib.lpslam_hip_stream.argtypes = [C.c_void_p]
        for name in ("lpslam_hip_match_stereo",):
            getattr(_lib, name).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
        _lib.lpslam_hip_match_stereo_strided.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        _lib.lpslam_hip_match_bf_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        _lib.lpslam_hip_get_bf_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_float, C.c_int32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    return _lib


def _check(rc):
    if rc != 0:
        raise LpslamHipError("lpslam_hip error %d: %s" % (rc, load().lpslam_hip_last_error().decode()))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def set_flat_priorities(flat, late_ok=False):
    """process-wide: streams of contexts created from now on at the default priority (True) or in the three classes (False); None: the environment.
    True after a priority stream exists in the process is refused (RuntimeError) unless late_ok"""
    _check(load().lpslam_hip_set_flat_priorities(C.c_int32(-1 if flat is None else ((2 if late_ok else 1) if flat else 0))))


def set_shared_launches(mode):
    """process-wide: launches shared by the sessions of a process -- 0 never, 1 always, 2 when two or more sessions are tracking (default), None: the environment"""
    _check(load().lpslam_hip_set_shared_launches(C.c_int32(-1 if mode is None else int(mode))))


def shared_launch_counters(device=0):
    b, r = C.c_int64(0), C.c_int64(0)
    _check(load().lpslam_hip_shared_launch_counters(C.c_int32(device), C.byref(b), C.byref(r)))
    return b.value, r.value


def shared_front_end_counters(device=0):
    b, r = C.c_int64(0), C.c_int64(0)
    _check(load().lpslam_hip_shared_front_end_counters(C.c_int32(device), C.byref(b), C.byref(r)))
    return b.value, r.value


def shared_solve_counters(device=0):
    b, r = C.c_int64(0), C.c_int64(0)
    _check(load().lpslam_hip_shared_solve_counters(C.c_int32(device), C.byref(b), C.byref(r)))
    return b.value, r.value


def device_count():
    n = C.c_int(0)
    rc = load().lpslam_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class Context:
    """One front-end context = one GPU, one stream, `max_images` resident image slots."""

    def __init__(self, width, height, max_keypoints=2000, scale_factor=1.2, num_levels=8, ini_thr=20, min_thr=7,
                 max_images=2, device=0, session=False):
        self.lib = load()
        self.cfg = FrontendConfig(width, height, max_keypoints, scale_factor, num_levels, ini_thr, min_thr, max_images, device)
        h = C.c_void_p()
        # session: a slice of the device's session pool (lpslam_hip_create_session: what a tracker plugin creates)
        _check((self.lib.lpslam_hip_create_session if session else self.lib.lpslam_hip_create)(C.byref(self.cfg), C.byref(h)))
        self.h = h
        self.max_kp = self.lib.lpslam_hip_max_keypoints_per_image(self.h)
        L = num_levels
        w = (C.c_int32 * MAX_LEVELS)(); hh = (C.c_int32 * MAX_LEVELS)(); p = (C.c_int32 * MAX_LEVELS)()
        q = (C.c_int32 * MAX_LEVELS)(); s = (C.c_float * MAX_LEVELS)()
        _check(self.lib.lpslam_hip_level_info(self.h, w, hh, p, q, s))
        self.level_w, self.level_h, self.level_pitch = list(w[:L]), list(hh[:L]), list(p[:L])
        self.quota, self.scale = list(q[:L]), list(s[:L])
        import weakref
        self._children = weakref.WeakSet()      # objects that hand memory back to this context when they are destroyed

    def close(self):
        if getattr(self, "h", None):
            for child in list(getattr(self, "_children", ())):
                child.close()
            self.lib.lpslam_hip_destroy(self.h)
            self.h = None

    __del__ = close

    @property
    def stream(self):
        return self.lib.lpslam_hip_stream(self.h)

    def sync(self):
        _check(self.lib.lpslam_hip_sync(self.h))

    def front_end(self, image, stereo, fxb=0.0, baseline=0.0):
        """extraction of the slot (pair), stereo match and delivery of the frame's results as one asynchronous call"""
        f = self.lib.lpslam_hip_front_end
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_float, C.c_float]
        _check(f(self.h, int(image), 1 if stereo else 0, float(fxb), float(baseline)))

    def front_end_images(self, image, left, right=None, fxb=0.0, baseline=0.0):
        """upload of the frame into the slot (pair) + front_end, as one asynchronous call"""
        f = self.lib.lpslam_hip_front_end_images
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float]
        left = np.ascontiguousarray(left); right = None if right is None else np.ascontiguousarray(right)
        _check(f(self.h, int(image), _p(left), None if right is None else _p(right), left.shape[1], float(fxb), float(baseline)))

    def front_end_images_adjusted(self, image, left, right=None, fxb=0.0, baseline=0.0, params=None):
        """front_end_images with the intensity adjustment of the slot (pair) between the uploads and the front end"""
        f = self.lib.lpslam_hip_front_end_images_adjusted
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.POINTER(AdjustParams)]
        left = np.ascontiguousarray(left); right = None if right is None else np.ascontiguousarray(right)
        p = params if params is not None else AdjustParams()
        _check(f(self.h, int(image), _p(left), None if right is None else _p(right), left.shape[1], float(fxb), float(baseline), C.byref(p)))

    def front_end_pixels(self, image, left, right=None, fxb=0.0, baseline=0.0, params=None):
        """the colour form of front_end_images / front_end_images_adjusted: left, right are Pixels (right None: monocular), params an
        AdjustParams or None (no adjustment)"""
        f = self.lib.lpslam_hip_front_end_pixels
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.POINTER(Pixels), C.POINTER(Pixels), C.c_float, C.c_float, C.POINTER(AdjustParams)]
        _check(f(self.h, int(image), C.byref(left), None if right is None else C.byref(right), float(fxb), float(baseline),
                 None if params is None else C.byref(params)))

    def upload_pixels(self, image, pixels):
        """the colour form of upload: a Pixels into a slot, converted to grey on the device"""
        f = self.lib.lpslam_hip_upload_pixels
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.POINTER(Pixels)]
        _check(f(self.h, int(image), C.byref(pixels)))
        self.sync()

    def upload_raw_pixels(self, image, eye, pixels, params=None):
        """the colour form of upload_raw / upload_raw_adjusted (params an AdjustParams or None): convert, adjust, remap"""
        f = self.lib.lpslam_hip_upload_raw_pixels
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.POINTER(Pixels), C.POINTER(AdjustParams)]
        _check(f(self.h, int(image), int(eye), C.byref(pixels), None if params is None else C.byref(params)))
        self.sync()

    def adjust_intensity(self, first, n, params=None):
        """image slots [first, first + n) adjusted in place on level 0 (asynchronous; AdjustParams, default: the reference's constants)"""
        f = self.lib.lpslam_hip_adjust_intensity
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(AdjustParams)]
        p = params if params is not None else AdjustParams()
        _check(f(self.h, int(first), int(n), C.byref(p)))

    def adjust_intensity_last(self, image):
        """test hook (synchronising): (lo, hi, the 256 histogram words) of the last adjustment of a slot"""
        f = self.lib.lpslam_hip_adjust_intensity_last
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        lo, hi = C.c_int32(), C.c_int32()
        hist = np.zeros(256, np.uint32)
        _check(f(self.h, int(image), C.byref(lo), C.byref(hi), _p(hist)))
        return lo.value, hi.value, hist

    def upload_raw_adjusted(self, image, eye, arr, params=None):
        """upload_raw with the raw frame adjusted before it is remapped"""
        arr = np.ascontiguousarray(arr, np.uint8)
        assert arr.shape == (self.cfg.height, self.cfg.width), arr.shape
        f = self.lib.lpslam_hip_upload_raw_image_adjusted
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(AdjustParams)]
        p = params if params is not None else AdjustParams()
        _check(f(self.h, int(image), int(eye), _p(arr), arr.shape[1], C.byref(p)))
        self.sync()

    def set_mapping_reserve(self, cus_per_xcd):
        """compute units of every XCD the front end's kernels leave to the bundle adjustments that run beside them (idle context)"""
        f = self.lib.lpslam_hip_set_mapping_reserve
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int32]
        _check(f(self.h, int(cus_per_xcd)))

    def debug_occupy_unreserved(self, microseconds):
        """Test hook: every compute unit outside the mapping reserve is held (whole LDS) for `microseconds`; returns how many are."""
        n = C.c_int32(0)
        _check(self.lib.lpslam_hip_debug_occupy_unreserved(self.h, C.c_int32(int(microseconds)), C.byref(n)))
        return n.value

    def ba_counters(self):
        """totals over every bundle-adjustment problem of this context: signatures in the graph cache, graphs built, replays, timed-out hand-overs (band, update)"""
        out = (C.c_int64 * 5)()
        _check(self.lib.lpslam_hip_ba_counters(self.h, out, 5))
        return dict(zip(("signatures", "graphs", "replays", "timeouts_band", "timeouts_update"), (int(v) for v in out)))

    def ba_graph_replays(self):
        f = self.lib.lpslam_hip_ba_graph_replays
        f.restype = C.c_int64; f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def ba_wg_factorisations(self):
        f = self.lib.lpslam_hip_ba_wg_factorisations
        f.restype = C.c_int64; f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def pose_optimize_passes(self):
        f = self.lib.lpslam_hip_pose_optimize_passes
        f.restype = C.c_int32; f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def timer_begin(self, slot):
        _check(self.lib.lpslam_hip_timer_begin(self.h, slot))

    def timer_end(self, slot):
        _check(self.lib.lpslam_hip_timer_end(self.h, slot))

    def timer_ms(self, slot):
        ms = C.c_float()
        _check(self.lib.lpslam_hip_timer_read(self.h, slot, C.byref(ms)))
        return ms.value

    def image_ptr(self, image):
        ptr = C.c_void_p(); pitch = C.c_int32()
        _check(self.lib.lpslam_hip_image_ptr(self.h, image, C.byref(ptr), C.byref(pitch)))
        return ptr.value, pitch.value

    def upload(self, image, arr):
        arr = np.ascontiguousarray(arr, np.uint8)
        assert arr.shape == (self.cfg.height, self.cfg.width), arr.shape
        _check(self.lib.lpslam_hip_upload_image(self.h, image, _p(arr), arr.shape[1]))
        self.sync()      # host array may be freed by the caller

    def host_frame(self, arr=None):
        """a page-locked (height, width) uint8 frame owned by the context (lpslam_hip_host_alloc), optionally filled from `arr`"""
        hgt, wid = self.cfg.height, self.cfg.width
        ptr = C.c_void_p()
        f = self.lib.lpslam_hip_host_alloc
        f.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        _check(f(self.h, hgt * wid, C.byref(ptr)))
        buf = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(hgt, wid))
        if arr is not None:
            buf[...] = arr
        return buf

    def host_free(self, frame):
        f = self.lib.lpslam_hip_host_free
        f.argtypes = [C.c_void_p, C.c_void_p]
        _check(f(self.h, frame.ctypes.data))

    def host_register(self, arr):
        f = self.lib.lpslam_hip_host_register
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        _check(f(self.h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr):
        f = self.lib.lpslam_hip_host_unregister
        f.argtypes = [C.c_void_p, C.c_void_p]
        _check(f(self.h, arr.ctypes.data))

    def upload_async(self, first, frames):
        """lpslam_hip_upload_images_async: frames[i] -> slot first + i on the copy stream; returns at once (the frames must stay
        alive and unchanged until an extraction of the slots has been synchronised)"""
        n = len(frames)
        ptrs = (C.c_void_p * n)(*[fr.ctypes.data for fr in frames])
        for fr in frames:
            assert fr.dtype == np.uint8 and fr.shape == (self.cfg.height, self.cfg.width) and fr.strides[1] == 1, (fr.dtype, fr.shape)
        f = self.lib.lpslam_hip_upload_images_async
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int32]
        _check(f(self.h, int(first), n, ptrs, int(frames[0].strides[0])))

    def set_rectify_map(self, eye, map_x, map_y):
        mx = np.ascontiguousarray(map_x, np.float32); my = np.ascontiguousarray(map_y, np.float32)
        assert mx.shape == (self.cfg.height, self.cfg.width) and my.shape == mx.shape
        _check(self.lib.lpslam_hip_set_rectify_map(self.h, int(eye), _p(mx), _p(my)))

    def set_mask(self, eye, mask):
        """camera mask of one eye (uint8, image size, 0 = masked out); None removes it"""
        if mask is None:
            _check(self.lib.lpslam_hip_set_mask(self.h, int(eye), None, 0)); return
        m = np.ascontiguousarray(mask, np.uint8)
        assert m.shape == (self.cfg.height, self.cfg.width), m.shape
        _check(self.lib.lpslam_hip_set_mask(self.h, int(eye), _p(m), m.shape[1]))

    def upload_raw(self, image, eye, arr):
        arr = np.ascontiguousarray(arr, np.uint8)
        assert arr.shape == (self.cfg.height, self.cfg.width), arr.shape
        _check(self.lib.lpslam_hip_upload_raw_image(self.h, image, int(eye), _p(arr), arr.shape[1]))
        self.sync()

    def match_projection(self, image, queries, q_desc, hamming_thr=100, lowe_ratio=0.8, taken=None, use_stereo=False):
        q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE); d = np.ascontiguousarray(q_desc, np.uint8)
        assert d.shape == (len(q), 32)
        t = np.ascontiguousarray(taken, np.uint8) if taken is not None else None
        idx = np.full(max(len(q), 1), -1, np.int32); dist = np.zeros(max(len(q), 1), np.int32); n = C.c_int32()
        f = self.lib.lpslam_hip_match_projection
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32,
                      C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self.h, image, _p(q), _p(d), len(q), int(hamming_thr), float(lowe_ratio), _p(t), int(use_stereo), _p(idx), _p(dist), C.byref(n)))
        return idx[:len(q)].copy(), dist[:len(q)].copy(), n.value

    def match_fuse(self, image, queries, q_desc, hamming_thr=50, use_stereo=False):
        q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE); d = np.ascontiguousarray(q_desc, np.uint8)
        idx = np.full(max(len(q), 1), -1, np.int32); dist = np.zeros(max(len(q), 1), np.int32); n = C.c_int32()
        f = self.lib.lpslam_hip_match_fuse
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self.h, image, _p(q), _p(d), len(q), int(hamming_thr), int(use_stereo), _p(idx), _p(dist), C.byref(n)))
        return idx[:len(q)].copy(), dist[:len(q)].copy(), n.value

    def match_area(self, image, queries, q_desc, hamming_thr=50, lowe_ratio=0.9):
        q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE); d = np.ascontiguousarray(q_desc, np.uint8)
        idx = np.full(max(len(q), 1), -1, np.int32); dist = np.zeros(max(len(q), 1), np.int32); n = C.c_int32()
        f = self.lib.lpslam_hip_match_area
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self.h, image, _p(q), _p(d), len(q), int(hamming_thr), float(lowe_ratio), _p(idx), _p(dist), C.byref(n)))
        return idx[:len(q)].copy(), dist[:len(q)].copy(), n.value

    def window_match_rescans(self):
        """single-query rescans the last match_projection / match_fuse / match_area call made"""
        f = self.lib.lpslam_hip_window_match_rescans
        f.restype = C.c_int32; f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def remap_staged(self, image, eye):
        _check(self.lib.lpslam_hip_remap_staged(self.h, image, int(eye)))

    def prefetch(self):
        """context manager: upload / remap / extract / stereo calls of THIS thread go to the context's prefetch stream"""
        ctx = self
        class _Section:
            def __enter__(self_inner):
                _check(ctx.lib.lpslam_hip_prefetch_begin(ctx.h))
            def __exit__(self_inner, *exc):
                _check(ctx.lib.lpslam_hip_prefetch_end(ctx.h))
                return False
        return _Section()

    def prefetch_join(self):
        _check(self.lib.lpslam_hip_prefetch_join(self.h))

    def prefetch_frame(self, image, with_stereo=True):
        """queues the read-back of `image` behind what this thread has enqueued for it: frame(image) then finds the results delivered"""
        _check(self.lib.lpslam_hip_prefetch_frame(self.h, image, 1 if with_stereo else 0))

    def extract(self, n_images):
        _check(self.lib.lpslam_hip_extract(self.h, n_images))

    def extract_range(self, first, n_images):
        _check(self.lib.lpslam_hip_extract_range(self.h, first, n_images))

    def stage(self, name, n_images):
        _check(getattr(self.lib, "lpslam_hip_stage_" + name)(self.h, n_images))

    def set_keypoint_camera(self, model):
        """fisheye model of every slot (a Fisheye, or None to clear it): extraction then ends with the undistort stage"""
        f = self.lib.lpslam_hip_set_keypoint_camera
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(Fisheye)]
        _check(f(self.h, None if model is None else C.byref(model)))

    def set_keypoint_camera_radtan(self, model):
        """radial-tangential model of every slot (a Radtan; None or all-zero coefficients clear it); replaces a fisheye model"""
        f = self.lib.lpslam_hip_set_keypoint_camera_radtan
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(Radtan)]
        _check(f(self.h, None if model is None else C.byref(model)))

    def undistort_points_radtan(self, model, xy):
        """undistort_points for a Radtan model"""
        f = self.lib.lpslam_hip_undistort_points_radtan
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(Radtan), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.full(xy.shape, np.nan, np.float32); valid = np.zeros(len(xy), np.uint8)
        _check(f(self.h, C.byref(model), _p(xy), len(xy), _p(out), _p(valid)))
        return out, valid.astype(bool)

    def stage_undistort(self, n_images):
        f = self.lib.lpslam_hip_stage_undistort
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int]
        _check(f(self.h, int(n_images)))

    def undistort_dropped(self, image):
        """keypoints the undistort stage's last run removed from the slot"""
        f = self.lib.lpslam_hip_undistort_dropped
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
        n = C.c_int32()
        _check(f(self.h, int(image), C.byref(n)))
        return n.value

    def undistort_points(self, model, xy):
        """the stage's arithmetic on an (n, 2) float32 array of pixels: (undistorted (n, 2) float32, valid (n,) bool)"""
        f = self.lib.lpslam_hip_undistort_points
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(Fisheye), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.full(xy.shape, np.nan, np.float32); valid = np.zeros(len(xy), np.uint8)
        _check(f(self.h, C.byref(model), _p(xy), len(xy), _p(out), _p(valid)))
        return out, valid.astype(bool)

    def triangulate_neighbours(self, image, group1, pose1, cam, sets, scale=None, capacity=None):
        """lpslam_hip_triangulate_neighbours: the keypoints of slot `image` (view pose1, 7 doubles) against `sets`, a list of dicts with
        kpts (KP_DTYPE), desc (n, 32), group (int32), optional x_right / depth (float32), pose (7), F (3, 3), epipole ((x, y) or None).
        Returns a dict of arrays per (set, query): j, dist, code (n_sets, nq, 8), X (n_sets, nq, 8, 3), count (n_sets, nq)."""
        f = self.lib.lpslam_hip_triangulate_neighbours
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TriCamera), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                      C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        scale = np.ascontiguousarray(self.scale if scale is None else scale, np.float32)
        cap = self.max_kp if capacity is None else int(capacity)
        ns = len(sets)
        keep, arr = [], (TriSet * max(ns, 1))()
        for k, s in enumerate(sets):
            kp = np.ascontiguousarray(s["kpts"], KP_DTYPE); desc = np.ascontiguousarray(s["desc"], np.uint8); grp = np.ascontiguousarray(s["group"], np.int32)
            xr = None if s.get("x_right") is None else np.ascontiguousarray(s["x_right"], np.float32)
            dep = None if s.get("depth") is None else np.ascontiguousarray(s["depth"], np.float32)
            keep += [kp, desc, grp, xr, dep]
            t = arr[k]
            t.kpts, t.desc32, t.group = kp.ctypes.data, desc.ctypes.data, grp.ctypes.data
            t.x_right = None if xr is None else xr.ctypes.data; t.depth = None if dep is None else dep.ctypes.data
            t.n = int(s.get("n", len(kp)))
            t.pose = (C.c_double * 7)(*[float(v) for v in s["pose"]]); t.F = (C.c_double * 9)(*[float(v) for v in np.asarray(s["F"], np.float64).reshape(9)])
            ep = s.get("epipole")
            t.has_epipole = 0 if ep is None else 1
            t.epipole = (C.c_double * 2)(*([0.0, 0.0] if ep is None else [float(ep[0]), float(ep[1])]))
        group1 = None if group1 is None else np.ascontiguousarray(group1, np.int32)
        pose1 = np.ascontiguousarray(pose1, np.float64)
        j = np.full((ns, cap, 8), -1, np.int32); dist = np.full((ns, cap, 8), 256, np.int32); code = np.zeros((ns, cap, 8), np.int32)
        X = np.full((ns, cap, 8, 3), np.nan, np.float64); count = np.zeros((ns, cap), np.int32)
        nq = C.c_int32(0)
        _check(f(self.h, int(image), _p(group1), _p(pose1), C.byref(cam), arr if ns else None, ns, _p(scale), len(scale), cap,
                 C.byref(nq), _p(j), _p(dist), _p(code), _p(X), _p(count)))
        n = nq.value
        return {"j": j[:, :n], "dist": dist[:, :n], "code": code[:, :n], "X": X[:, :n], "count": count[:, :n]}

    def triangulate_pairs(self, cam, pose1, pose2, kp1, kp2, scale=None):
        """tri_pair on caller pairs (TRI_KP_DTYPE arrays): (code (n,) int32, X (n, 3) float64, NaN where the code is 0)"""
        f = self.lib.lpslam_hip_triangulate_pairs
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(TriCamera), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        scale = np.ascontiguousarray(self.scale if scale is None else scale, np.float32)
        kp1 = np.ascontiguousarray(kp1, TRI_KP_DTYPE); kp2 = np.ascontiguousarray(kp2, TRI_KP_DTYPE)
        assert len(kp1) == len(kp2)
        pose1 = np.ascontiguousarray(pose1, np.float64); pose2 = np.ascontiguousarray(pose2, np.float64)
        code = np.zeros(len(kp1), np.int32); X = np.full((len(kp1), 3), np.nan, np.float64)
        _check(f(self.h, C.byref(cam), _p(scale), len(scale), _p(pose1), _p(pose2), _p(kp1), _p(kp2), len(kp1), _p(code), _p(X)))
        return code, X

    def keypoints(self, image):
        kp = np.zeros(self.max_kp, KP_DTYPE); desc = np.zeros((self.max_kp, 32), np.uint8)
        n = C.c_int32()
        _check(self.lib.lpslam_hip_get_keypoints(self.h, image, _p(kp), _p(desc), self.max_kp, C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy()

    def frame(self, image):
        """keypoints, descriptors, x_right, depth of one slot in one round trip (lpslam_hip_get_frame)"""
        kp = np.zeros(self.max_kp, KP_DTYPE); desc = np.zeros((self.max_kp, 32), np.uint8)
        xr = np.zeros(self.max_kp, np.float32); dep = np.zeros(self.max_kp, np.float32)
        n = C.c_int32()
        _check(self.lib.lpslam_hip_get_frame(self.h, image, _p(kp), _p(desc), _p(xr), _p(dep), self.max_kp, C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy(), xr[:n.value].copy(), dep[:n.value].copy()

    def frame_view(self, image, with_stereo=True):
        """lpslam_hip_get_frame_view: copies made from the context's page-locked block (valid until the next frame call)"""
        kp = C.c_void_p(); desc = C.c_void_p(); xr = C.c_void_p(); dep = C.c_void_p(); n = C.c_int32()
        f = self.lib.lpslam_hip_get_frame_view
        f.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self.h, image, 1 if with_stereo else 0, C.byref(kp), C.byref(desc), C.byref(xr), C.byref(dep), C.byref(n)))
        m = n.value
        def arr(ptr, dtype, count):
            return np.frombuffer(C.string_at(ptr.value, count * np.dtype(dtype).itemsize), dtype).copy() if (ptr.value and count) else np.zeros(0, dtype)
        return arr(kp, KP_DTYPE, m), arr(desc, np.uint8, 32 * m).reshape(-1, 32), arr(xr, np.float32, m if with_stereo else 0), arr(dep, np.float32, m if with_stereo else 0)

    def pyramid_level(self, image, level):
        out = np.zeros((self.level_h[level], self.level_w[level]), np.uint8)
        _check(self.lib.lpslam_hip_get_pyramid_level(self.h, image, level, _p(out), out.shape[1]))
        return out

    def candidates(self, image, level):
        n = C.c_int32()
        _check(self.lib.lpslam_hip_get_candidates(self.h, image, level, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), CORNER_DTYPE)
        _check(self.lib.lpslam_hip_get_candidates(self.h, image, level, _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def set_descriptors(self, image, desc):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        _check(self.lib.lpslam_hip_set_descriptors(self.h, image, _p(desc), len(desc)))

    def match_bf(self, query, train):
        _check(self.lib.lpslam_hip_match_bf(self.h, query, train))

    def match_bf_strided(self, q0, t0, stride, n):
        _check(self.lib.lpslam_hip_match_bf_strided(self.h, q0, t0, stride, n))

    def bf_knn2(self, query):
        bi = np.zeros(self.max_kp, np.int32); bd = np.zeros(self.max_kp, np.int32); sd = np.zeros(self.max_kp, np.int32)
        n = C.c_int32()
        _check(self.lib.lpslam_hip_get_bf_knn2(self.h, query, _p(bi), _p(bd), _p(sd), self.max_kp, C.byref(n)))
        return bi[:n.value].copy(), bd[:n.value].copy(), sd[:n.value].copy()

    def bf_matches(self, query, train, max_dist=50, ratio=0.0, cross_check=False):
        oq = np.zeros(self.max_kp, np.int32); ot = np.zeros(self.max_kp, np.int32); od = np.zeros(self.max_kp, np.int32)
        n = C.c_int32()
        _check(self.lib.lpslam_hip_get_bf_matches(self.h, query, train, int(max_dist), float(ratio), int(cross_check),
                                                  _p(oq), _p(ot), _p(od), self.max_kp, C.addressof(n)))
        return oq[:n.value].copy(), ot[:n.value].copy(), od[:n.value].copy()

    def match_bf_descriptors(self, query, scratch, desc, max_dist=50, ratio=0.0, cross_check=False):
        """set_descriptors(scratch, desc) + match_bf(query, scratch) + bf_matches(query, scratch, ...) as one call with one wait"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        oq = np.zeros(self.max_kp, np.int32); ot = np.zeros(self.max_kp, np.int32); od = np.zeros(self.max_kp, np.int32)
        n = C.c_int32()
        _check(self.lib.lpslam_hip_match_bf_descriptors(self.h, query, scratch, _p(desc), len(desc), int(max_dist), float(ratio), int(cross_check),
                                                        _p(oq), _p(ot), _p(od), self.max_kp, C.addressof(n)))
        return oq[:n.value].copy(), ot[:n.value].copy(), od[:n.value].copy()

    def desc_store_put(self, key, desc):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        f = self.lib.lpslam_hip_desc_store_put; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        _check(f(self.h, int(key), _p(desc), len(desc)))

    def desc_store_drop(self, key):
        f = self.lib.lpslam_hip_desc_store_drop; f.argtypes = [C.c_void_p, C.c_int32]
        _check(f(self.h, int(key)))

    def match_bf_stored(self, query, keys, max_dist=50, ratio=0.0, cross_check=False):
        """the slot `query` against every stored descriptor set in `keys`, one call: [(mq, mt, md)] per key"""
        keys = np.ascontiguousarray(keys, np.int32); n = len(keys); cap = self.max_kp
        oq = np.zeros((max(n, 1), cap), np.int32); ot = np.zeros_like(oq); od = np.zeros_like(oq); cnt = np.zeros(max(n, 1), np.int32)
        f = self.lib.lpslam_hip_match_bf_stored
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        _check(f(self.h, int(query), _p(keys), n, int(max_dist), float(ratio), int(cross_check), _p(oq), _p(ot), _p(od), cap, _p(cnt)))
        return [(oq[k, :cnt[k]].copy(), ot[k, :cnt[k]].copy(), od[k, :cnt[k]].copy()) for k in range(n)]

    def desc_store_mask(self, key, mask):
        """per-descriptor mask of a stored set (nonzero: its matches count in rank_stored)"""
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        f = self.lib.lpslam_hip_desc_store_mask; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        _check(f(self.h, int(key), _p(mask), len(mask)))

    def rank_stored(self, query, keys=None, max_dist=50, ratio=0.75, top_k=8):
        """stored sets ranked by their cross-checked, mask-passing matches with slot `query`: (keys, votes), best first;
        keys=None ranks every stored set"""
        kk = None if keys is None else np.ascontiguousarray(keys, np.int32)
        ok = np.zeros(max(int(top_k), 1), np.int32); ov = np.zeros_like(ok); n = C.c_int32()
        f = self.lib.lpslam_hip_rank_stored
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self.h, int(query), _p(kk), 0 if kk is None else len(kk), int(max_dist), float(ratio), int(top_k), _p(ok), _p(ov), C.byref(n)))
        return ok[:n.value].copy(), ov[:n.value].copy()

    def scan_geometry_put(self, cos_sin):
        """uploads a table of beam directions ((n, 2) float64: cos a, sin a); returns its id"""
        cs = np.ascontiguousarray(cos_sin, np.float64).reshape(-1, 2)
        gid = C.c_int32()
        f = self.lib.lpslam_hip_scan_geometry_put; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        _check(f(self.h, _p(cs), len(cs), C.byref(gid)))
        return gid.value

    def scan_store_put(self, key, geometry_id, ranges, range_min, range_max, range_threshold):
        r = np.ascontiguousarray(ranges, np.float32).reshape(-1)
        f = self.lib.lpslam_hip_scan_store_put
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float]
        _check(f(self.h, int(key), int(geometry_id), _p(r), len(r), float(range_min), float(range_max), float(range_threshold)))

    def scan_store_drop(self, key):
        f = self.lib.lpslam_hip_scan_store_drop; f.argtypes = [C.c_void_p, C.c_int32]
        _check(f(self.h, int(key)))

    def occupancy_build(self, poses, res, max_side, out=None, sizing=False):
        """poses: SCAN_POSE_DTYPE array.  Returns (grid (height, width) int8 or None when sizing, info dict); `out` (flat int8) is
        the caller's buffer, its size the capacity"""
        poses = np.ascontiguousarray(poses, SCAN_POSE_DTYPE)
        info = GridInfo()
        f = self.lib.lpslam_hip_occupancy_build
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        if sizing:
            _check(f(self.h, _p(poses), len(poses), float(res), int(max_side), None, 0, C.byref(info)))
            return None, info.as_dict()
        if out is None:
            _check(f(self.h, _p(poses), len(poses), float(res), int(max_side), None, 0, C.byref(info)))
            out = np.empty(max(info.width * info.height, 1), np.int8)
        _check(f(self.h, _p(poses), len(poses), float(res), int(max_side), _p(out), len(out), C.byref(info)))
        return out[:info.width * info.height].reshape(info.height, info.width), info.as_dict()

    def match_stereo(self, left, right, fxb, baseline):
        _check(self.lib.lpslam_hip_match_stereo(self.h, left, right, float(fxb), float(baseline)))

    def match_stereo_strided(self, l0, r0, stride, n, fxb, baseline):
        _check(self.lib.lpslam_hip_match_stereo_strided(self.h, l0, r0, stride, n, float(fxb), float(baseline)))

    def stereo(self, left):
        xr = np.zeros(self.max_kp, np.float32); dep = np.zeros(self.max_kp, np.float32); bi = np.zeros(self.max_kp, np.int32)
        n = C.c_int32()
        _check(self.lib.lpslam_hip_get_stereo(self.h, left, _p(xr), _p(dep), _p(bi), self.max_kp, C.byref(n)))
        return xr[:n.value].copy(), dep[:n.value].copy(), bi[:n.value].copy()


class BundleAdjuster:
    """Device-resident bundle-adjustment problem (lpslam_hip_ba_*)."""

    def __init__(self, ctx, poses, fixed, points, obs, cam, robust_kernel=True, build=True):
        self.ctx = ctx
        self.lib = ctx.lib
        poses = np.ascontiguousarray(poses, np.float64); points = np.ascontiguousarray(points, np.float64)
        fixed = np.ascontiguousarray(fixed, np.uint8); obs = np.ascontiguousarray(obs, BA_OBS_DTYPE)
        self.n_poses, self.n_points, self.n_obs = len(poses), len(points), len(obs)
        c = BaCamera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["fxb"],
                     float(np.sqrt(5.991)) if robust_kernel else 0.0, float(np.sqrt(7.815)) if robust_kernel else 0.0)
        h = C.c_void_p()
        # build=False: the host half alone (lpslam_hip_ba_prepare: no kernel, thread safe); ba_build_batch enqueues the device half of many
        _check((self.lib.lpslam_hip_ba_create if build else self.lib.lpslam_hip_ba_prepare)(ctx.h, _p(poses), _p(fixed), self.n_poses, _p(points), self.n_points,
                                                                                           _p(obs), self.n_obs, C.byref(c), C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lpslam_hip_ba_destroy(self.h)
            self.h = None

    __del__ = close

    def solver(self):
        """('band' | 'dense', block half-bandwidth found at creation or -1)"""
        sv, hb = C.c_int32(), C.c_int32()
        _check(self.lib.lpslam_hip_ba_get_solver(self.h, C.byref(sv), C.byref(hb)))
        return ("band" if sv.value == 2 else "dense"), hb.value

    def schur_part(self):
        """(part, capacity): terms per part of the dense path's pair lists, chosen by the build, and the further parts there was room for"""
        p, c = C.c_int32(0), C.c_int32(0)
        _check(self.lib.lpslam_hip_ba_get_schur_part(self.h, C.byref(p), C.byref(c)))
        return p.value, c.value

    def timeouts(self):
        """(band, update): hand-overs between workgroups that timed out on this problem so far -- expected (0, 0)"""
        a, b = C.c_int32(0), C.c_int32(0)
        _check(self.lib.lpslam_hip_ba_timeouts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_solver(self, name):
        _check(self.lib.lpslam_hip_ba_set_solver(self.h, {"auto": 0, "dense": 1, "band": 2}[name]))

    def set_active(self, active=None):
        a = np.ascontiguousarray(active, np.uint8) if active is not None else None
        _check(self.lib.lpslam_hip_ba_set_active(self.h, _p(a)))

    def optimize(self, robust=True, iters=10):
        log = np.zeros(max(iters, 1), BA_LOG_DTYPE); done = C.c_int32()
        _check(self.lib.lpslam_hip_ba_optimize(self.h, int(robust), int(iters), _p(log), C.byref(done)))
        return log[:done.value].copy()

    def optimize_begin(self, robust=True, iters=10):
        self._iters = int(iters)
        _check(self.lib.lpslam_hip_ba_optimize_begin(self.h, int(robust), int(iters)))

    def optimize_end(self):
        log = np.zeros(max(self._iters, 1), BA_LOG_DTYPE); done = C.c_int32()
        _check(self.lib.lpslam_hip_ba_optimize_end(self.h, _p(log), C.byref(done)))
        return log[:done.value].copy()

    def reset(self):
        _check(self.lib.lpslam_hip_ba_reset(self.h))

    def set_state(self, poses=None, points=None):
        """new creation-time poses / landmarks for the same observation graph (None keeps them); resets the LM state"""
        ps = None if poses is None else np.ascontiguousarray(poses, np.float64)
        pt = None if points is None else np.ascontiguousarray(points, np.float64)
        assert ps is None or ps.shape == (self.n_poses, 7)
        assert pt is None or pt.shape == (self.n_points, 3)
        _check(self.lib.lpslam_hip_ba_set_state(self.h, _p(ps) if ps is not None else None, _p(pt) if pt is not None else None))

    def optimize_profiled(self, robust=True, iters=10):
        """per-kernel HIP-event times of one optimize() call: {kernel: (ms summed, marks, launches per mark)}, iterations"""
        t = BaKernelTimes()
        _check(self.lib.lpslam_hip_ba_optimize_profiled(self.h, int(robust), int(iters), C.byref(t)))
        band = self.solver()[0] == "band"
        one_pass = t.launches[5] == 0 and t.launches[6] > 0      # back substitution + trial + linearisation in one launch (ba_update.inl)
        names = ["k_ba_lin", "k_ba_point_sum", "k_schur_group" if band else "k_ba_schur", "chol", "k_chol_xsolve", "k_ba_backsub", "k_ba_update" if one_pass else "k_ba_trial", "k_schur_band_reduce"]
        return {n: (t.ms[i], t.launches[i], t.launches_per_mark[i]) for i, n in enumerate(names) if t.launches[i] or n == "chol"}, t.iterations, t.dim

    def pose_optimize(self):
        out = np.zeros(max(self.n_obs, 1), np.uint8); n = C.c_int32()
        _check(self.lib.lpslam_hip_ba_pose_optimize(self.h, _p(out), C.byref(n)))
        return out[:self.n_obs], n.value

    def local(self, first=5, second=10):
        out = np.zeros(max(self.n_obs, 1), np.uint8)
        _check(self.lib.lpslam_hip_ba_local(self.h, int(first), int(second), _p(out)))
        return out[:self.n_obs]

    def state(self):
        poses = np.zeros((self.n_poses, 7)); points = np.zeros((self.n_points, 3))
        _check(self.lib.lpslam_hip_ba_get(self.h, _p(poses), _p(points)))
        return poses, points

    def chi2(self):
        chi = np.zeros(max(self.n_obs, 1)); pos = np.zeros(max(self.n_obs, 1), np.uint8)
        _check(self.lib.lpslam_hip_ba_chi2(self.h, _p(chi), _p(pos)))
        return chi[:self.n_obs], pos[:self.n_obs]


    def optimize_partitioned(self, comm, robust=True, iters=10):
        """lpslam_hip_ba_optimize_partitioned: `comm` is an RcclComm (or a raw ncclComm_t value)"""
        log = np.zeros(max(iters, 1), BA_LOG_DTYPE); done = C.c_int32()
        f = self.lib.lpslam_hip_ba_optimize_partitioned
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        _check(f(self.h, getattr(comm, "comm", comm), int(robust), int(iters), _p(log), C.addressof(done)))
        return log[:done.value].copy()

    # ---- partitioned (multi-GPU) solve: phases of one LM trial (see include/lpslam_hip.h) ----
    def reduced_buffer(self):
        ptr = C.c_void_p(); n = C.c_int64()
        _check(self.lib.lpslam_hip_ba_reduced_buffer(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def scalar_buffer(self):
        ptr = C.c_void_p(); n = C.c_int64()
        _check(self.lib.lpslam_hip_ba_scalar_buffer(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def step_begin(self, robust, first):
        _check(self.lib.lpslam_hip_ba_step_begin(self.h, int(robust), int(first)))

    def step_lambda0(self):
        _check(self.lib.lpslam_hip_ba_step_lambda0(self.h))

    def step_solve(self):
        _check(self.lib.lpslam_hip_ba_step_solve(self.h))

    def step_end(self):
        a = C.c_int32(); f = C.c_int32()
        _check(self.lib.lpslam_hip_ba_step_end(self.h, C.byref(a), C.byref(f)))
        return bool(a.value), bool(f.value)

    def status(self):
        o = C.c_int32(); st = C.c_int32(); lam = C.c_double(); chi = C.c_double()
        _check(self.lib.lpslam_hip_ba_status(self.h, C.byref(o), C.byref(st), C.byref(lam), C.byref(chi)))
        return dict(outer_done=o.value, stopped=bool(st.value), lam=lam.value, chi2=chi.value)


class Vocabulary:
    """lpslam_hip_vocab: a DBoW2 vocabulary tree in HBM.  nodes: structured array (parent, desc[32], weight, is_leaf) in file order."""

    def __init__(self, ctx, k, L, parent, desc, weight, is_leaf):
        self.ctx, self.lib = ctx, ctx.lib
        parent = np.ascontiguousarray(parent, np.int32); desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        assert desc.shape == (len(parent), 32)
        h = C.c_void_p()
        f = self.lib.lpslam_hip_vocab_create
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        _check(f(ctx.h, int(k), int(L), len(parent), _p(parent), _p(desc), _p(weight), _p(is_leaf), C.byref(h)))
        self.h = h
        ctx._children.add(self)
        k_, L_, nn, nw = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.lib.lpslam_hip_vocab_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
        _check(self.lib.lpslam_hip_vocab_info(self.h, C.byref(k_), C.byref(L_), C.byref(nn), C.byref(nw)))
        self.k, self.L, self.n_nodes, self.n_words = k_.value, L_.value, nn.value, nw.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.lpslam_hip_vocab_destroy.argtypes = [C.c_void_p]
            self.lib.lpslam_hip_vocab_destroy(self.h)
            self.h = None

    __del__ = close

    def transform(self, image, levels_up=4):
        """word id, word weight, node id per keypoint of an image slot"""
        cap = self.ctx.max_kp
        w = np.zeros(cap, np.int32); wt = np.zeros(cap, np.float32); nd = np.zeros(cap, np.int32); n = C.c_int32()
        f = self.lib.lpslam_hip_bow_transform
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        _check(f(self.ctx.h, self.h, int(image), int(levels_up), _p(w), _p(wt), _p(nd), cap, C.byref(n)))
        return w[:n.value].copy(), wt[:n.value].copy(), nd[:n.value].copy()

    def transform_host(self, desc, levels_up=4):
        d = np.ascontiguousarray(desc, np.uint8)
        n = len(d)
        w = np.zeros(max(n, 1), np.int32); wt = np.zeros(max(n, 1), np.float32); nd = np.zeros(max(n, 1), np.int32)
        f = self.lib.lpslam_hip_bow_transform_host
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self.ctx.h, self.h, _p(d), n, int(levels_up), _p(w), _p(wt), _p(nd)))
        return w[:n], wt[:n], nd[:n]


def match_bow_tree(ctx, q_desc, q_node, t_desc, t_node, hamming_thr=50, lowe_ratio=0.75, t_taken=None):
    qd = np.ascontiguousarray(q_desc, np.uint8); qn = np.ascontiguousarray(q_node, np.int32)
    td = np.ascontiguousarray(t_desc, np.uint8); tn = np.ascontiguousarray(t_node, np.int32)
    tk = np.ascontiguousarray(t_taken, np.uint8) if t_taken is not None else None
    idx = np.full(max(len(qn), 1), -1, np.int32); dist = np.zeros(max(len(qn), 1), np.int32); n = C.c_int32()
    f = ctx.lib.lpslam_hip_match_bow_tree
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    _check(f(ctx.h, _p(qd), _p(qn), len(qn), _p(td), _p(tn), len(tn), _p(tk), int(hamming_thr), float(lowe_ratio), _p(idx), _p(dist), C.byref(n)))
    return idx[:len(qn)], dist[:len(qn)], n.value


def match_bow_tree_multi(ctx, q_desc, q_node, t_descs, t_nodes, hamming_thr=50, lowe_ratio=0.75, t_takens=None):
    """one query set against several target sets in one round trip (lpslam_hip_match_bow_tree_multi); a list of (idx, dist, n) per set"""
    qd = np.ascontiguousarray(q_desc, np.uint8); qn = np.ascontiguousarray(q_node, np.int32)
    ns = len(t_descs)
    tds = [np.ascontiguousarray(t, np.uint8) for t in t_descs]; tns = [np.ascontiguousarray(t, np.int32) for t in t_nodes]
    tks = [np.ascontiguousarray(t, np.uint8) if t is not None else None for t in (t_takens or [None] * ns)]
    idx = [np.full(max(len(qn), 1), -1, np.int32) for _ in range(ns)]; dist = [np.zeros(max(len(qn), 1), np.int32) for _ in range(ns)]
    arr = lambda xs: (C.c_void_p * max(ns, 1))(*[x.ctypes.data if x is not None and x.size else None for x in xs])
    nts = (C.c_int32 * max(ns, 1))(*[len(t) for t in tns]); nm = (C.c_int32 * max(ns, 1))()
    f = ctx.lib.lpslam_hip_match_bow_tree_multi
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(ctx.h, _p(qd), _p(qn), len(qn), ns, arr(tds), arr(tns), nts, arr(tks) if t_takens is not None else None, int(hamming_thr), float(lowe_ratio), arr(idx), arr(dist), nm))
    return [(idx[i][:len(qn)], dist[i][:len(qn)], int(nm[i])) for i in range(ns)]

PNP_MAX_ITERATIONS = 1024          # LPSLAM_HIP_PNP_MAX_ITERATIONS
_PNP_ARGS = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def _pnp_arrays(offsets, pw, obs, inv_sigma2, cam4):
    off = np.ascontiguousarray(offsets, np.int32)
    n_sets = len(off) - 1
    total = int(off[-1]) if n_sets >= 0 else 0
    out = (np.zeros((max(n_sets, 1), 7)), np.zeros(max(n_sets, 1), np.int32), np.zeros(max(total, 1), np.uint8), np.full(max(n_sets, 1), -1, np.int32))
    return off, n_sets, total, np.ascontiguousarray(pw, np.float64), np.ascontiguousarray(obs, np.float64), np.ascontiguousarray(inv_sigma2, np.float64), np.ascontiguousarray(cam4, np.float64), out


def pnp_ransac_batch(ctx, offsets, pw, obs, inv_sigma2, cam4, iterations=100, seed=0x9E3779B9, want_iteration=True):
    """lpslam_hip_pnp_ransac_batch: the sets are matches offsets[s] .. offsets[s + 1] of pw (n, 3), obs (n, 2), inv_sigma2 (n);
    returns pose7 (S, 7), n_inliers (S), the per-match flags (n) and the winning iteration per set (-1: none; None when not asked for)"""
    off, n_sets, total, pw, obs, w, cam, (pose, cnt, fl, best) = _pnp_arrays(offsets, pw, obs, inv_sigma2, cam4)
    f = ctx.lib.lpslam_hip_pnp_ransac_batch
    f.argtypes = [C.c_void_p] + _PNP_ARGS
    _check(f(ctx.h, n_sets, _p(off), _p(pw), _p(obs), _p(w), _p(cam), int(iterations), int(seed) & 0xffffffff, _p(pose), _p(cnt), _p(fl), _p(best) if want_iteration else None))
    return pose[:n_sets], cnt[:n_sets], fl[:total], (best[:n_sets] if want_iteration else None)


_host_lib = None


def host_lib():
    """the host library (lpslam_amd/liblpslam.so): the CPU definitions behind the shims below, no device needed"""
    global _host_lib
    if _host_lib is None:
        _host_lib = C.CDLL(os.path.join(_HERE, "liblpslam.so"))
    return _host_lib


def pnp_ransac_batch_host(offsets, pw, obs, inv_sigma2, cam4, iterations=100, seed=0x9E3779B9, want_iteration=True):
    """lpslam_pnp_ransac_batch_host: LpSlam::pnp_solve_ransac on each set, the CPU definition of pnp_ransac_batch (same results)"""
    off, n_sets, total, pw, obs, w, cam, (pose, cnt, fl, best) = _pnp_arrays(offsets, pw, obs, inv_sigma2, cam4)
    f = host_lib().lpslam_pnp_ransac_batch_host
    f.argtypes = _PNP_ARGS; f.restype = C.c_int
    if f(n_sets, _p(off), _p(pw), _p(obs), _p(w), _p(cam), int(iterations), int(seed) & 0xffffffff, _p(pose), _p(cnt), _p(fl), _p(best) if want_iteration else None):
        raise LpslamHipError("lpslam_pnp_ransac_batch_host refused its arguments")
    return pose[:n_sets], cnt[:n_sets], fl[:total], (best[:n_sets] if want_iteration else None)


def pnp_sample_table(n, iterations, seed):
    """lpslam_pnp_sample_table: the (iterations, 4) match indices pnp_solve_ransac draws for a set of n >= 4 matches"""
    f = host_lib().lpslam_pnp_sample_table
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p]; f.restype = C.c_int
    table = np.full((max(int(iterations), 1), 4), -1, np.int32)
    if not f(int(n), int(iterations), int(seed) & 0xffffffff, _p(table)):
        raise LpslamHipError("lpslam_pnp_sample_table: n < 4 or iterations < 1")
    return table


def epnp4_host(p4, u4, cam4):
    """lpslam_epnp4_host: the host form of epnp4 (csrc/epnp_math.h) on four matches; (R (3, 3), t (3)) or None"""
    f = host_lib().lpslam_epnp4_host
    f.argtypes = [C.c_void_p] * 5; f.restype = C.c_int
    p4 = np.ascontiguousarray(p4, np.float64); u4 = np.ascontiguousarray(u4, np.float64); cam = np.ascontiguousarray(cam4, np.float64)
    assert p4.size == 12 and u4.size == 8 and cam.size == 4
    R = np.zeros(9); t = np.zeros(3)
    return (R.reshape(3, 3), t) if f(_p(p4), _p(u4), _p(cam), _p(R), _p(t)) else None


TWO_VIEW_MAX_ITERATIONS = 1024     # LPSLAM_HIP_TWO_VIEW_MAX_ITERATIONS
TWO_VIEW_MAX_POSES = 8             # LPSLAM_HIP_TWO_VIEW_MAX_POSES
_TV_RANSAC_ARGS = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_TV_POSES_ARGS = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]


def _tv_ransac_arrays(offsets, p1, p2):
    off = np.ascontiguousarray(offsets, np.int32)
    n_sets = len(off) - 1
    total = int(off[-1]) if n_sets >= 0 else 0
    out = (np.full((max(n_sets, 1), 2), -1, np.int32), np.zeros((max(n_sets, 1), 2)), np.zeros((max(n_sets, 1), 2, 3, 3)),
           np.zeros(max(total, 1), np.uint8), np.zeros(max(total, 1), np.uint8))
    return off, n_sets, total, np.ascontiguousarray(p1, np.float64), np.ascontiguousarray(p2, np.float64), out


def _tv_ransac_result(n_sets, total, out):
    best, score, model, fh, ff = out
    return best[:n_sets], score[:n_sets], model[:n_sets], fh[:total], ff[:total]


def two_view_ransac_batch(ctx, offsets, p1, p2, sigma=1.0, iterations=100, seed=0x9E3779B9):
    """lpslam_hip_two_view_ransac_batch: the sets are matches offsets[s] .. offsets[s + 1] of p1, p2 (n, 2) pixels; returns per set and
    model (0 = H, 1 = F) the winning iteration (S, 2; -1: none), its score (S, 2), the matrix (S, 2, 3, 3) and the inlier flags of
    the H and of the F winner (n each)"""
    off, n_sets, total, p1, p2, out = _tv_ransac_arrays(offsets, p1, p2)
    f = ctx.lib.lpslam_hip_two_view_ransac_batch
    f.argtypes = [C.c_void_p] + _TV_RANSAC_ARGS
    _check(f(ctx.h, n_sets, _p(off), _p(p1), _p(p2), float(sigma), int(iterations), int(seed) & 0xffffffff, *[_p(a) for a in out]))
    return _tv_ransac_result(n_sets, total, out)


def two_view_ransac_batch_host(offsets, p1, p2, sigma=1.0, iterations=100, seed=0x9E3779B9):
    """lpslam_two_view_ransac_batch_host: step 1 of LpSlam::two_view_initialize on each set, the CPU definition of two_view_ransac_batch"""
    off, n_sets, total, p1, p2, out = _tv_ransac_arrays(offsets, p1, p2)
    f = host_lib().lpslam_two_view_ransac_batch_host
    f.argtypes = _TV_RANSAC_ARGS; f.restype = C.c_int
    if f(n_sets, _p(off), _p(p1), _p(p2), float(sigma), int(iterations), int(seed) & 0xffffffff, *[_p(a) for a in out]):
        raise LpslamHipError("lpslam_two_view_ransac_batch_host refused its arguments")
    return _tv_ransac_result(n_sets, total, out)


def _tv_poses_arrays(R, t, K4, p1, p2, inlier):
    R = np.ascontiguousarray(R, np.float64).reshape(-1, 9); t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2); p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
    fl = np.ascontiguousarray(inlier, np.uint8)
    P, n = len(R), len(p1)
    assert len(t) == P and len(p2) == n and len(fl) == n
    out = (np.zeros((P, n, 3)), np.zeros((P, n)), np.zeros((P, n), np.uint8))      # (nothing is written when P or n is 0)
    return P, n, R, t, np.ascontiguousarray(K4, np.float64), p1, p2, fl, out


def two_view_check_poses(ctx, R, t, K4, p1, p2, inlier, th2):
    """lpslam_hip_two_view_check_poses: P motion hypotheses (R (P, 3, 3), t (P, 3)) over n matches; X (P, n, 3), cosp (P, n), code (P, n)"""
    P, n, R, t, K, p1, p2, fl, (X, cosp, code) = _tv_poses_arrays(R, t, K4, p1, p2, inlier)
    f = ctx.lib.lpslam_hip_two_view_check_poses
    f.argtypes = [C.c_void_p] + _TV_POSES_ARGS
    _check(f(ctx.h, P, _p(R), _p(t), _p(K), n, _p(p1), _p(p2), _p(fl), float(th2), _p(X), _p(cosp), _p(code)))
    return X[:P, :n], cosp[:P, :n], code[:P, :n]


def two_view_check_poses_host(R, t, K4, p1, p2, inlier, th2):
    """lpslam_two_view_check_poses_host: the per-match part of two_view_initialize's pose check, the CPU definition of two_view_check_poses"""
    P, n, R, t, K, p1, p2, fl, (X, cosp, code) = _tv_poses_arrays(R, t, K4, p1, p2, inlier)
    f = host_lib().lpslam_two_view_check_poses_host
    f.argtypes = _TV_POSES_ARGS; f.restype = C.c_int
    if f(P, _p(R), _p(t), _p(K), n, _p(p1), _p(p2), _p(fl), float(th2), _p(X), _p(cosp), _p(code)):
        raise LpslamHipError("lpslam_two_view_check_poses_host refused its arguments")
    return X[:P, :n], cosp[:P, :n], code[:P, :n]


def two_view_sample_table(n, iterations, seed):
    """lpslam_two_view_sample_table: the (iterations, 8) match indices two_view_initialize draws for a set of n >= 8 matches"""
    f = host_lib().lpslam_two_view_sample_table
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p]; f.restype = C.c_int
    table = np.full((max(int(iterations), 1), 8), -1, np.int32)
    if not f(int(n), int(iterations), int(seed) & 0xffffffff, _p(table)):
        raise LpslamHipError("lpslam_two_view_sample_table: n < 8 or iterations < 1")
    return table


def two_view_models8_host(x1, x2):
    """lpslam_two_view_models8_host: the header's estimators (csrc/two_view_math.h) at eight matches; (H (3, 3), F (3, 3))"""
    f = host_lib().lpslam_two_view_models8_host
    f.argtypes = [C.c_void_p] * 4; f.restype = None
    x1 = np.ascontiguousarray(x1, np.float64); x2 = np.ascontiguousarray(x2, np.float64)
    assert x1.size == 16 and x2.size == 16
    H = np.zeros(9); F = np.zeros(9)
    f(_p(x1), _p(x2), _p(H), _p(F))
    return H.reshape(3, 3), F.reshape(3, 3)


class RcclComm:
    """An ncclComm_t made through ctypes (tests and bench.py: the product's caller is C++ and links RCCL itself).  `unique_id` is the
    128-byte id of rank 0 (RcclComm.unique_id()), handed to the other ranks by the caller's own means."""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            last = None
            for name in ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"):
                try:
                    cls._lib = C.CDLL(name, mode=C.RTLD_GLOBAL); break
                except OSError as e:
                    last = e
            if cls._lib is None:
                raise LpslamHipError("RCCL not found: %s" % last)
        return cls._lib

    @classmethod
    def unique_id(cls):
        buf = C.create_string_buffer(128)
        rc = cls.lib().ncclGetUniqueId(buf)
        if rc != 0:
            raise LpslamHipError("ncclGetUniqueId failed: %d" % rc)
        return buf.raw

    def __init__(self, unique_id, world, rank):
        class Uid(C.Structure):
            _fields_ = [("internal", C.c_char * 128)]
        uid = Uid(); C.memmove(C.byref(uid), unique_id, 128)
        comm = C.c_void_p()
        f = self.lib().ncclCommInitRank
        f.argtypes = [C.POINTER(C.c_void_p), C.c_int, Uid, C.c_int]
        rc = f(C.byref(comm), int(world), uid, int(rank))
        if rc != 0:
            raise LpslamHipError("ncclCommInitRank failed: %d" % rc)
        self.comm = comm

    def close(self):
        if getattr(self, "comm", None):
            f = self.lib().ncclCommDestroy; f.argtypes = [C.c_void_p]
            f(self.comm); self.comm = None


def ba_factor_kernel_name(dim, band=False):
    """name of the kernel that factors a reduced system of `dim` unknowns (rule of enqueue_solve and lp_enqueue_factor_solve in csrc/ba.hip)"""
    return "k_chol_band" if band else "k_chol_pair"          # k_chol_wg takes over only in batches of 40 dense problems and more


def ba_build_batch(problems):
    """the device half of creation (structure build) for problems made with build=False: one launch chain for all of them"""
    lib = load()
    arr = (C.c_void_p * len(problems))(*[p.h for p in problems])
    _check(lib.lpslam_hip_ba_build_batch(arr, len(problems)))


def ba_set_state_batch(problems, poses, points):
    """lpslam_hip_ba_set_state of every problem in one call (poses[i] / points[i]: arrays or None)"""
    n = len(problems)
    ps = [None if a is None else np.ascontiguousarray(a, np.float64) for a in poses]
    pt = [None if a is None else np.ascontiguousarray(a, np.float64) for a in points]
    hs = (C.c_void_p * n)(*[p.h for p in problems])
    pa = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in ps])
    ta = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in pt])
    f = problems[0].lib.lpslam_hip_ba_set_state_batch
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    _check(f(hs, n, pa, ta))


def ba_state_batch(problems):
    """lpslam_hip_ba_get of every problem in one call: [(poses, points)]"""
    n = len(problems)
    out = [(np.empty((p.n_poses, 7)), np.empty((p.n_points, 3))) for p in problems]
    hs = (C.c_void_p * n)(*[p.h for p in problems])
    pa = (C.c_void_p * n)(*[o[0].ctypes.data for o in out])
    ta = (C.c_void_p * n)(*[o[1].ctypes.data for o in out])
    f = problems[0].lib.lpslam_hip_ba_get_batch
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    _check(f(hs, n, pa, ta))
    return out


def ba_optimize_batch(problems, robust=True, iters=10):
    """lpslam_hip_ba_optimize_batch: the problems (BundleAdjuster objects on one device) advanced by one launch chain.
    Returns one iteration log per problem."""
    n = len(problems)
    lib = problems[0].lib
    hs = (C.c_void_p * n)(*[p.h for p in problems])
    stride = max(int(iters), 1)
    logs = np.zeros((n, stride), BA_LOG_DTYPE); done = np.zeros(n, np.int32)
    _check(lib.lpslam_hip_ba_optimize_batch(hs, n, int(robust), int(iters), _p(logs), stride, _p(done)))
    return [logs[i, :done[i]].copy() for i in range(n)]


def ba_reset_batch(problems):
    n = len(problems)
    hs = (C.c_void_p * n)(*[p.h for p in problems])
    _check(problems[0].lib.lpslam_hip_ba_reset_batch(hs, n))


def ba_debug_solve(problems, As, bs):
    """lpslam_hip_ba_debug_solve (test hook): the factor-and-solve of the caller's systems As[i] x = bs[i] through the launches a solve
    of these problems takes; As[i] is the matrix of 6 x (free keyframes of problems[i]) rows.  A problem with the dense solver takes a
    full symmetric matrix (panel-pair chain or k_chol_wg); a problem on the band solver, ("band", hbw), takes one that is zero below the
    diagonal further than 6 hbw + 5 from it, through k_chol_band, which reads the lower triangle only (the strict upper triangle may
    hold anything, NaN included).  A batch may mix the two.  Returns ([x_i], pivot flags); x_i of a flagged solve is the zero step.
    The problems need a reset() before they optimise again."""
    n = len(problems)
    As = [np.ascontiguousarray(a, np.float64) for a in As]; bs = [np.ascontiguousarray(b, np.float64) for b in bs]
    assert len(As) == n and len(bs) == n
    for p, a, b in zip(problems, As, bs):
        assert a.ndim == 2 and a.shape[0] == a.shape[1] and b.shape == (a.shape[0],)
        read = np.tril(a) if p.solver()[0] == "band" else a
        assert np.isfinite(read).all() and np.isfinite(b).all(), "finite inputs only"
    xs = [np.zeros(len(b)) for b in bs]
    flags = np.zeros(n, np.int32)
    hs = (C.c_void_p * n)(*[p.h for p in problems])
    aa = (C.c_void_p * n)(*[a.ctypes.data for a in As])
    ba = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
    xa = (C.c_void_p * n)(*[x.ctypes.data for x in xs])
    f = problems[0].lib.lpslam_hip_ba_debug_solve
    f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(hs, n, aa, ba, xa, _p(flags)))
    return xs, flags


def ba_obs_array(prob):
    o = np.zeros(len(prob["obs_pose"]), BA_OBS_DTYPE)
    o["pose"] = prob["obs_pose"]; o["point"] = prob["obs_point"]
    o["u"] = prob["obs_uvr"][:, 0]; o["v"] = prob["obs_uvr"][:, 1]; o["ur"] = prob["obs_uvr"][:, 2]
    o["inv_sigma2"] = prob["obs_inv_sigma2"]
    return o


def ba_local_window(ctx, poses, fixed, points, obs, cam, first=5, second=10):
    """a keyframe's local bundle adjustment in one call (lpslam_hip_ba_local_window): returns (poses, points, outlier mask)"""
    po = np.ascontiguousarray(poses, np.float64).copy(); pt = np.ascontiguousarray(points, np.float64).copy()
    fx = np.ascontiguousarray(fixed, np.uint8); o = np.ascontiguousarray(obs, BA_OBS_DTYPE)
    c = BaCamera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["fxb"], float(np.sqrt(5.991)), float(np.sqrt(7.815)))
    out = np.zeros(max(len(o), 1), np.uint8)
    f = ctx.lib.lpslam_hip_ba_local_window
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    _check(f(ctx.h, _p(po), _p(fx), len(po), _p(pt), len(pt), _p(o), len(o), C.byref(c), int(first), int(second), _p(out)))
    return po, pt, out[:len(o)].astype(bool)


def sim3_edges(ei, ej, meas):
    e = np.zeros(len(ei), SIM3_EDGE_DTYPE)
    e["i"] = ei; e["j"] = ej; e["meas"] = meas
    return e


class PoseGraph:
    """Device-resident Sim3 pose graph (lpslam_hip_sim3_*): vertices n x 8 (qw qx qy qz tx ty tz s)."""

    def __init__(self, ctx, verts, fixed, edges, fix_scale=True):
        self.ctx = ctx
        self.lib = ctx.lib
        verts = np.ascontiguousarray(verts, np.float64); fixed = np.ascontiguousarray(fixed, np.uint8)
        edges = np.ascontiguousarray(edges, SIM3_EDGE_DTYPE)
        self.n, self.n_edges = len(verts), len(edges)
        h = C.c_void_p()
        _check(self.lib.lpslam_hip_sim3_create(ctx.h, _p(verts), _p(fixed), self.n, _p(edges), self.n_edges, int(fix_scale), C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lpslam_hip_sim3_destroy(self.h)
            self.h = None

    __del__ = close

    def optimize(self, iters=50):
        log = np.zeros(max(iters, 1), BA_LOG_DTYPE); done = C.c_int32()
        _check(self.lib.lpslam_hip_sim3_optimize(self.h, int(iters), _p(log), C.byref(done)))
        return log[:done.value].copy()

    def get(self):
        v = np.zeros((self.n, 8))
        _check(self.lib.lpslam_hip_sim3_get(self.h, _p(v)))
        return v

    def chi2(self):
        c = np.zeros(self.n_edges)
        _check(self.lib.lpslam_hip_sim3_chi2(self.h, _p(c)))
        return c


def sim3_pairs(prob):
    p = np.zeros(len(prob["p1c"]), SIM3_PAIR_DTYPE)
    for k in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        p[k] = prob[k]
    return p


def sim3_transform_optimize(ctx, s12, pairs_list, cam1, cam2, chi_sq=10.0, fix_scale=True):
    """Batch of loop candidates (lpslam_hip_sim3_transform_optimize): s12 (n x 8), one pair array per candidate.
    Returns (s12 n x 8, list of inlier masks, inlier counts)."""
    s = np.ascontiguousarray(np.atleast_2d(s12), np.float64).copy()
    n = len(pairs_list)
    start = np.zeros(n + 1, np.int32); start[1:] = np.cumsum([len(p) for p in pairs_list])
    pairs = np.ascontiguousarray(np.concatenate(pairs_list) if n else np.zeros(0, SIM3_PAIR_DTYPE), SIM3_PAIR_DTYPE)
    c1 = np.ascontiguousarray(cam1, np.float64); c2 = np.ascontiguousarray(cam2, np.float64)
    inl = np.zeros(max(len(pairs), 1), np.uint8); cnt = np.zeros(max(n, 1), np.int32)
    f = ctx.lib.lpslam_hip_sim3_transform_optimize
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
    _check(f(ctx.h, n, _p(s), _p(pairs), _p(start), _p(c1), _p(c2), float(chi_sq), int(fix_scale), _p(inl), _p(cnt)))
    return s, [inl[start[i]:start[i + 1]].astype(bool) for i in range(n)], cnt[:n].copy()


SIM3_RANSAC_MAX_ITERATIONS = 1024          # LPSLAM_HIP_SIM3_RANSAC_MAX_ITERATIONS


def _sim3_batch_arrays(pairs_list, cam1, cam2, first=0):
    """the pairs of all sets in one array behind `first` unused records, pair_start (from `first`), both cameras"""
    n = len(pairs_list)
    start = np.full(n + 1, int(first), np.int32); start[1:] += np.cumsum([len(p) for p in pairs_list], dtype=np.int64).astype(np.int32)
    pairs = np.ascontiguousarray(np.concatenate([np.zeros(int(first), SIM3_PAIR_DTYPE)] + [np.ascontiguousarray(p, SIM3_PAIR_DTYPE) for p in pairs_list]), SIM3_PAIR_DTYPE)
    return n, start, pairs, np.ascontiguousarray(cam1, np.float64), np.ascontiguousarray(cam2, np.float64)


_SIM3_RANSAC_ARGS = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def _sim3_ransac(f, head, pairs_list, cam1, cam2, fix_scale, iterations, seed, want_iteration, first):
    n, start, pairs, c1, c2 = _sim3_batch_arrays(pairs_list, cam1, cam2, first)
    s12 = np.zeros((max(n, 1), 8)); cnt = np.zeros(max(n, 1), np.int32); inl = np.zeros(max(len(pairs), 1), np.uint8); best = np.full(max(n, 1), -1, np.int32)
    rc = f(*head, n, _p(pairs), _p(start), _p(c1), _p(c2), int(bool(fix_scale)), int(iterations), int(seed) & 0xffffffff, _p(s12), _p(cnt), _p(inl), _p(best) if want_iteration else None)
    return rc, (s12[:n], cnt[:n], [inl[start[i]:start[i + 1]].copy() for i in range(n)], (best[:n] if want_iteration else None))


def sim3_ransac_batch(ctx, pairs_list, cam1, cam2, fix_scale=True, iterations=200, seed=0x9E3779B9, want_iteration=True, first=0):
    """lpslam_hip_sim3_ransac_batch: one SIM3_PAIR_DTYPE array per set (`first`: pair_start[0], that many unused records in front);
    returns s12 (S, 8), n_inliers (S), a list of per-pair flags and the winning iteration per set (-1: none; None when not asked for)"""
    f = ctx.lib.lpslam_hip_sim3_ransac_batch
    f.argtypes = [C.c_void_p] + _SIM3_RANSAC_ARGS
    rc, out = _sim3_ransac(f, (ctx.h,), pairs_list, cam1, cam2, fix_scale, iterations, seed, want_iteration, first)
    _check(rc)
    return out


def sim3_ransac_batch_host(pairs_list, cam1, cam2, fix_scale=True, iterations=200, seed=0x9E3779B9, want_iteration=True, first=0):
    """lpslam_sim3_ransac_batch_host: LpSlam::sim3_solve_ransac on each set, the CPU definition of sim3_ransac_batch (same results)"""
    f = host_lib().lpslam_sim3_ransac_batch_host
    f.argtypes = _SIM3_RANSAC_ARGS; f.restype = C.c_int
    rc, out = _sim3_ransac(f, (), pairs_list, cam1, cam2, fix_scale, iterations, seed, want_iteration, first)
    if rc:
        raise LpslamHipError("lpslam_sim3_ransac_batch_host refused its arguments")
    return out


def sim3_sample_table(n, iterations, seed):
    """lpslam_sim3_sample_table: the (iterations, 3) pair indices sim3_solve_ransac draws for a set of n >= 3 pairs"""
    f = host_lib().lpslam_sim3_sample_table
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p]; f.restype = C.c_int
    table = np.full((max(int(iterations), 1), 3), -1, np.int32)
    if not f(int(n), int(iterations), int(seed) & 0xffffffff, _p(table)):
        raise LpslamHipError("lpslam_sim3_sample_table: n < 3 or iterations < 1")
    return table


def sim3_verify_batch(ctx, pairs_list, cam1, cam2, fix_scale=True, iterations=200, seed=0x9E3779B9, min_seed_inliers=12, chi_sq=10.0, want_inlier=True):
    """lpslam_hip_sim3_verify_batch: RANSAC, gate and transform optimiser for a batch of loop candidates in one call; returns
    seed_inliers (S), s12 (S, 8), n_inliers (S) and a list of the optimiser's per-pair flags (None when not asked for)"""
    n, start, pairs, c1, c2 = _sim3_batch_arrays(pairs_list, cam1, cam2)
    seed_cnt = np.zeros(max(n, 1), np.int32); s12 = np.zeros((max(n, 1), 8)); cnt = np.zeros(max(n, 1), np.int32); inl = np.zeros(max(len(pairs), 1), np.uint8)
    f = ctx.lib.lpslam_hip_sim3_verify_batch
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(ctx.h, n, _p(pairs), _p(start), _p(c1), _p(c2), int(bool(fix_scale)), int(iterations), int(seed) & 0xffffffff, int(min_seed_inliers), float(chi_sq),
             _p(seed_cnt), _p(s12), _p(cnt), _p(inl) if want_inlier else None))
    return seed_cnt[:n], s12[:n], cnt[:n], ([inl[start[i]:start[i + 1]].copy() for i in range(n)] if want_inlier else None)


POSE_COV_MAX_SETS, POSE_COV_MAX_OBS = 4096, 1 << 18          # LPSLAM_HIP_POSE_COV_MAX_SETS, LPSLAM_HIP_POSE_COV_MAX_OBS
_POSE_COV_ARGS = [C.c_int32] + [C.c_void_p] * 11


def _pose_cov(f, head, set_start, pose7, obs, active, cam):
    start = np.ascontiguousarray(set_start, np.int32)
    n = len(start) - 1
    pose = np.ascontiguousarray(pose7, np.float64).reshape(-1); ob = np.ascontiguousarray(obs, np.float64).reshape(-1)
    act = np.ascontiguousarray(active, np.uint8).reshape(-1); cm = np.ascontiguousarray(cam, np.float64).reshape(-1)
    m = max(n, 1)
    assert len(pose) >= 7 * n and len(cm) == 5 and (n < 1 or (len(ob) >= 7 * int(start[-1]) and len(act) >= int(start[-1])))
    info = np.zeros((m, 21)); cov = np.zeros((m, 21)); chi2 = np.zeros(m); piv = np.zeros(m); used = np.zeros(m, np.int32); status = np.zeros(m, np.int32)
    rc = f(*head, n, _p(start), _p(pose), _p(ob) if len(ob) else None, _p(act) if len(act) else None, _p(cm), _p(info), _p(cov), _p(chi2), _p(piv), _p(used), _p(status))
    return rc, dict(info21=info[:n], cov21=cov[:n], chi2=chi2[:n], min_pivot=piv[:n], n_used=used[:n], status=status[:n])


def pose_covariance_batch(ctx, set_start, pose7, obs, active, cam):
    """lpslam_hip_pose_covariance_batch: set i owns observations [set_start[i], set_start[i + 1]) of obs (rows u v ur inv_sigma2 X Y Z) and
    of active (1 = use) and the pose pose7[i]; cam = fx fy cx cy fxb.  Returns a dictionary of info21 (S, 21), cov21 (S, 21), chi2,
    min_pivot, n_used and status (S each; 0 = a covariance, 1 = fewer than 3 observations, 2 = refused)."""
    f = ctx.lib.lpslam_hip_pose_covariance_batch
    f.argtypes = [C.c_void_p] + _POSE_COV_ARGS
    rc, out = _pose_cov(f, (ctx.h,), set_start, pose7, obs, active, cam)
    _check(rc)
    return out


def pose_covariance_batch_host(set_start, pose7, obs, active, cam):
    """lpslam_pose_covariance_batch_host: the CPU definition of pose_covariance_batch (csrc/pose_cov_math.h; the same bits).  A refusal
    raises with the code the device call answers (1 invalid, 3 capacity) in the exception's `code`."""
    f = host_lib().lpslam_pose_covariance_batch_host
    f.argtypes = _POSE_COV_ARGS; f.restype = C.c_int
    rc, out = _pose_cov(f, (), set_start, pose7, obs, active, cam)
    if rc:
        e = LpslamHipError("lpslam_pose_covariance_batch_host refused its arguments (%d)" % rc)
        e.code = rc
        raise e
    return out


def pose_sigmas_host(pose7, cov21):
    """lpslam_pose_sigmas_host: x_sigma, y_sigma, z_sigma (lpslam axes) and the orientation sigma (radians) of a pose's covariance"""
    f = host_lib().lpslam_pose_sigmas_host
    f.argtypes = [C.c_void_p] * 3; f.restype = C.c_int
    pose = np.ascontiguousarray(pose7, np.float64).reshape(7); cov = np.ascontiguousarray(cov21, np.float64).reshape(21); out = np.zeros(4)
    if f(_p(pose), _p(cov), _p(out)):
        raise LpslamHipError("lpslam_pose_sigmas_host refused its arguments")
    return out


def match_orientation_filter(angle_q, angle_t, match_idx):
    aq = np.ascontiguousarray(angle_q, np.float32); at = np.ascontiguousarray(angle_t, np.float32)
    m = np.ascontiguousarray(match_idx, np.int32).copy(); n = C.c_int32()
    _check(load().lpslam_hip_match_orientation_filter(_p(aq), _p(at), _p(m), len(m), C.byref(n)))
    return m, n.value


def pose_optimize(ctx, pose7, points, obs, cam, robust_kernel=True):
    """optimize::pose_optimizer in one launch (lpslam_hip_pose_optimize): returns (pose7, outlier mask, inliers)."""
    pose = np.ascontiguousarray(pose7, np.float64).copy(); pts = np.ascontiguousarray(points, np.float64)
    o = np.ascontiguousarray(obs, BA_OBS_DTYPE)
    c = BaCamera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["fxb"],
                 float(np.sqrt(5.991)) if robust_kernel else 0.0, float(np.sqrt(7.815)) if robust_kernel else 0.0)
    out = np.zeros(max(len(o), 1), np.uint8); n = C.c_int32()
    _check(ctx.lib.lpslam_hip_pose_optimize(ctx.h, _p(pose), _p(pts), len(pts), _p(o), len(o), C.byref(c), _p(out), C.byref(n)))
    return pose, out[:len(o)].astype(bool), n.value


class JpegEncoder:
    """Baseline JPEG encoder on the device (lpslam_hip_jpeg_*): grey images in, the host encoder's streams out, byte for byte."""

    def __init__(self, max_width, max_height, max_images=2):
        self.lib = load()
        self.lib.lpslam_hip_jpeg_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self.lib.lpslam_hip_jpeg_destroy.argtypes = [C.c_void_p]
        self.lib.lpslam_hip_jpeg_encode.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
        h = C.c_void_p()
        _check(self.lib.lpslam_hip_jpeg_create(int(max_width), int(max_height), int(max_images), C.byref(h)))
        self.h = h
        self.max_width, self.max_height, self.max_images = int(max_width), int(max_height), int(max_images)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lpslam_hip_jpeg_destroy(self.h)
            self.h = None

    __del__ = close

    def encode_raw(self, images, quality=95, caps=None):
        """one call for the list of 2-D uint8 images (row strides taken from the arrays): returns (status, sizes, outputs); outputs are
        uint8 arrays of capacity caps[i] (default: enough), to be cut to sizes[i] when status is 0"""
        n = len(images)
        imgs = [np.asarray(im) for im in images]
        if caps is None:
            caps = [1024 + 2 * im.size + 512 for im in imgs]
        outs = [np.full(max(int(c), 1), 0xA5, np.uint8) for c in caps]
        px = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in imgs])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        w = np.array([im.shape[1] for im in imgs] or [0], np.int32)
        hh = np.array([im.shape[0] for im in imgs] or [0], np.int32)
        st = np.array([im.strides[0] for im in imgs] or [0], np.int32)
        cp = np.array(list(caps) or [0], np.int64)
        sz = np.full(max(n, 1), -1, np.int64)
        rc = self.lib.lpslam_hip_jpeg_encode(self.h, n, px, _p(w), _p(hh), _p(st), int(quality), op, _p(cp), _p(sz))
        return rc, sz[:n].copy(), outs

    def encode(self, images, quality=95):
        """list of 2-D uint8 images -> list of JPEG streams (bytes); raises on error"""
        for im in images:
            if np.asarray(im).dtype != np.uint8 or np.asarray(im).ndim != 2 or np.asarray(im).strides[1] != 1:
                raise ValueError("2-D uint8 images with contiguous rows only")
        rc, sizes, outs = self.encode_raw(images, quality)
        _check(rc)
        return [o[:s].tobytes() for o, s in zip(outs, sizes)]


JPEG_DECODED, JPEG_NOT_TAKEN, JPEG_IRREGULAR = 0, 1, 2
JPEG_DEC_COLOR = 1                                      # lpslam_hip_jpeg_dec_create2 flag


class JpegDecoder:
    """Baseline JPEG decoder on the device (lpslam_hip_jpeg_dec_*): streams in, the host decoder's samples out, bit for bit.  Every
    image gets a status: JPEG_DECODED, JPEG_NOT_TAKEN (a class left to the host decoder) or JPEG_IRREGULAR (the host decoder gives the
    verdict).  color=True (LPSLAM_HIP_JPEG_DEC_COLOR): three-component 4:4:4 / 4:2:2 / 4:2:0 streams are taken too and give their first
    component, as the host decoder does; without it they are JPEG_NOT_TAKEN.  restart=True (lpslam_hip_jpeg_dec_take_restart): streams
    of either class with a restart interval are taken too; without it they are JPEG_NOT_TAKEN."""

    def __init__(self, max_width, max_height, max_images=2, color=False, restart=False):
        self.lib = load()
        self.lib.lpslam_hip_jpeg_dec_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self.lib.lpslam_hip_jpeg_dec_create2.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p]
        self.lib.lpslam_hip_jpeg_dec_destroy.argtypes = [C.c_void_p]
        self.lib.lpslam_hip_jpeg_decode.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
        self.lib.lpslam_hip_jpeg_dec_last.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        h = C.c_void_p()
        if color:
            _check(self.lib.lpslam_hip_jpeg_dec_create2(int(max_width), int(max_height), int(max_images), JPEG_DEC_COLOR, C.byref(h)))
        else:
            _check(self.lib.lpslam_hip_jpeg_dec_create(int(max_width), int(max_height), int(max_images), C.byref(h)))
        self.h = h
        self.max_width, self.max_height, self.max_images = int(max_width), int(max_height), int(max_images)
        if restart:
            self.take_restart(True)

    def take_restart(self, on):
        self.lib.lpslam_hip_jpeg_dec_take_restart.argtypes = [C.c_void_p, C.c_int32]
        _check(self.lib.lpslam_hip_jpeg_dec_take_restart(self.h, 1 if on else 0))

    def close(self):
        if getattr(self, "h", None):
            self.lib.lpslam_hip_jpeg_dec_destroy(self.h)
            self.h = None

    __del__ = close

    def decode_raw(self, streams, caps=None, strides=None):
        """one call for the list of streams (bytes): returns (rc, status, widths, heights, outputs); outputs are uint8 arrays of capacity
        caps[i] (default: the decoder's maximum) filled with 0xA5 before the call, rows strides[i] apart (default: the maximum width)"""
        n = len(streams)
        bufs = [np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
        if strides is None:
            strides = [self.max_width] * n
        if caps is None:
            caps = [self.max_width * self.max_height] * n
        outs = [np.full(max(int(c), 1), 0xA5, np.uint8) for c in caps]
        sp = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        ss = np.array([len(s) for s in streams] or [0], np.int64)
        st = np.array(list(strides) or [0], np.int32)
        cp = np.array(list(caps) or [0], np.int64)
        w = np.full(max(n, 1), -1, np.int32); hh = np.full(max(n, 1), -1, np.int32); status = np.full(max(n, 1), -1, np.int32)
        rc = self.lib.lpslam_hip_jpeg_decode(self.h, n, sp, _p(ss), op, _p(st), _p(cp), _p(w), _p(hh), _p(status))
        return rc, status[:n].copy(), w[:n].copy(), hh[:n].copy(), outs

    def decode(self, streams):
        """list of streams -> list of (status, image or None); raises on an error of the call itself"""
        rc, status, w, h, outs = self.decode_raw(streams)
        _check(rc)
        res = []
        for s, ww, hh, o in zip(status, w, h, outs):
            if s != JPEG_DECODED:
                res.append((int(s), None))
                continue
            res.append((int(s), np.lib.stride_tricks.as_strided(o, (int(hh), int(ww)), (self.max_width, 1)).copy()))
        return res

    def last(self, n):
        """test hook: per image of the last call (rounds, subsequences, blocks)"""
        r = np.zeros(n, np.int32); s = np.zeros(n, np.int32); b = np.zeros(n, np.int32)
        _check(self.lib.lpslam_hip_jpeg_dec_last(self.h, int(n), _p(r), _p(s), _p(b)))
        return [(int(x), int(y), int(z)) for x, y, z in zip(r, s, b)]
