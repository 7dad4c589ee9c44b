"""ctypes face of the host library (lpslam_amd/liblpslam.so): the plain-C shim over the C++ LpSlamManager mirror
(lpslam_amd/host/interface.cpp).  Used by the tests; C++ clients include include/lpslam_manager.h instead."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblpslam.so")


class ROSTimestamp(C.Structure):
    _fields_ = [("seconds", C.c_int32), ("nanoseconds", C.c_int64)]


class Position(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("x", "y", "z", "x_sigma", "y_sigma", "z_sigma")]


class OrientationS(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("w", "x", "y", "z", "sigma")]


class GlobalState(C.Structure):
    _fields_ = [("position", Position), ("orientation", OrientationS), ("valid", C.c_bool)]


class GlobalStateInTime(C.Structure):
    _fields_ = [("timestamp", C.c_int64), ("ros_timestamp", ROSTimestamp), ("has_ros_timestamp", C.c_uint8), ("state", GlobalState)]


class ImageDescription(C.Structure):
    _fields_ = [("structure", C.c_int), ("format", C.c_int), ("image_conversion", C.c_int), ("height", C.c_uint32),
                ("width", C.c_uint32), ("imageSize", C.c_uint32), ("imageSizeSecond", C.c_uint32),
                ("hasRosTimestamp", C.c_uint8), ("rosTimestamp", ROSTimestamp)]


class CameraConfiguration(C.Structure):
    _fields_ = [("camera_number", C.c_uint32), ("distortion_function", C.c_int), ("f_x", C.c_double), ("f_y", C.c_double),
                ("c_x", C.c_double), ("c_y", C.c_double), ("dist", C.c_double * 8), ("mask_type", C.c_int),
                ("mask_parameter", C.c_double), ("resolution_x", C.c_int), ("resolution_y", C.c_int), ("fps", C.c_double),
                ("focal_x_baseline", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3)]


class Status(C.Structure):
    _fields_ = [("localization", C.c_int), ("feature_points", C.c_long), ("key_frames", C.c_long), ("frame_time", C.c_double), ("fps", C.c_double)]


class FeatureEntry(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class MapInfo(C.Structure):
    _fields_ = [("x_cell_size", C.c_float), ("y_cell_size", C.c_float), ("x_cell_count", C.c_uint32), ("y_cell_count", C.c_uint32),
                ("x_origin", C.c_float), ("y_origin", C.c_float)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


RECON_CB = C.CFUNCTYPE(None, C.POINTER(GlobalStateInTime), C.c_void_p)
IMAGE_CB = C.CFUNCTYPE(None, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint8), ImageDescription, C.c_void_p)
NAV_CB = C.CFUNCTYPE(C.c_int, ROSTimestamp, C.POINTER(GlobalStateInTime), C.POINTER(GlobalStateInTime), C.c_void_p)

STEREO_TWO_BUFFER, FORMAT_8UC1, FORMAT_8UC3, NO_DISTORTION, ODOM_ONLY = 3, 1, 2, 3, 1
PINHOLE, FISHEYE, OMNI = 0, 1, 2          # LpSlamCameraDistortionFunction
ONE_IMAGE_COMPRESSED, STEREO_COMPRESSED = 4, 5          # LpSlamImageStructure
ONE_IMAGE, STEREO_LEFT_TOP_RIGHT_BOTTOM, STEREO_LEFT_LEFT_RIGHT_RIGHT = 0, 1, 2
FORMAT_8UC4, FORMAT_NV12, FORMAT_YUV16 = 3, 4, 5          # LpSlamImageFormat (YUV16: UYVY, two bytes per pixel)
CONVERSION_NONE, CONVERSION_BGR2RGB = 0, 1          # LpSlamImageConversion
PIXEL_GRAY8, PIXEL_RGB8, PIXEL_BGR8, PIXEL_NV12, PIXEL_UYVY = range(5)          # LPSLAM_HIP_PIXEL_* (include/lpslam_hip.h)
JPEG_DECODE_DEVICE_KEY = "jpeg_decode_device"          # manager section of the configuration file: false = decode compressed frames on the host
JPEG_DECODE_COLOR_DEVICE_KEY = "jpeg_decode_color_device"    # the same for three-component (YCbCr) streams alone; default true
JPEG_DECODE_RESTART_DEVICE_KEY = "jpeg_decode_restart_device"    # true = streams with a restart interval go to the device too; default false
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.lpslam_manager_create.restype = C.c_void_p
        for name in ("destroy", "start", "stop"):
            getattr(_lib, "lpslam_manager_" + name).argtypes = [C.c_void_p]
        _lib.lpslam_manager_set_log_level.argtypes = [C.c_void_p, C.c_int]
        for name in ("add_tracker", "add_processor", "add_source"):
            getattr(_lib, "lpslam_manager_" + name).argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        _lib.lpslam_manager_read_configuration_file.argtypes = [C.c_void_p, C.c_char_p]
        _lib.lpslam_manager_log_to_file.argtypes = [C.c_void_p, C.c_char_p]
        _lib.lpslam_manager_read_replay_items.argtypes = [C.c_void_p, C.c_char_p]
        _lib.lpslam_manager_set_camera_configuration.argtypes = [C.c_void_p, C.POINTER(CameraConfiguration)]
        _lib.lpslam_manager_default_camera_configuration.argtypes = [C.POINTER(CameraConfiguration)]
        _lib.lpslam_manager_on_reconstruction.argtypes = [C.c_void_p, RECON_CB, C.c_void_p]
        _lib.lpslam_manager_on_image.argtypes = [C.c_void_p, IMAGE_CB, C.c_void_p]
        _lib.lpslam_manager_request_nav_data.argtypes = [C.c_void_p, NAV_CB, C.c_void_p]
        _lib.lpslam_manager_add_stereo_image.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ImageDescription)]
        _lib.lpslam_manager_add_image.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(ImageDescription)]
        _lib.lpslam_manager_status.argtypes = [C.c_void_p, C.POINTER(Status)]
        _lib.lpslam_manager_features.argtypes = [C.c_void_p, C.POINTER(FeatureEntry), C.c_size_t, C.POINTER(C.c_float)]
        _lib.lpslam_manager_features.restype = C.c_size_t
        _lib.lpslam_manager_features_count.argtypes = [C.c_void_p]
        _lib.lpslam_manager_features_count.restype = C.c_size_t
        _lib.lpslam_roundtrip_state.argtypes = [C.POINTER(GlobalStateInTime), C.POINTER(GlobalStateInTime)]
    return _lib


def default_camera():
    c = CameraConfiguration()
    load().lpslam_manager_default_camera_configuration(C.byref(c))
    return c


class Manager:
    def __init__(self, log_level=2):
        self.lib = load()
        self.h = self.lib.lpslam_manager_create()
        self.lib.lpslam_manager_set_log_level(self.h, log_level)
        self.results = []
        self._keep = []

    def close(self):
        if self.h:
            self.lib.lpslam_manager_destroy(self.h)
            self.h = None

    __del__ = close

    def log_to_file(self, path, level=1):
        """LpSlamManager::logToFile + setLogLevel (1 = Info): the tracker's statistics line is read back from it by the tests"""
        self.lib.lpslam_manager_set_log_level(self.h, level)
        self.lib.lpslam_manager_log_to_file(self.h, str(path).encode())

    @staticmethod
    def statistics(path):
        """the last "VSLAM statistics: key=value ..." line of a log file as a dict (counters as ints, ms_* timings as floats)"""
        out = {}
        for line in open(path, errors="replace"):
            if "VSLAM statistics:" in line:
                out = {k: (float(v) if k.startswith("ms_") else int(v)) for k, v in (kv.split("=") for kv in line.split("VSLAM statistics:")[1].split())}
        return out

    def tracker_statistics(self):
        """this manager's own "VSLAM statistics" line of its last stop() as a dict (the log file is process-wide)"""
        f = self.lib.lpslam_manager_tracker_statistics
        f.restype = C.c_size_t; f.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        buf = C.create_string_buffer(8192)          # (the line has grown past 2 KB of keys and values)
        f(self.h, buf, 8192)
        line = buf.value.decode(errors="replace")
        if "VSLAM statistics:" not in line:
            return {}
        return {k: (float(v) if k.startswith("ms_") else int(v)) for k, v in (kv.split("=") for kv in line.split("VSLAM statistics:")[1].split())}

    def read_configuration_file(self, path):
        return bool(self.lib.lpslam_manager_read_configuration_file(self.h, path.encode()))

    def add_tracker(self, name, cfg=""):
        """cfg: the tracker's JSON object as text; every key goes to the plugin as written (INTEGRATION.md lists them, e.g.
        "triangulateNeighbours": 10, "relocaliseOnDevice": true, "initialiseOnDevice": true, "verifyLoopsOnDevice": true,
        "poseSigma": true -- the results' x_sigma, y_sigma, z_sigma and orientation sigma from the pose covariance call, `sigma` of collect_results)"""
        return bool(self.lib.lpslam_manager_add_tracker(self.h, name.encode(), cfg.encode()))

    def add_processor(self, name, cfg=""):
        return bool(self.lib.lpslam_manager_add_processor(self.h, name.encode(), cfg.encode()))

    def read_replay_items(self, path):
        return bool(self.lib.lpslam_manager_read_replay_items(self.h, str(path).encode()))

    def add_source(self, name, cfg=""):
        return bool(self.lib.lpslam_manager_add_source(self.h, name.encode(), cfg.encode()))

    def set_camera(self, cam):
        self.lib.lpslam_manager_set_camera_configuration(self.h, C.byref(cam))

    def collect_results(self, on_result=None):
        def cb(state, _):
            s = state.contents
            self.results.append(dict(timestamp=s.timestamp, valid=bool(s.state.valid),
                                     p=(s.state.position.x, s.state.position.y, s.state.position.z),
                                     q=(s.state.orientation.w, s.state.orientation.x, s.state.orientation.y, s.state.orientation.z),
                                     sigma=(s.state.position.x_sigma, s.state.position.y_sigma, s.state.position.z_sigma, s.state.orientation.sigma)))
            if on_result is not None:
                on_result()
        f = RECON_CB(cb); self._keep.append(f)
        self.lib.lpslam_manager_on_reconstruction(self.h, f, None)

    def count_results(self):
        """installs the library's compiled counting callback (no interpreter on the notify thread): result_counts() = (results, valid)"""
        self.lib.lpslam_manager_count_results.argtypes = [C.c_void_p]
        self.lib.lpslam_manager_count_results(self.h)

    def result_counts(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.lpslam_manager_result_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self.lib.lpslam_manager_result_counts(self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def collect_images(self):
        """LpSlamManager::addOnImageCallback: every frame the worker takes comes back as JPEG (quality 70) on the image thread;
        self.images gets (timestamp, camera, structure, format, left stream, right stream or None)"""
        self.images = []

        def cb(ts, cam, buf, desc, _):
            n0, n1 = int(desc.imageSize), int(desc.imageSizeSecond)
            raw = C.string_at(buf, n0 + n1)
            self.images.append((int(ts), int(cam), int(desc.structure), int(desc.format), raw[:n0], raw[n0:] if n1 else None))
        f = IMAGE_CB(cb); self._keep.append(f)
        self.lib.lpslam_manager_on_image(self.h, f, None)

    def provide_odometry(self, native=False):
        """answers every navigation request with a valid identity odometry; native=True installs the library's compiled callback
        (lpslam_manager_request_identity_nav_data) instead of a Python one -- no interpreter on the worker thread's path"""
        if native:
            self.lib.lpslam_manager_request_identity_nav_data.argtypes = [C.c_void_p]
            self.lib.lpslam_manager_request_identity_nav_data(self.h)
            return

        def cb(ts, odom, mp, _):
            odom.contents.state.valid = True
            odom.contents.state.orientation.w = 1.0
            return ODOM_ONLY
        f = NAV_CB(cb); self._keep.append(f)
        self.lib.lpslam_manager_request_nav_data(self.h, f, None)

    def add_buffer(self, ts_ns, buf, width, height, fmt, structure=ONE_IMAGE, conversion=CONVERSION_NONE, image_size=None, camera=0, ros=True):
        """addImageFromBuffer with a single-buffer frame of any format and structure: `buf` holds the bytes as the client has them
        (Stereo_LeftTop_RightBottom: `height` counts both eyes; NV12 / YUV16: each eye a complete picture, the LOWER one the left
        camera's); image_size: desc.imageSize (default: the buffer's size)"""
        import numpy as np
        buf = np.ascontiguousarray(buf, np.uint8)
        d = ImageDescription(int(structure), int(fmt), int(conversion), int(height), int(width), buf.size if image_size is None else int(image_size), 0,
                             1 if ros else 0, ROSTimestamp(int(ts_ns // 10**9), int(ts_ns)))
        return bool(self.lib.lpslam_manager_add_image(self.h, camera, int(ts_ns), buf.ctypes.data, C.byref(d)))

    def add_stereo(self, ts_ns, left, right, ros=True, fmt=FORMAT_8UC1, conversion=CONVERSION_NONE):
        """two buffers: (h, w) uint8 each, or -- fmt=FORMAT_8UC3 -- (h, w, 3)"""
        d = ImageDescription(STEREO_TWO_BUFFER, int(fmt), int(conversion), left.shape[0], left.shape[1], left.size, right.size,
                             1 if ros else 0, ROSTimestamp(int(ts_ns // 10**9), int(ts_ns)))
        return bool(self.lib.lpslam_manager_add_stereo_image(self.h, 0, int(ts_ns), left.ctypes.data, right.ctypes.data, C.byref(d)))

    def add_image(self, ts_ns, img, camera=0, ros=True):
        d = ImageDescription(0, FORMAT_8UC1, 0, img.shape[0], img.shape[1], img.size, 0, 1 if ros else 0, ROSTimestamp(int(ts_ns // 10**9), int(ts_ns)))
        return bool(self.lib.lpslam_manager_add_image(self.h, camera, int(ts_ns), img.ctypes.data, C.byref(d)))

    def add_jpeg(self, ts_ns, data, camera=0, ros=True):
        """a compressed frame (LpSlamImageFormat_8UC1_JPEPG, one image): decoded by the manager as the reference does with cv::imdecode"""
        raw = bytes(data)
        buf = C.create_string_buffer(raw, len(raw))
        d = ImageDescription(0, 0, 0, 0, 0, len(raw), 0, 1 if ros else 0, ROSTimestamp(int(ts_ns // 10**9), int(ts_ns)))
        return bool(self.lib.lpslam_manager_add_image(self.h, camera, int(ts_ns), C.cast(buf, C.c_void_p), C.byref(d)))

    def add_jpeg_pair(self, ts_ns, left, right, camera=0, ros=True):
        """a compressed stereo frame as the image callback hands it out (Stereo_Compressed: the left stream, then the right one)"""
        raw = bytes(left) + bytes(right)
        buf = C.create_string_buffer(raw, len(raw))
        d = ImageDescription(STEREO_COMPRESSED, 0, 0, 0, 0, len(left), len(right), 1 if ros else 0, ROSTimestamp(int(ts_ns // 10**9), int(ts_ns)))
        return bool(self.lib.lpslam_manager_add_image(self.h, camera, int(ts_ns), C.cast(buf, C.c_void_p), C.byref(d)))

    @staticmethod
    def compress_image(bgra):
        """LpSlamManager::compressImage: an (h, w, 4) BGRA image -> the JPEG stream of its grey version (bytes), or None"""
        import numpy as np
        bgra = np.ascontiguousarray(bgra, np.uint8)
        h, w = bgra.shape[:2]
        d = ImageDescription(0, 3, 0, h, w, bgra.size, 0, 0, ROSTimestamp(0, 0))          # LpSlamImageFormat_8UC4
        out = np.zeros(bgra.size, np.uint8)
        n = C.c_uint32(0)
        f = load().lpslam_manager_compress_image
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(ImageDescription), C.c_void_p, C.POINTER(C.c_uint32)]
        if not f(bgra.ctypes.data, C.byref(d), out.ctypes.data, C.byref(n)):
            return None
        return out[:n.value].tobytes()

    def set_record(self, on):
        """setRecord: start() writes the session to slam_<local time>.pb in the working directory ("Recording file")"""
        f = self.lib.lpslam_manager_set_record; f.argtypes = [C.c_void_p, C.c_int]
        f(self.h, 1 if on else 0)

    def set_record_images(self, on):
        """setRecordImages: False drops the camera records (result records are still written)"""
        f = self.lib.lpslam_manager_set_record_images; f.argtypes = [C.c_void_p, C.c_int]
        f(self.h, 1 if on else 0)

    def set_write_image_files(self, on):
        """setWriteImageFiles: every 10th frame the worker takes as <n>_left.jpg / <n>_right.jpg in the working directory"""
        f = self.lib.lpslam_manager_set_write_image_files; f.argtypes = [C.c_void_p, C.c_int]
        f(self.h, 1 if on else 0)

    def recorder_counters(self):
        """test hook: {device_images, host_images, records, bytes} of this manager's recorder"""
        import numpy as np
        out = np.zeros(4, np.uint64)
        f = self.lib.lpslam_manager_recorder_counters; f.argtypes = [C.c_void_p, C.c_void_p]
        f(self.h, out.ctypes.data)
        return dict(zip(("device_images", "host_images", "records", "bytes"), (int(v) for v in out)))

    def decoder_counters(self):
        """test hook: {device_images, host_images, refused_images}: the compressed images of this manager's replay and of add_jpeg /
        add_jpeg_pair, by where they were decoded.  The device path is on unless the configuration file says
        {"manager": {"jpeg_decode_device": false}} (JPEG_DECODE_DEVICE_KEY)."""
        import numpy as np
        out = np.zeros(3, np.uint64)
        f = self.lib.lpslam_manager_decoder_counters; f.argtypes = [C.c_void_p, C.c_void_p]
        f(self.h, out.ctypes.data)
        return dict(zip(("device_images", "host_images", "refused_images"), (int(v) for v in out)))

    def start(self):
        self.lib.lpslam_manager_start(self.h)

    def stop(self):
        self.lib.lpslam_manager_stop(self.h)

    def status(self):
        s = Status()
        self.lib.lpslam_manager_status(self.h, C.byref(s))
        return s

    def features(self, cap=100000):
        buf = (FeatureEntry * cap)()
        t = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
        n = self.lib.lpslam_manager_features(self.h, buf, cap, t)
        return [(buf[i].x, buf[i].y, buf[i].z) for i in range(n)]

    def features_count(self):
        return int(self.lib.lpslam_manager_features_count(self.h))

    def mapping_set_mode(self, enable):
        """mappingSetMode: mapping on (True) or localisation only against a loaded map (False); call before start()"""
        f = self.lib.lpslam_manager_mapping_set_mode; f.argtypes = [C.c_void_p, C.c_int]; f.restype = C.c_int
        return bool(f(self.h, 1 if enable else 0))

    def mapping_set_filename(self, path):
        """mappingSetFilename: the map database file (used when the tracker's useMapDb is on); call before start()"""
        f = self.lib.lpslam_manager_mapping_set_filename; f.argtypes = [C.c_void_p, C.c_char_p]; f.restype = C.c_int
        return bool(f(self.h, str(path).encode()))

    def add_laser_scan(self, ros_ts_ns, ranges, range_min, range_max, angle_min, angle_max, increment, range_threshold):
        """mappingAddLaserScan; the scan's ROS time is stamped as add_stereo stamps a frame's (ros_ts_ns in nanoseconds)"""
        import numpy as np
        r = np.ascontiguousarray(ranges, np.float32)
        ts = ROSTimestamp(int(ros_ts_ns // 10**9), int(ros_ts_ns))
        f = self.lib.lpslam_manager_add_laser_scan
        f.argtypes = [C.c_void_p, C.POINTER(ROSTimestamp), C.c_void_p, C.c_size_t] + [C.c_float] * 6
        f(self.h, C.byref(ts), r.ctypes.data, len(r), float(range_min), float(range_max), float(angle_min), float(angle_max),
          float(increment), float(range_threshold))

    def provide_laser_transform(self, R, t):
        """answers RequestNavTransformation(Laser -> Camera) with the laser's pose in the camera's lpslam frame (rotation matrix R,
        translation t); call before start()"""
        f = self.lib.lpslam_manager_provide_laser_transform; f.argtypes = [C.c_void_p, C.POINTER(GlobalState)]
        self._laser_state = laser_state(R, t)
        f(self.h, C.byref(self._laser_state))

    def map_raw_size(self):
        f = self.lib.lpslam_manager_map_raw_size; f.argtypes = [C.c_void_p]; f.restype = C.c_ulong
        return int(f(self.h))

    def map_scans(self):
        """test hook: the scans the grid is built from: (ROS time nanoseconds field, origin, fwd, left) each"""
        import numpy as np
        f = self.lib.lpslam_manager_map_scans; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]; f.restype = C.c_size_t
        n = f(self.h, None, None, 0)
        st = (ROSTimestamp * max(n, 1))(); ps = np.zeros((max(n, 1), 7), np.float64)      # lpslam_hip_scan_pose: key, pad, 6 doubles
        n = min(n, f(self.h, st, ps.ctypes.data, n))
        return [(st[i].nanoseconds, ps[i, 1:3].copy(), ps[i, 3:5].copy(), ps[i, 5:7].copy()) for i in range(n)]

    def map_raw(self, capacity=None):
        """mappingGetMapRaw: (LpMapInfo fields, np.int8 grid of shape (height, width)); capacity: the buffer's size (default: the
        current map_raw_size())"""
        import numpy as np
        cap = self.map_raw_size() if capacity is None else int(capacity)
        buf = np.full(max(cap, 1), -1, np.int8)
        info = MapInfo()
        f = self.lib.lpslam_manager_map_raw; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(MapInfo)]
        f(self.h, buf.ctypes.data, cap, C.byref(info))
        w, h = info.x_cell_count, info.y_cell_count
        return info.as_dict(), buf[:w * h].reshape(h, w)


def adjust_intensity(img, low_out=-0.3, high_out=1.4, low_fraction=0.01, high_fraction=0.99, padding=None):
    """the host implementation of the AdjustIntensity processor's arithmetic (lpslam_adjust_intensity), CPU only: `img` is a 2-D uint8
    array whose rows may be strided (a view of a wider array); returns (adjusted copy of the same shape, lo, hi), or None when the
    library rejects the arguments.  padding: a list that receives the bytes between the rows after the call (they start as 0xA5)"""
    import numpy as np
    assert img.dtype == np.uint8 and img.ndim == 2 and (img.shape[1] == 1 or img.strides[1] == 1)
    h, w = img.shape
    stride = max(int(img.strides[0]), w)
    buf = np.full(h * stride, 0xA5, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, shape=(h, w), strides=(stride, 1))
    rows[...] = img
    params = (C.c_double * 4)(float(low_out), float(high_out), float(low_fraction), float(high_fraction))
    lo_hi = (C.c_int * 2)(-1, -1)
    f = load().lpslam_adjust_intensity
    f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    if not f(buf.ctypes.data, w, h, stride, params, lo_hi):
        return None
    if padding is not None:
        padding.append(buf.reshape(h, stride)[:, w:].copy())
    return rows.copy(), int(lo_hi[0]), int(lo_hi[1])


def gray_from_pixels(data, width, height, fmt, stride=None, chroma=None, chroma_stride=0, padding=None, out_stride=None):
    """the host implementation of the colour / YUV -> grey conversion (lpslam_gray_from_pixels), CPU only: `data` is a uint8 array
    that holds the frame (rows `stride` bytes apart, default: tightly packed), fmt a PIXEL_* constant; returns the (height, width) grey
    image, or None when the library rejects the arguments.  padding: a list that receives the bytes between the output rows (0xA5)"""
    import numpy as np
    data = np.ascontiguousarray(data, np.uint8)
    row = {PIXEL_GRAY8: width, PIXEL_RGB8: 3 * width, PIXEL_BGR8: 3 * width, PIXEL_NV12: width, PIXEL_UYVY: 2 * width}.get(fmt, width)
    stride = row if stride is None else int(stride)
    ostride = width if out_stride is None else int(out_stride)
    out = np.full(height * ostride, 0xA5, np.uint8)
    f = load().lpslam_gray_from_pixels
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    ch = None if chroma is None else np.ascontiguousarray(chroma, np.uint8)
    if not f(out.ctypes.data, ostride, int(width), int(height), data.ctypes.data, stride, None if ch is None else ch.ctypes.data, int(chroma_stride), int(fmt)):
        return None
    out = out.reshape(height, ostride)
    if padding is not None:
        padding.append(out[:, width:].copy())
    return out[:, :width].copy()


def realise_entry(data, width, height, fmt, adjust=None):
    """test hook (lpslam_realise_entry): a queue entry with `data` as its pending colour source (tightly packed) and, with
    adjust = (low_out, high_out, low_fraction, high_fraction), a pending intensity adjustment, through realiseGray + realiseAdjust"""
    import numpy as np
    data = np.ascontiguousarray(data, np.uint8)
    row = {PIXEL_RGB8: 3 * width, PIXEL_BGR8: 3 * width, PIXEL_NV12: width, PIXEL_UYVY: 2 * width}[fmt]
    out = np.zeros((height, width), np.uint8)
    f = load().lpslam_realise_entry
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]
    params = None if adjust is None else (C.c_double * 4)(*[float(v) for v in adjust])
    if not f(data.ctypes.data, data.size, row, int(width), int(height), int(fmt), params, out.ctypes.data):
        return None
    return out


def laser_state(R, t):
    """LpSlamGlobalState of a rotation matrix and a translation (lpslam axes)"""
    import numpy as np
    R = np.asarray(R, np.float64)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    s = GlobalState()
    s.position.x, s.position.y, s.position.z = (float(v) for v in t)
    s.orientation.w, s.orientation.x, s.orientation.y, s.orientation.z = w, x, y, z
    s.valid = True
    return s


def scan_pose(T_cw, state):
    """the map-plane pose of a keyframe's scan (host/occupancy.h), CPU only: T_cw 4x4 (optical axes), state the laser -> camera
    LpSlamGlobalState (GlobalState).  Returns (origin, fwd, left), each (y, z) of the world's lpslam axes"""
    import numpy as np
    lib = load()
    T = np.ascontiguousarray(T_cw, np.float64).reshape(16)
    out = np.zeros(6, np.float64)
    f = lib.lpslam_occupancy_scan_pose; f.argtypes = [C.c_void_p, C.POINTER(GlobalState), C.c_void_p]
    f(T.ctypes.data, C.byref(state), out.ctypes.data)
    return out[:2].copy(), out[2:4].copy(), out[4:].copy()


def map_file_info(path):
    """validates a map database file: (True, counts) with counts = {keyframes, live_keyframes, landmarks, next_landmark_id, stereo},
    or (False, reason)"""
    lib = load()
    f = lib.lpslam_map_file_info; f.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]; f.restype = C.c_int
    counts = (C.c_int64 * 5)(); why = C.create_string_buffer(512)
    if not f(str(path).encode(), counts, why, 512):
        return False, why.value.decode()
    return True, dict(zip(("keyframes", "live_keyframes", "landmarks", "next_landmark_id", "stereo"), list(counts)))


def map_file_rewrite(src, dst):
    """reads a map database file and writes it back: (True, "") or (False, reason)"""
    lib = load()
    f = lib.lpslam_map_file_rewrite; f.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]; f.restype = C.c_int
    why = C.create_string_buffer(512)
    ok = bool(f(str(src).encode(), str(dst).encode(), why, 512))
    return ok, why.value.decode()


def map_file_camera_check(path, session):
    """compares a map file's camera record with a session's (lpslam_map_file_camera_check): session = 16 numbers {stereo, width, height,
    fx, fy, cx, cy, focal_x_baseline, num_levels, scale_factor, model, k1 .. k4, max_angle -- model 2: k1, k2, p1, p2, k3}.  (1, "") they agree; (0, what differs);
    (-1, why the file itself was rejected)"""
    import numpy as np
    lib = load()
    f = lib.lpslam_map_file_camera_check; f.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t]; f.restype = C.c_int
    s = np.ascontiguousarray(session, np.float64)
    assert s.size == 16
    why = C.create_string_buffer(512)
    rc = int(f(str(path).encode(), s.ctypes.data, why, 512))
    return rc, why.value.decode()


def fisheye_undistort(model, xy):
    """the host form of the fisheye undistortion (csrc/fisheye_math.h), CPU only: model = 9 numbers {fx, fy, cx, cy, k1 .. k4, max_angle
    in radians}, xy (n, 2) float64 pixels.  Returns (out (n, 2) float32 with NaN where invalid, valid (n,) bool, theta (n,))"""
    import numpy as np
    lib = load()
    f = lib.lpslam_fisheye_undistort; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = None
    m = np.ascontiguousarray(model, np.float64); xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    out = np.zeros((n, 2), np.float32); valid = np.zeros(n, np.uint8); theta = np.zeros(n, np.float64)
    f(m.ctypes.data, xy.ctypes.data, n, out.ctypes.data, valid.ctypes.data, theta.ctypes.data)
    return out, valid.astype(bool), theta


def fisheye_forward(model, xyz, width, height):
    """the host form of the forward model and the tracker's visibility rule, CPU only: xyz (n, 3) camera-frame points.  Returns (sensor
    pixel (n, 2), angle from the axis (n,), visible (n,) bool)"""
    import numpy as np
    lib = load()
    f = lib.lpslam_fisheye_forward; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = None
    m = np.ascontiguousarray(model, np.float64); xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n = len(xyz)
    s = np.zeros((n, 2), np.float64); theta = np.zeros(n, np.float64); vis = np.zeros(n, np.uint8)
    f(m.ctypes.data, xyz.ctypes.data, n, int(width), int(height), s.ctypes.data, theta.ctypes.data, vis.ctypes.data)
    return s, theta, vis.astype(bool)


def fisheye_session_model(mgr, yaml_path=None, max_angle_deg=70.0):
    """the keypoint camera a monocular tracker of Manager `mgr` would start with (camera 0 of its configuration, the YAML file of
    configFromFile, fisheyeMaxAngleDeg), without a device: (1, 9 numbers), (0, None) for a camera that is not a fisheye one, (-1, reason)"""
    import numpy as np
    f = mgr.lib.lpslam_manager_fisheye_session_model
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_void_p, C.c_char_p, C.c_size_t]; f.restype = C.c_int
    model = np.zeros(9, np.float64); why = C.create_string_buffer(512)
    rc = int(f(mgr.h, (str(yaml_path).encode() if yaml_path else None), float(max_angle_deg), model.ctypes.data, why, 512))
    return (rc, model) if rc == 1 else (rc, why.value.decode() if rc < 0 else None)


def radtan_undistort(model, xy):
    """the host form of the radial-tangential undistortion (csrc/radtan_math.h), CPU only: model = 9 numbers {fx, fy, cx, cy, k1, k2, p1,
    p2, k3}, xy (n, 2) float64 pixels.  Returns (out (n, 2) float32 with NaN where invalid, valid (n,) bool, squared residual in pixels
    (n,), smallest denominator of the five steps (n,))"""
    import numpy as np
    lib = load()
    f = lib.lpslam_radtan_undistort; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = None
    m = np.ascontiguousarray(model, np.float64); xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    out = np.zeros((n, 2), np.float32); valid = np.zeros(n, np.uint8); res2 = np.zeros(n, np.float64); den = np.zeros(n, np.float64)
    f(m.ctypes.data, xy.ctypes.data, n, out.ctypes.data, valid.ctypes.data, res2.ctypes.data, den.ctypes.data)
    return out, valid.astype(bool), res2, den


def radtan_bounds(model, width, height):
    """the bounds of the undistorted image as the tracker computes them at start, CPU only: ((min_x, max_x, min_y, max_y), share of
    invalid border pixels), or (None, share) when no border pixel is valid (the start is refused)"""
    import numpy as np
    lib = load()
    f = lib.lpslam_radtan_bounds; f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]; f.restype = C.c_int
    m = np.ascontiguousarray(model, np.float64); b = np.zeros(4, np.float64); share = C.c_double()
    ok = f(m.ctypes.data, int(width), int(height), b.ctypes.data, C.byref(share))
    return (tuple(b) if ok else None), share.value


def radtan_forward(model, xyz, bounds, width, height):
    """the host form of the forward model and the tracker's visibility rule, CPU only: xyz (n, 3) camera-frame points, bounds as
    radtan_bounds gives them.  Returns (sensor pixel (n, 2), visible (n,) bool)"""
    import numpy as np
    lib = load()
    f = lib.lpslam_radtan_forward; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]; f.restype = None
    m = np.ascontiguousarray(model, np.float64); xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(bounds, np.float64)
    n = len(xyz)
    s = np.zeros((n, 2), np.float64); vis = np.zeros(n, np.uint8)
    f(m.ctypes.data, xyz.ctypes.data, n, b.ctypes.data, int(width), int(height), s.ctypes.data, vis.ctypes.data)
    return s, vis.astype(bool)


def radtan_session_model(mgr, yaml_path=None):
    """the radial-tangential keypoint camera a monocular tracker of Manager `mgr` would start with (camera 0 of its configuration, the
    YAML file of configFromFile), without a device: (1, 9 numbers), (0, None) for no model, (-1, reason)"""
    import numpy as np
    f = mgr.lib.lpslam_manager_radtan_session_model
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t]; f.restype = C.c_int
    model = np.zeros(9, np.float64); why = C.create_string_buffer(512)
    rc = int(f(mgr.h, (str(yaml_path).encode() if yaml_path else None), model.ctypes.data, why, 512))
    return (rc, model) if rc == 1 else (rc, why.value.decode() if rc < 0 else None)


TRI_KP_DTYPE = [("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("x_right", "<f4"), ("depth", "<f4")]      # lpslam_hip_tri_keypoint


def tri_candidates_host(cam, scale, kp1, desc1, group1, kp2, desc2, group2, F, epipole):
    """the host form of the triangulation step's candidate gate (csrc/triangulate_math.h), CPU only: cam = 6 numbers {fx, fy, cx, cy,
    focal_x_baseline, scale_factor}, kp1 / kp2 arrays of TRI_KP_DTYPE, epipole (x, y) or None.  Returns (j (n1, 8) with -1, dist (n1, 8)
    with 256, count (n1,), keys (n1, 8) uint64)"""
    import numpy as np
    f = load().lpslam_tri_candidates_host
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = None
    cam = np.ascontiguousarray(cam, np.float64); scale = np.ascontiguousarray(scale, np.float32)
    kp1 = np.ascontiguousarray(kp1, np.dtype(TRI_KP_DTYPE)); kp2 = np.ascontiguousarray(kp2, np.dtype(TRI_KP_DTYPE))
    desc1 = np.ascontiguousarray(desc1, np.uint8); desc2 = np.ascontiguousarray(desc2, np.uint8)
    group1 = np.ascontiguousarray(group1, np.int32); group2 = np.ascontiguousarray(group2, np.int32)
    F = np.ascontiguousarray(F, np.float64).reshape(9); ep = np.array([0.0, 0.0] if epipole is None else [epipole[0], epipole[1]], np.float64)
    n1, n2 = len(kp1), len(kp2)
    keys = np.full((n1, 8), 2 ** 64 - 1, np.uint64); count = np.zeros(n1, np.int32)
    f(cam.ctypes.data, scale.ctypes.data, kp1.ctypes.data, desc1.ctypes.data, group1.ctypes.data, n1, kp2.ctypes.data, desc2.ctypes.data, group2.ctypes.data, n2,
      F.ctypes.data, ep.ctypes.data, 0 if epipole is None else 1, keys.ctypes.data, count.ctypes.data)
    empty = keys == np.uint64(2 ** 64 - 1)
    j = np.where(empty, -1, (keys & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
    dist = np.where(empty, 256, (keys >> np.uint64(32)).astype(np.int64)).astype(np.int32)
    return j, dist, count, keys


def tri_pair_host(cam, scale, pose1, pose2, kp1, kp2):
    """the host form of tri_pair on n pairs: (code (n,) int32, X (n, 3) float64 with NaN where the code is 0)"""
    import numpy as np
    f = load().lpslam_tri_pair_host
    f.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p]; f.restype = None
    cam = np.ascontiguousarray(cam, np.float64); scale = np.ascontiguousarray(scale, np.float32)
    pose1 = np.ascontiguousarray(pose1, np.float64); pose2 = np.ascontiguousarray(pose2, np.float64)
    kp1 = np.ascontiguousarray(kp1, np.dtype(TRI_KP_DTYPE)); kp2 = np.ascontiguousarray(kp2, np.dtype(TRI_KP_DTYPE))
    n = len(kp1)
    code = np.zeros(n, np.int32); X = np.full((n, 3), np.nan, np.float64)
    f(cam.ctypes.data, scale.ctypes.data, pose1.ctypes.data, pose2.ctypes.data, kp1.ctypes.data, kp2.ctypes.data, n, code.ctypes.data, X.ctypes.data)
    return code, X


def tri_replay_host(keys, count, n2, skip=None):
    """the ordered replay of one neighbour over candidate lists (keys (n1, 8) uint64): (match (n1,), rank (n1,), exhausted)"""
    import numpy as np
    f = load().lpslam_tri_replay_host
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]; f.restype = C.c_int
    keys = np.ascontiguousarray(keys, np.uint64); count = np.ascontiguousarray(count, np.int32)
    n1 = len(count)
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    match = np.zeros(n1, np.int32); rank = np.zeros(n1, np.int32)
    ex = f(keys.ctypes.data, count.ctypes.data, n1, int(n2), None if skip is None else skip.ctypes.data, match.ctypes.data, rank.ctypes.data)
    return match, rank, int(ex)


def tri_epipolar(cam, pose_c, pose_n):
    """F (3, 3) with x_n^T F x_c = 0 and the epipole of c in n ((x, y) or None), as the tracker derives them"""
    import numpy as np
    f = load().lpslam_tri_epipolar
    f.argtypes = [C.c_void_p] * 5; f.restype = C.c_int
    cam = np.ascontiguousarray(cam, np.float64); pc = np.ascontiguousarray(pose_c, np.float64); pn = np.ascontiguousarray(pose_n, np.float64)
    F = np.zeros(9, np.float64); ep = np.zeros(2, np.float64)
    has = f(cam.ctypes.data, pc.ctypes.data, pn.ctypes.data, F.ctypes.data, ep.ctypes.data)
    return F.reshape(3, 3), (float(ep[0]), float(ep[1])) if has else None


def tri_option_ok(n):
    """whether the tracker accepts triangulateNeighbours = n"""
    f = load().lpslam_tri_option_ok; f.argtypes = [C.c_int]; f.restype = C.c_int
    return bool(f(int(n)))


def tri_neighbour_list(covisible, prev, n):
    """the tracker's neighbour list: the covisible keyframes in their order, the previous keyframe (prev >= 0) in front when absent, cut to n"""
    import numpy as np
    f = load().lpslam_tri_neighbour_list; f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]; f.restype = C.c_int
    cov = np.ascontiguousarray(covisible, np.int32)
    out = np.zeros(len(cov) + 1, np.int32)
    k = f(cov.ctypes.data, len(cov), int(prev), int(n), out.ctypes.data)
    return [int(v) for v in out[:k]]


def tri_baseline_accepts(pose_c, pose_n, min_distance):
    import numpy as np
    f = load().lpslam_tri_baseline_accepts; f.argtypes = [C.c_void_p, C.c_void_p, C.c_double]; f.restype = C.c_int
    pc = np.ascontiguousarray(pose_c, np.float64); pn = np.ascontiguousarray(pose_n, np.float64)
    return bool(f(pc.ctypes.data, pn.ctypes.data, float(min_distance)))


def tri_median_depth(depths):
    import numpy as np
    f = load().lpslam_tri_median_depth; f.argtypes = [C.c_void_p, C.c_int]; f.restype = C.c_double
    d = np.ascontiguousarray(depths, np.float64)
    return float(f(d.ctypes.data, len(d)))
