"""Reference arithmetic of the radial-tangential keypoint camera in numpy float64, written from the definition:
the five fixed-point steps of the undistortion with the validity rule, the forward model, the bounds of the undistorted image, the
tracker's visibility rule and the stable compaction the device stage performs on a keypoint slot."""
import numpy as np

ITERATIONS = 5
MAX_RES2 = 0.25          # (0.5 pixel)^2: the localisation quantum of a level-0 FAST corner


class Model:
    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.p1, self.p2, self.k3 = float(k1), float(k2), float(p1), float(p2), float(k3)

    def as_array(self):
        return np.array([self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.p1, self.p2, self.k3], np.float64)


# the two planted models of the tests: a mild barrel lens, and one that folds over inside a 640 x 480 image
MILD = Model(520.0, 520.0, 320.0, 240.0, -0.25, 0.06, 0.001, -0.0005, 0.0)
FOLD = Model(400.0, 405.0, 320.0, 240.0, -0.6, 0.05, 0.002, -0.001, 0.0)


def distort(m, x, y):
    """normalised -> normalised distorted"""
    r2 = x * x + y * y
    rad = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2
    xd = x * rad + 2.0 * m.p1 * x * y + m.p2 * (r2 + 2.0 * x * x)
    yd = y * rad + m.p1 * (r2 + 2.0 * y * y) + 2.0 * m.p2 * x * y
    return xd, yd


def undistort(m, xy):
    """xy: (n, 2) pixels.  Returns a dict: out (n, 2) float32 (NaN where invalid), valid, den (n, 5) the denominator of every step,
    min_den, res2 the squared distance in pixels between the pixel and the forward model of the (FP64) result."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    with np.errstate(all="ignore"):
        x0 = (xy[:, 0] - m.cx) / m.fx; y0 = (xy[:, 1] - m.cy) / m.fy
        x, y = x0.copy(), y0.copy()
        den = np.zeros((n, ITERATIONS), np.float64)
        for it in range(ITERATIONS):
            r2 = x * x + y * y
            d = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2
            dx = 2.0 * m.p1 * x * y + m.p2 * (r2 + 2.0 * x * x)
            dy = m.p1 * (r2 + 2.0 * y * y) + 2.0 * m.p2 * x * y
            den[:, it] = d
            x = (x0 - dx) / d; y = (y0 - dy) / d
        xd, yd = distort(m, x, y)
        ex = m.fx * xd + m.cx - xy[:, 0]; ey = m.fy * yd + m.cy - xy[:, 1]
        res2 = ex * ex + ey * ey
        rx = m.fx * x + m.cx; ry = m.fy * y + m.cy
        valid = (den > 0.0).all(axis=1) & (res2 <= MAX_RES2) & np.isfinite(rx) & np.isfinite(ry)
        out = np.stack([rx, ry], 1).astype(np.float32)
    out[~valid] = np.nan
    min_den = np.fmin.reduce(den, axis=1, initial=np.inf)            # (fmin: a NaN denominator is not a minimum)
    return {"out": out, "valid": valid, "den": den, "min_den": min_den, "res2": res2}


def decisive(r, margin=1e-9):
    """points whose validity does not hang on the last bits: the squared residual not within `margin` (relative) of the bound, and no
    denominator within `margin` of zero"""
    with np.errstate(invalid="ignore"):
        near_res = np.abs(r["res2"] - MAX_RES2) <= margin * MAX_RES2
        near_den = (np.abs(r["den"]) < margin).any(axis=1) if len(r["den"]) else np.zeros(0, bool)
    return ~(near_res | near_den)


def forward(m, xyz):
    """camera-frame points (n, 3), z > 0: sensor pixel (n, 2)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        xd, yd = distort(m, xyz[:, 0] / xyz[:, 2], xyz[:, 1] / xyz[:, 2])
        return np.stack([m.fx * xd + m.cx, m.fy * yd + m.cy], 1)


def border_pixels(width, height):
    xs = np.arange(width, dtype=np.float64); ys = np.arange(1, height - 1, dtype=np.float64)
    return np.concatenate([np.stack([xs, np.zeros(width)], 1), np.stack([xs, np.full(width, height - 1.0)], 1),
                           np.stack([np.zeros(len(ys)), ys], 1), np.stack([np.full(len(ys), width - 1.0), ys], 1)])


def bounds(m, width, height):
    """((min_x, max_x, min_y, max_y) over the valid border pixels or None when there is none, share of invalid border pixels)"""
    r = undistort(m, border_pixels(width, height))
    v = r["valid"]
    if not v.any():
        return None, 1.0
    o = r["out"][v].astype(np.float64)
    return (o[:, 0].min(), o[:, 0].max(), o[:, 1].min(), o[:, 1].max()), float((~v).mean())


def visible(m, b, xyz, width, height):
    """the tracker's rule: in front, the pinhole (u, v) inside the bounds, the sensor pixel inside the image"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = m.fx * xyz[:, 0] / xyz[:, 2] + m.cx; v = m.fy * xyz[:, 1] / xyz[:, 2] + m.cy
        s = forward(m, xyz)
        return (xyz[:, 2] > 0) & (u >= b[0]) & (u <= b[1]) & (v >= b[2]) & (v <= b[3]) & (s[:, 0] >= 0) & (s[:, 0] < width) & (s[:, 1] >= 0) & (s[:, 1] < height)


def compact(m, kp, desc):
    """the device stage on one slot: kp (structured, fields x / y / ...), desc (n, 32).  Survivors in order with x, y replaced; every
    other field and the descriptors untouched.  Returns (kp, desc, dropped, result of undistort)."""
    r = undistort(m, np.stack([kp["x"].astype(np.float64), kp["y"].astype(np.float64)], 1))
    keep = r["valid"]
    out = kp[keep].copy()
    out["x"] = r["out"][keep, 0]; out["y"] = r["out"][keep, 1]
    return out, desc[keep].copy(), int((~keep).sum()), r


def ulp_diff(a, b):
    """distance of float32 arrays in units in the last place"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
