"""numpy restatement of what include/ilcc_overlay.h chains beyond camera_image_ref.py: cv_bridge's conversion to
bgr8 and cv::undistort of the COLOUR image (K11c), and pcd2image's cv::circle per projected point (K12).  OpenCV is
not available to the tests, so -- as for K11 -- this file IS the specification.

The map and the tap positions are camera_image_ref's own (imported, not restated); the blend is applied to each of
B, G, R.  cv::circle(image, Point(x, y), 0.6, Scalar(r, g, b), 2): the radius is an int, so 0.6 becomes 0; with
thickness 2 OpenCV 3 goes EllipseEx -> PolyLine -> ThickLine on a zero-length segment, which draws a filled Circle of
radius (2 * 2^15 + 2^15) >> 16 = 1, whose midpoint loop fills row y: x-1 .. x+1 and rows y-1, y+1: x only.
Scalar(r, g, b) on a bgr8 image puts r into byte 0."""
import numpy as np

from camera_image_ref import image_msg, tap_positions, undistort_map  # noqa: F401  (image_msg: for the bag tests)

REFERENCE_STAMP = ((0, -1), (-1, 0), (0, 0), (1, 0), (0, 1))       # (dx, dy)
HIT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("pad", "u1"), ("index", "<u4")])


def to_bgr8(src, encoding):
    """(H, W) or (H, W, C) uint8 -> (H, W, 3) uint8 B, G, R."""
    src = np.asarray(src)
    if encoding == "mono8":
        return np.repeat(src.reshape(src.shape[0], src.shape[1], 1), 3, axis=2)
    if encoding in ("bgr8", "bgra8"):
        return src[..., :3].copy()
    if encoding in ("rgb8", "rgba8"):
        return src[..., 2::-1].copy()
    raise ValueError(encoding)


def undistort_bgr8(src, encoding, cam):
    """cv::undistort(bgr8(src), K, d, K): remap(INTER_LINEAR, BORDER_CONSTANT 0) of every channel."""
    bgr = to_bgr8(src, encoding).astype(np.int64)
    H, W = bgr.shape[:2]
    assert (H, W) == (cam.height, cam.width)
    iu, iv = undistort_map(cam)
    x0, y0, valid = tap_positions(iu, iv)
    a = np.where(valid, iu.astype(np.int64) & 31, 0)
    b = np.where(valid, iv.astype(np.int64) & 31, 0)
    acc = np.zeros((H, W, 3), np.int64)
    for dx, dy, wgt in ((0, 0, 32 * (32 - a) * (32 - b)), (1, 0, 32 * a * (32 - b)), (0, 1, 32 * (32 - a) * b), (1, 1, 32 * a * b)):
        xx, yy = x0 + dx, y0 + dy
        inside = valid & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)      # each tap on its own
        tap = np.where(inside[..., None], bgr[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)
        acc += wgt[..., None] * tap
    return ((acc + 16384) >> 15).astype(np.uint8)


def convert_bgr8(src, encoding, cam=None):
    return to_bgr8(src, encoding) if cam is None else undistort_bgr8(src, encoding, cam)


def make_hits(x, y, rgb):
    """HIT_DTYPE records from coordinates and (n, 3) colours; index = position."""
    x = np.asarray(x)
    hits = np.zeros(x.size, HIT_DTYPE)
    hits["x"], hits["y"] = x, y
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    hits["r"], hits["g"], hits["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    hits["index"] = np.arange(x.size)
    return hits


def draw_hits(image, hits, stamp=REFERENCE_STAMP):
    """The sequential loop of pcd2image.cpp:59-83 on a copy of the (H, W, 3) image: python ints, so x + dx cannot wrap."""
    out = np.array(image, copy=True)
    H, W = out.shape[:2]
    xs, ys = hits["x"].tolist(), hits["y"].tolist()
    colours = np.stack([hits["r"], hits["g"], hits["b"]], 1)
    for k in range(len(xs)):
        for dx, dy in stamp:
            px, py = xs[k] + dx, ys[k] + dy
            if 0 <= px < W and 0 <= py < H:
                out[py, px] = colours[k]
    return out


def draw_hits_highest_wins(image, hits, stamp=REFERENCE_STAMP):
    """The same image stated another way: every pixel takes the colour of the highest hit index whose stamp covers it."""
    out = np.array(image, copy=True)
    H, W = out.shape[:2]
    owner = np.zeros(H * W, np.int64)
    x, y = hits["x"].astype(np.int64), hits["y"].astype(np.int64)
    k1 = np.arange(1, len(hits) + 1, dtype=np.int64)
    for dx, dy in stamp:
        px, py = x + dx, y + dy
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        np.maximum.at(owner, py[ok] * W + px[ok], k1[ok])
    owner = owner.reshape(H, W)
    drawn = owner > 0
    who = owner[drawn] - 1
    out[drawn] = np.stack([hits["r"][who], hits["g"][who], hits["b"][who]], 1)
    return out


def read_ppm(path):
    """(H, W, 3) R,G,B pixels of a binary PPM as ilcc_save_ppm_bgr writes it."""
    blob = open(path, "rb").read()
    magic, size, maxval, rest = blob.split(b"\n", 3)
    assert magic == b"P6" and maxval == b"255", blob[:20]
    w, h = (int(v) for v in size.split())
    assert len(rest) == 3 * w * h
    return np.frombuffer(rest, np.uint8).reshape(h, w, 3)
