"""numpy restatement of include/ilcc_camera_image.h (K11): cv_bridge's conversion to mono8 and
cv::undistort(image, K, d, K) as OpenCV 3 documents them -- cvtColor's 14-bit fixed-point gray,
initUndistortRectifyMap's formulas with R = I and the new camera matrix = K, and remap with
INTER_LINEAR, BORDER_CONSTANT 0, 5 fractional bits and 15-bit weights.  OpenCV itself is not
available to the tests, so this file IS the specification ("unpinned"); it has
the role cbdetect_ref.py has for K10.  Every step is one fp64 operation, in the order the header
gives, so that the GPU's unfused arithmetic reproduces it bit for bit.

Also here: the sensor_msgs/Image serializer the bag tests need, and the renderer of a chessboard
seen through the distortion.
"""
import math
import struct
from collections import namedtuple

import numpy as np

IMAGE_MD5 = "060021388200f6f0f447d0fcd9c64743"
IMAGE_TYPE = "sensor_msgs/Image"
ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")          # index = ilcc_image_encoding
BPP = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}
OUTSIDE = -2 ** 31                                                # map code of a pixel with no source
INTER_BITS = 5

Camera = namedtuple("Camera", "fx fy cx cy d width height")      # d = (k1, k2, p1, p2, k3)


def camera(fx, cx, fy, cy, d, width, height):
    d = tuple(float(v) for v in d) + (0.0,) * (5 - len(d))
    return Camera(float(fx), float(fy), float(cx), float(cy), d, int(width), int(height))


def to_mono8(src, encoding):
    """(H, W) or (H, W, C) uint8 -> (H, W) uint8: Y = (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    src = np.asarray(src)
    if encoding == "mono8":
        return src.reshape(src.shape[0], src.shape[1]).copy()
    p = src.astype(np.int64)
    r, b = (p[..., 2], p[..., 0]) if encoding in ("bgr8", "bgra8") else (p[..., 0], p[..., 2])
    return ((4899 * r + 9617 * p[..., 1] + 1868 * b + 8192) >> 14).astype(np.uint8)


def undistort_map(cam):
    """(iu, iv): int32 (height, width) source coordinates in 1/32 pixel, OUTSIDE where there is none."""
    fx, fy, cx, cy = (np.float64(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    k1, k2, p1, p2, k3 = (np.float64(v) for v in cam.d)
    ifx, x0 = np.float64(1.0) / fx, -cx / fx
    ify, y0 = np.float64(1.0) / fy, -cy / fy
    j = np.arange(cam.width, dtype=np.float64)[None, :]
    i = np.arange(cam.height, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = np.broadcast_to(j * ifx + x0, (cam.height, cam.width))
        y = np.broadcast_to(i * ify + y0, (cam.height, cam.width))
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2.0 * x * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)) + cx
        v = fy * (y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy) + cy
        su, sv = u * 32.0, v * 32.0
        ok = (np.abs(su) < 2.0 ** 30) & (np.abs(sv) < 2.0 ** 30)      # False for NaN and inf as well
        iu = np.where(ok, np.rint(np.where(ok, su, 0.0)), OUTSIDE).astype(np.int64)
        iv = np.where(ok, np.rint(np.where(ok, sv, 0.0)), OUTSIDE).astype(np.int64)
    return iu.astype(np.int32), iv.astype(np.int32)


def tap_positions(iu, iv):
    """x0, y0 (floor of the code / 32) and the validity mask; OUTSIDE pixels get a position far outside."""
    valid = iu != OUTSIDE
    x0 = np.where(valid, iu.astype(np.int64) >> INTER_BITS, -4)
    y0 = np.where(valid, iv.astype(np.int64) >> INTER_BITS, -4)
    return x0, y0, valid


def taps_inside(iu, iv, width, height):
    """(4, H, W) bool: which of the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) lie in the source."""
    x0, y0, valid = tap_positions(iu, iv)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            out.append(valid & (xx >= 0) & (xx < width) & (yy >= 0) & (yy < height))
    return np.stack(out)


def remap(mono, iu, iv):
    """remap(INTER_LINEAR, BORDER_CONSTANT 0) of a mono8 image through the 1/32-pixel codes."""
    H, W = mono.shape
    x0, y0, valid = tap_positions(iu, iv)
    a = np.where(valid, iu.astype(np.int64) & 31, 0)
    b = np.where(valid, iv.astype(np.int64) & 31, 0)
    weights = (32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b)
    inside = taps_inside(iu, iv, W, H)
    src = mono.astype(np.int64)
    acc = np.zeros(iu.shape, np.int64)
    k = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = np.clip(x0 + dx, 0, W - 1), np.clip(y0 + dy, 0, H - 1)
            acc += weights[k] * np.where(inside[k], src[yy, xx], 0)
            k += 1
    return ((acc + 16384) >> 15).astype(np.uint8)


def undistort(src, encoding, cam):
    """cv::undistort(mono8(src), K, d, K)."""
    mono = to_mono8(src, encoding)
    assert mono.shape == (cam.height, cam.width)
    return remap(mono, *undistort_map(cam))


def convert(src, encoding, cam=None):
    return to_mono8(src, encoding) if cam is None else undistort(src, encoding, cam)


# ------------------------------------------------------------------------------------------ sensor_msgs/Image

def image_msg(pixels, encoding, *, step=None, seq=0, stamp=(0, 0), frame_id="camera", is_bigendian=0, pad_byte=0xAB,
              width=None, height=None, data=None):
    """Serialise sensor_msgs/Image: header, height, width, encoding, is_bigendian, step, data[].
    `pixels`: (H, W) or (H, W, C) uint8; rows are padded to `step` bytes with pad_byte.  `encoding` may be
    any string (the parser's refusals are tested with encodings the writer knows nothing about)."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    H, W = pixels.shape[:2]
    rows = pixels.reshape(H, -1)
    step = rows.shape[1] if step is None else step
    if data is None:
        if step > rows.shape[1]:
            rows = np.concatenate([rows, np.full((H, step - rows.shape[1]), pad_byte, np.uint8)], 1)
        data = rows.tobytes()
    out = struct.pack("<III", seq, stamp[0], stamp[1])
    out += struct.pack("<I", len(frame_id)) + frame_id.encode()
    out += struct.pack("<II", H if height is None else height, W if width is None else width)
    out += struct.pack("<I", len(encoding)) + encoding.encode()
    out += struct.pack("<BI", is_bigendian, step)
    out += struct.pack("<I", len(data)) + data
    return out


# ------------------------------------------------------------------------------------------ a board through the lens

def distort_points(cam, u, v):
    """Pinhole pixel (u, v) -> pixel of the distorted image (the forward model of undistort_map, in floats)."""
    k1, k2, p1, p2, k3 = cam.d
    x, y = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    return (cam.fx * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cam.cx,
            cam.fy * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cam.cy)


def undistort_points(cam, u, v, iterations=30):
    """Pixel of the distorted image -> pinhole pixel: the model's fixed point, iterated."""
    k1, k2, p1, p2, k3 = cam.d
    xd, yd = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / kr, (yd - dy) / kr
    return x * cam.fx + cam.cx, y * cam.fy + cam.cy


def render_board(size, cam=None, board=(7, 5), square=40.0, theta=0.0, centre=None, persp=(0.0, 0.0), blur=1.0, noise=2.0,
                 seed=0):
    """test_image_corners.render_board (same homography convention, blur and noise) with the lens in front:
    the pattern is sampled at the undistorted position of every 4 x 4 sub-pixel of the distorted image.
    Returns the uint8 image and the true 0-based PINHOLE inner-corner positions [y][x] -> (u, v)."""
    W, H = size
    rng = np.random.default_rng(seed)
    c, s = math.cos(theta), math.sin(theta)
    cx, cy = centre if centre is not None else (W / 2, H / 2)
    bw, bh = board
    ox, oy = (bw + 1) * square / 2, (bh + 1) * square / 2
    A = np.array([[c, -s, cx - (c * ox - s * oy)], [s, c, cy - (s * ox + c * oy)], [persp[0], persp[1], 1.0]])
    A[2, 2] = 1.0 - persp[0] * cx - persp[1] * cy
    Hinv = np.linalg.inv(A)
    ss = (np.arange(4) + 0.5) / 4 - 0.5
    acc = np.zeros((H, W))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for dy in ss:
        for dx in ss:
            px, py = xs + dx, ys + dy
            if cam is not None:
                px, py = undistort_points(cam, px, py)
            q = Hinv @ np.stack([px.ravel(), py.ravel(), np.ones(xs.size)])
            X, Y = (q[0] / q[2]).reshape(H, W), (q[1] / q[2]).reshape(H, W)
            inside = (X >= 0) & (X < (bw + 1) * square) & (Y >= 0) & (Y < (bh + 1) * square)
            black = (np.floor(X / square) + np.floor(Y / square)) % 2 == 0
            acc += np.where(inside & black, 30.0, 220.0)
    img = acc / 16
    if blur > 0:
        r = int(math.ceil(3 * blur))
        k = np.exp(-0.5 * (np.arange(-r, r + 1) / blur) ** 2)
        k /= k.sum()
        img = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, np.pad(img, r, mode="edge"))
        img = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, img)[r:-r, r:-r]
    img = img + rng.normal(0, noise, img.shape)
    img[0, 0], img[-1, -1] = 0, 255
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    P = np.array([[A @ np.array([(i + 1) * square, (j + 1) * square, 1.0]) for i in range(bw)] for j in range(bh)])
    return img, P[..., :2] / P[..., 2:3]
