"""numpy restatement of the Bayer part of include/ilcc_camera_image.h: what cv_bridge::toCvCopy(msg, MONO8 / "bgr8") makes
of a bayer_rggb8 / bayer_bggr8 / bayer_gbrg8 / bayer_grbg8 frame, i.e. OpenCV 3's scalar Bayer2RGB_ and Bayer2Gray_
(imgproc/src/demosaicing.cpp).  OpenCV is not available to the tests, so -- as camera_image_ref.py for the rest of K11 --
this file IS the specification.  It is written twice, and tests/test_bayer_cpu.py holds the two
against each other byte for byte:

  demosaic()       the positional rules of the header, vectorised: every interior pixel from its site's colour, then the
                   border by clamping the coordinates;
  demosaic_scan()  a plain loop in the shape of OpenCV's: row by row from the raw row above, `start_with_green` and the
                   side the blue channel lies on toggling per row, pixels taken in green / non-green turns, the two
                   border columns copied per row and the two border rows copied at the end.

The lens is camera_image_ref's own (undistort_map, remap; per channel for colour), and so is the message writer."""
import numpy as np

from camera_image_ref import image_msg, remap, undistort_map  # noqa: F401  (image_msg: for the bag tests)

BAYER_ENCODINGS = {"bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19}   # ilcc_image_encoding
PATTERNS = tuple(BAYER_ENCODINGS)
CR, CG, CB = 4899, 9617, 1868


def cfa(encoding):
    """The four letters of the name: the colours of pixels (0,0), (1,0) of row 0 and (0,1), (1,1) of row 1."""
    letters = encoding[len("bayer_"):-1]
    assert encoding in BAYER_ENCODINGS and sorted(letters) == ["b", "g", "g", "r"]
    return letters


def site_colours(encoding, w, h):
    """(h, w) array of 'r' / 'g' / 'b': the colour the sensor measures at every pixel."""
    letters = np.array(list(cfa(encoding))).reshape(2, 2)
    return letters[np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]


def mosaic(bgr, encoding):
    """Sample a (h, w, 3) B,G,R scene through the colour filter array: (h, w) raw bytes."""
    bgr = np.asarray(bgr)
    sites = site_colours(encoding, bgr.shape[1], bgr.shape[0])
    return np.where(sites == "b", bgr[..., 0], np.where(sites == "g", bgr[..., 1], bgr[..., 2])).astype(np.uint8)


# ------------------------------------------------------------------------------------------ (a) positional, vectorised

def _interior(raw, encoding):
    """B, G, R and Y of the interior pixels (1 .. h-2, 1 .. w-2) as int64 arrays (h-2, w-2)."""
    S = np.asarray(raw).astype(np.int64)
    h, w = S.shape
    c = S[1:-1, 1:-1]
    left, right, up, down = S[1:-1, :-2], S[1:-1, 2:], S[:-2, 1:-1], S[2:, 1:-1]
    cross = left + right + up + down
    diag = S[:-2, :-2] + S[:-2, 2:] + S[2:, :-2] + S[2:, 2:]
    sites = site_colours(encoding, w, h)
    own = sites[1:-1, 1:-1]
    # the colour of the row's non-green sites, per row (every row holds exactly one of r, b)
    row_colour = np.where((sites == "r").any(1), "r", "b")[1:-1, None]
    out = {}
    green = own == "g"
    g = np.where(green, c, (cross + 2) >> 2)
    horizontal, vertical = (left + right + 1) >> 1, (up + down + 1) >> 1
    opposite = (diag + 2) >> 2
    for colour, other in (("r", "b"), ("b", "r")):
        at_green = np.where(row_colour == colour, horizontal, vertical)
        out[colour] = np.where(green, at_green, np.where(own == colour, c, opposite))
    c_row = np.where(row_colour == "r", CR, CB)
    c_col = np.where(row_colour == "r", CB, CR)
    y_green = (2 * CG * c + c_row * (left + right) + c_col * (up + down) + 16384) >> 15
    c_own = np.where(own == "r", CR, CB)
    c_opp = np.where(own == "r", CB, CR)
    y_colour = (4 * c_own * c + CG * cross + c_opp * diag + 32768) >> 16
    return out["b"], g, out["r"], np.where(green, y_green, y_colour)


def _with_border(inner, w, h):
    """D(x, y) = I(clamp(x, 1, w-2), clamp(y, 1, h-2))"""
    yy = np.clip(np.arange(h), 1, h - 2) - 1
    xx = np.clip(np.arange(w), 1, w - 2) - 1
    return inner[yy[:, None], xx[None, :]]


def demosaic(raw, encoding, gray=False):
    """(h, w) raw uint8 -> (h, w, 3) uint8 B,G,R, or (h, w) uint8 Y with gray=True.  w, h >= 3."""
    raw = np.asarray(raw)
    h, w = raw.shape
    if w < 3 or h < 3:
        raise ValueError("a Bayer image must be at least 3 x 3")
    b, g, r, y = _interior(raw, encoding)
    if gray:
        return _with_border(y, w, h).astype(np.uint8)
    return np.stack([_with_border(v, w, h) for v in (b, g, r)], 2).astype(np.uint8)


# ------------------------------------------------------------------------------------------ (b) the scanning loop

def demosaic_scan(raw, encoding, gray=False):
    """The same image by OpenCV's own route.  For the row that is written (y + 1) the loop reads raw rows y, y + 1, y + 2
    at columns x, x + 1, x + 2 and writes pixel (x + 1, y + 1)."""
    S = [[int(v) for v in row] for row in np.asarray(raw)]
    h, w = len(S), len(S[0])
    if w < 3 or h < 3:
        raise ValueError("a Bayer image must be at least 3 x 3")
    letters = cfa(encoding)
    start_with_green = letters[3] == "g"                 # pixel (1, 1), the first one written
    blue = -1 if "b" in letters[2:] else 1                # channel offset from G of row 1's non-green colour: B is G - 1
    bcoeff, rcoeff = (CB, CR) if blue == -1 else (CR, CB)
    chans = 1 if gray else 3
    dst = [[[0] * chans for _ in range(w)] for _ in range(h)]
    for y in range(h - 2):
        r0, r1, r2 = S[y], S[y + 1], S[y + 2]
        out = dst[y + 1]
        green = start_with_green
        for x in range(w - 2):
            if green:
                if gray:
                    t0 = (r0[x + 1] + r2[x + 1]) * rcoeff
                    t1 = (r1[x] + r1[x + 2]) * bcoeff
                    t2 = r1[x + 1] * (2 * CG)
                    out[x + 1][0] = (t0 + t1 + t2 + (1 << 14)) >> 15
                else:
                    t0 = (r0[x + 1] + r2[x + 1] + 1) >> 1
                    t1 = (r1[x] + r1[x + 2] + 1) >> 1
                    px = out[x + 1]
                    px[1 - blue] = t0
                    px[1] = r1[x + 1]
                    px[1 + blue] = t1
            else:
                if gray:
                    t0 = (r0[x] + r0[x + 2] + r2[x] + r2[x + 2]) * rcoeff
                    t1 = (r0[x + 1] + r1[x] + r1[x + 2] + r2[x + 1]) * CG
                    t2 = r1[x + 1] * (4 * bcoeff)
                    out[x + 1][0] = (t0 + t1 + t2 + (1 << 15)) >> 16
                else:
                    t0 = (r0[x] + r0[x + 2] + r2[x] + r2[x + 2] + 2) >> 2
                    t1 = (r0[x + 1] + r1[x] + r1[x + 2] + r2[x + 1] + 2) >> 2
                    px = out[x + 1]
                    px[1 - blue] = t0
                    px[1] = t1
                    px[1 + blue] = r1[x + 1]
            green = not green
        out[0] = list(out[1])
        out[w - 1] = list(out[w - 2])
        blue = -blue
        bcoeff, rcoeff = rcoeff, bcoeff
        start_with_green = not start_with_green
    dst[0] = [list(p) for p in dst[1]]
    dst[h - 1] = [list(p) for p in dst[h - 2]]
    a = np.array(dst, np.int64)
    assert a.min() >= 0 and a.max() <= 255
    return a[..., 0].astype(np.uint8) if gray else a.astype(np.uint8)


# ------------------------------------------------------------------------------------------ with the lens

def to_mono8(raw, encoding, cam=None):
    """cv_bridge's MONO8 of a Bayer frame, then cv::undistort when a camera is given."""
    y = demosaic(raw, encoding, gray=True)
    return y if cam is None else remap(y, *undistort_map(cam))


def to_bgr8(raw, encoding, cam=None):
    """cv_bridge's "bgr8" of a Bayer frame, then cv::undistort of every channel when a camera is given."""
    bgr = demosaic(raw, encoding)
    if cam is None:
        return bgr
    iu, iv = undistort_map(cam)
    return np.stack([remap(np.ascontiguousarray(bgr[..., k]), iu, iv) for k in range(3)], 2)
