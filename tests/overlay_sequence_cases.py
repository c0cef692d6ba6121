"""Constructed inputs for K12b (include/ilcc_overlay_sequence.h) beyond paired_cases.py's batches.  Deterministic; no GPU needed.

  collision_batch   scan 0: 4097 + 300 points that all project into ONE pixel, with distinct intensities: the last point's colour
                    must win across the chunk seam; scan 1: a 3 x 3 block of pixels hit by interleaved points whose stamps overlap;
                    scans 2 and 3: two scans that share one image and hit the same pixels with other colours
  stamp_of_64       the custom stamp test_stream_contract.py builds for K12, restated
  hundreds          300 scans of 1 .. 5 points on the 37 x 23 camera"""
import numpy as np

import paired_cases as K
import project_cases as P

W, H = 16, 12
DIS = 8.0
ONE_PIXEL = (5, 7)
N_ONE_PIXEL = P.CHUNK + 1 + 300


def camera():
    return P.camera(width=W, height=H)          # identity: (x + 0.5, y + 0.5, 1) lands in pixel (x, y)


def _at(pixels, intensity):
    px = np.asarray(pixels, np.float64).reshape(-1, 2)
    return P.as_points(np.stack([px[:, 0] + 0.5, px[:, 1] + 0.5, np.ones(len(px))], 1), np.asarray(intensity, np.float32))


def one_pixel_scan():
    n = N_ONE_PIXEL
    return _at([ONE_PIXEL] * n, np.arange(n) % 61)                # hues 0 .. 255 over and over; the last point's is 17


def block_scan():
    """400 points that walk a 3 x 3 block in a scrambled order: every pixel is covered by the stamps of its neighbours' points too."""
    rng = np.random.default_rng(33)
    cells = [(x, y) for y in (3, 4, 5) for x in (9, 10, 11)]
    order = np.concatenate([rng.permutation(9) for _ in range(45)])[:400]
    return _at([cells[k] for k in order], (np.arange(400) * 7) % 61)


def shared_scans():
    rng = np.random.default_rng(34)
    pixels = np.stack([rng.integers(0, W, 150), rng.integers(0, H, 150)], 1)
    return _at(pixels, np.arange(150) % 61), _at(pixels[::-1], (np.arange(150) * 5 + 30) % 61)


def collision_batch():
    rng = np.random.default_rng(35)
    images = [rng.integers(0, 256, (H, 3 * W), dtype=np.uint8), rng.integers(0, 256, (H, 3 * W + 7), dtype=np.uint8)]
    a, b = shared_scans()
    return K._batch("collisions", [(one_pixel_scan(), 0), (block_scan(), 0), (a, 1), (b, 1)], images, camera(), DIS)


def stamp_of_64():
    rng = np.random.default_rng(11)
    stamp = [(127, 127), (-127, 127), (127, -127), (-127, -127), (-128, -128), (0, 0)]
    return stamp + [(int(a), int(b)) for a, b in rng.integers(-128, 128, (58, 2))]


def hundreds():
    name, cam, pts, tight, padded = [c for c in P.camera_family() if c[0] == "37x23 inside"][0]
    lengths = [1 + k % 5 for k in range(300)]
    assert sum(lengths) <= len(pts)
    scans, at = [], 0
    for k, n in enumerate(lengths):
        scans.append((pts[at:at + n], -1 if k % 17 == 5 else k % 2))
        at += n
    return K._batch("300 scans of 1 .. 5 points", scans, [tight, padded], cam, P.CAMERA_DIS)
