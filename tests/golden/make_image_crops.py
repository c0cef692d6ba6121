"""Generate pointgrey<i>_crop.npz from the reference's undistorted camera images.

Usage: python tests/golden/make_image_crops.py <dir holding pointgrey1.jpg .. pointgrey6.jpg>

Each crop is the box around that image's shipped corners (pointgrey<i>.txt, 1-based pixels) grown
by a margin, starting at 160 px, until the crop's min and max grey levels equal the full image's:
findCorners normalises the image by them, so the crop then sees the same normalised values.
Writes ``image`` (uint8, rows x cols) and ``origin`` (x0, y0: the crop's top-left pixel, 0-based).

The six fixtures ``pointgrey{1..6}_crop.npz`` come from the reference's undistorted camera images
(``ilcc2/process_data/pointgrey<i>.jpg``, decoded with Pillow, mode 'L').  Images 1 and 5 need 416
and 696 px margins: their only 0-valued pixels lie far from the board.  They are the input of the
camera-corner reference pin in ``tests/test_image_corners.py``.
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def crop_one(jpg, corners_txt, margin=160):
    img = np.asarray(Image.open(jpg).convert("L"))
    raw = np.loadtxt(corners_txt)
    X, Y = raw[:len(raw) // 2], raw[len(raw) // 2:]
    h, w = img.shape
    lo, hi = int(img.min()), int(img.max())
    while True:
        x0 = max(int(np.floor(X.min() - 1)) - margin, 0)
        y0 = max(int(np.floor(Y.min() - 1)) - margin, 0)
        x1 = min(int(np.ceil(X.max() - 1)) + margin + 1, w)
        y1 = min(int(np.ceil(Y.max() - 1)) + margin + 1, h)
        c = img[y0:y1, x0:x1]
        if int(c.min()) == lo and int(c.max()) == hi:
            return np.ascontiguousarray(c), np.array([x0, y0], dtype=np.int32), margin
        margin += 8


def main(src):
    for i in range(1, 7):
        c, origin, margin = crop_one(os.path.join(src, f"pointgrey{i}.jpg"), os.path.join(HERE, f"pointgrey{i}.txt"))
        out = os.path.join(HERE, f"pointgrey{i}_crop.npz")
        np.savez_compressed(out, image=c, origin=origin)
        print(f"{out}: {c.shape[1]} x {c.shape[0]} at {tuple(origin)}, margin {margin}, {os.path.getsize(out)} B")


if __name__ == "__main__":
    main(sys.argv[1])
