"""Writes the JPEG fixtures of this folder and expected.json with Pillow (libjpeg-turbo):

    python tests/golden/jpeg/make_jpeg_fixtures.py [folder with pointgrey1..6.jpg]

expected.json maps every file to its size, its sampling and the SHA-256 of the pixels Pillow decodes from it, as the
library lays them out: (rows, cols) mono8 or (rows, cols, 3) B, G, R, packed.  The hashes are recorded results: they
tie the tests to libjpeg where Pillow is not installed.  The pointgrey files are the reference's own camera frames
(ilcc2/process_data); given their folder, the script copies them here and records their hashes too."""
import hashlib
import io
import json
import os
import shutil
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (4, 3), (7, 5), (8, 8), (9, 7), (16, 16), (17, 33), (31, 16), (33, 17), (50, 35), (255, 9), (257, 9)]   # (w, h)
MODES = [("gray", "L", 0), ("444", "RGB", 0), ("422", "RGB", 1), ("420", "RGB", 2)]   # name, Pillow mode, subsampling


def content(kind, w, h, channels, rng):
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    else:   # a smooth ramp, another direction per channel
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // max(w + h - 2, 1))][:channels],
                     axis=-1).astype(np.uint8)
    return a[..., 0] if channels == 1 else a


def record(expected, name, data):
    im = Image.open(io.BytesIO(data))
    px = np.asarray(im)
    if im.mode == "RGB":
        px = px[..., ::-1]
    sampling = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[im.layer[0][1:3]] if im.mode == "RGB" else "gray"
    expected[name] = {"width": im.width, "height": im.height, "sampling": sampling,
                      "sha256": hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()}


def main():
    rng = np.random.default_rng(20130)
    expected = {}

    def save(name, array, mode, **kw):
        buf = io.BytesIO()
        Image.fromarray(array, mode).save(buf, "JPEG", **kw)
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(buf.getvalue())
        record(expected, name, buf.getvalue())

    for kind in ("noise", "ramp"):
        for w, h in SIZES:
            for mname, mode, sub in MODES:
                for q in (50, 95):
                    for ri in (0, 2):
                        a = content(kind, w, h, 1 if mode == "L" else 3, rng)
                        save("%s_%dx%d_%s_q%d_r%d.jpg" % (kind, w, h, mname, q, ri), a, mode, quality=q, subsampling=sub,
                             restart_marker_blocks=ri)
    a = content("noise", 50, 35, 3, rng)
    save("optimize_50x35_420.jpg", a, "RGB", quality=75, subsampling=2, optimize=True)
    exif = Image.Exif()
    exif[0x010E] = "chessboard"                       # ImageDescription
    save("comment_exif_33x17_422.jpg", content("ramp", 33, 17, 3, rng), "RGB", quality=75, subsampling=1, comment=b"a comment",
         exif=exif.tobytes())
    y, x = np.mgrid[0:24, 0:40]
    checker = (((x // 3 + y // 3) & 1) * 255).astype(np.uint8)
    save("checker_40x24_gray_q100.jpg", checker, "L", quality=100)
    save("checker_40x24_420_q100.jpg", np.stack([checker, 255 - checker, checker], axis=-1), "RGB", quality=100, subsampling=2)

    # frames for the bag chain: a rendered chessboard the detector finds (tests/test_image_corners.py: render_board), gray
    # for ilcc_bag_find_chessboard and tinted 4:2:0 for ilcc_bag_pcd2image
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(os.path.dirname(os.path.dirname(HERE)))]
    from test_image_corners import render_board
    board, _ = render_board((480, 400), theta=0.2, square=36.0, seed=3)
    save("board_480x400_gray_q90.jpg", np.asarray(board), "L", quality=90)
    small, _ = render_board((320, 240), theta=-0.3, square=22.0, seed=5)
    y, x = np.mgrid[0:240, 0:320]
    tinted = np.stack([small, (small * 0.8).astype(np.uint8), ((small * 0.5) + x // 4).astype(np.uint8)], axis=-1)
    save("board_320x240_420_q90.jpg", tinted, "RGB", quality=90, subsampling=2)

    for i in range(1, 7):
        name = "pointgrey%d.jpg" % i
        if len(sys.argv) > 1:
            shutil.copyfile(os.path.join(sys.argv[1], name), os.path.join(HERE, name))
        with open(os.path.join(HERE, name), "rb") as f:
            record(expected, name, f.read())
    with open(os.path.join(HERE, "expected.json"), "w") as f:
        json.dump(expected, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
