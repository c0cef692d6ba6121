"""Writes expected.json and the small .jpg files of this folder with Pillow (libjpeg-turbo):

    python tests/golden/jpeg_write/make_jpeg_write_fixtures.py

expected.json maps every case of tests/jpeg_write_cases.py to the size and the SHA-256 of the FILE Pillow writes for the
case's seeded source pixels (save(..., "JPEG", quality=q, subsampling=s, restart_marker_blocks=r)), and
"pointgrey1_reencoded_q95" to those of Pillow's re-encode, at quality 95, of what it decodes from
tests/golden/jpeg/pointgrey1.jpg.  The hashes are recorded results: they tie the tests to libjpeg where Pillow is not
installed.  The files kept here are the smallest cases, so that a mismatch can be diffed segment by segment."""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_write_cases as K   # noqa: E402

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def pillow_file(px, mode, quality, restart):
    buf = io.BytesIO()
    if mode == "gray":
        Image.fromarray(np.asarray(px), "L").save(buf, "JPEG", quality=quality, restart_marker_blocks=restart)
    else:
        Image.fromarray(np.ascontiguousarray(np.asarray(px)[..., ::-1]), "RGB").save(buf, "JPEG", quality=quality,
                                                                                     subsampling=SUBSAMPLING[mode],
                                                                                     restart_marker_blocks=restart)
    return buf.getvalue()


def main():
    expected = {}
    keep = set(K.committed_files())
    for name, (_, w, h, mode, q, r) in K.cases().items():
        data = pillow_file(K.source(name), mode, q, r)
        expected[name] = {"bytes": len(data), "sha256": K.sha256(data)}
        if name + ".jpg" in keep:
            with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
                f.write(data)
    frame = np.asarray(Image.open(os.path.join(os.path.dirname(HERE), "jpeg", "pointgrey1.jpg")))
    data = pillow_file(frame, "gray", 95, 0)
    expected["pointgrey1_reencoded_q95"] = {"bytes": len(data), "sha256": K.sha256(data)}
    with open(os.path.join(HERE, "expected.json"), "w") as f:
        json.dump(expected, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
