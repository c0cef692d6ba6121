"""numpy specification of include/ilcc_overlay_sequence.h, composed from the restatements the single-scan entries already have:
project_cases.project_intensity (K8's intensity entry) and overlay_ref.draw_hits (K12's sequential loop).  No GPU is needed here.

  overlay_batch          K12b: per paired scan, the hits of the scan drawn on a copy of its image; n_drawn = the hits
  highest_point_wins     the same picture stated the way K12b computes it: every pixel takes the colour of the highest IN-SCAN POINT
                         index whose stamp covers it, without a hit list
  canvas_bytes           the whole output array as the entry leaves it: rows at their stride, canvases at their pitch, FILL elsewhere
  sequence_bytes         ilcc_overlay_sequence_bytes from the three JPEG sizes it adds up
  chain                  ilcc_bag_pcd2image_all_pairs: paired_ref.pair_by_stamp + paired_ref.image_to_bgr8 + overlay_batch +
                         jpeg_write_ref.encode of the B,G,R picture at 4:2:0"""
import numpy as np

import jpeg_write_ref
import overlay_ref as O
import paired_ref
import project_cases as P

REFERENCE_STAMP = O.REFERENCE_STAMP


def packed(image, cam):
    """(H, step) uint8 rows of B,G,R -> (H, W, 3)"""
    img = np.asarray(image, np.uint8)
    return img[:, :3 * cam.width].reshape(cam.height, cam.width, 3)


def overlay_batch(xyzi, offsets, images, image_of_scan, cam, dis, lo=0.0, hi=60.0, stamp=REFERENCE_STAMP):
    """-> (canvases: per scan an (H, W, 3) uint8 picture, None for an unpaired scan; n_drawn [n_scans] uint32)"""
    xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    canvases, n_drawn = [], np.zeros(len(image_of_scan), np.uint32)
    for s, k in enumerate(image_of_scan):
        if k < 0:
            canvases.append(None)
            continue
        hits = P.project_intensity(xyzi[int(offsets[s]):int(offsets[s + 1])], cam, dis, lo, hi)
        canvases.append(O.draw_hits(packed(images[k], cam), hits, stamp))
        n_drawn[s] = len(hits)
    return canvases, n_drawn


def highest_point_wins(points, image, cam, dis, lo=0.0, hi=60.0, stamp=REFERENCE_STAMP):
    """One scan the way K12b draws it: owner[pixel] = max over the kept points whose stamp covers it of (in-scan index + 1); the
    pixel takes that point's colour.  No compaction, no hit index."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    out = np.array(packed(image, cam), copy=True)
    H, W = out.shape[:2]
    sp = P.space_to_plane(pts, cam, dis)
    idx = np.flatnonzero(sp["keep"]).astype(np.int64)
    x, y = sp["px"][idx].astype(np.int64), sp["py"][idx].astype(np.int64)
    owner = np.zeros(H * W, np.int64)
    for dx, dy in stamp:
        px, py = x + dx, y + dy
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        np.maximum.at(owner, py[ok] * W + px[ok], idx[ok] + 1)
    owner = owner.reshape(H, W)
    drawn = owner > 0
    who = owner[drawn] - 1
    out[drawn] = P.hsv_to_rgb(P.hue_of(pts[who, 3], lo, hi))            # (r, g, b) into bytes 0, 1, 2
    return out, len(idx)


def canvas_bytes(canvases, cam, stride, pitch, total, fill):
    """The output array of `total` bytes: scan s's rows at s * pitch + y * stride, 3 * width bytes each; `fill` everywhere else."""
    out = np.full(int(total), fill, np.uint8)
    w3 = 3 * cam.width
    for s, c in enumerate(canvases):
        if c is None:
            continue
        assert s * pitch + stride * (cam.height - 1) + w3 <= total
        rows = np.lib.stride_tricks.as_strided(out[s * pitch:], (cam.height, w3), (stride, 1))
        rows[:] = np.ascontiguousarray(c, np.uint8).reshape(cam.height, w3)
    return out


def up(x, to=256):
    return (int(x) + to - 1) // to * to


def sequence_bytes(width, height, out_bytes_per_image, coef_count, fdct_scratch, k17_scratch):
    """The header's formula; the three JPEG sizes are the library's own for ilcc_jpeg_write_info(width, height, 3, 2, 2, ...) and
    out = out_bytes_per_image (0: width * height) rounded up to 16."""
    out = up(out_bytes_per_image if out_bytes_per_image else width * height, 16)
    return up(3 * width * height) + up(4 * width * height) + up(2 * coef_count) + up(fdct_scratch) + up(out) + 256 + k17_scratch(out)


def chain(clouds, images, cam, T, dis, max_dt_ns, quality=95, first=0, stride=1, max_scans=0):
    """clouds: [(stamp, (n, 4) float32)] in topic order; images: [(stamp, pixels, encoding)] in topic order.
    -> [(record dict, jpeg bytes or None, (H, W, 3) picture or None)] per selected scan, what ilcc_bag_pcd2image_all_pairs hands its
    sink with keep_pixels (the record without `route`, which is not the specification's to say)."""
    picked = list(range(first, len(clouds), stride))
    if max_scans:
        picked = picked[:max_scans]
    image_ns = [paired_ref.stamp_ns(st) for st, _, _ in images]
    cloud_ns = [paired_ref.stamp_ns(clouds[i][0]) for i in picked]
    image_of, dt = paired_ref.pair_by_stamp(cloud_ns, image_ns, max_dt_ns)
    nearest, _ = paired_ref.pair_by_stamp(cloud_ns, image_ns, 2 ** 64)
    proj = paired_ref.projection(cam, T)
    bgr, out = {}, []
    for k, i in enumerate(picked):
        stamp, pts = clouds[i]
        j = image_of[k]
        rec = dict(message=i, stamp_sec=stamp[0], stamp_nsec=stamp[1], image_message=j,
                   image_stamp_sec=images[nearest[k]][0][0] if nearest[k] >= 0 else 0,
                   image_stamp_nsec=images[nearest[k]][0][1] if nearest[k] >= 0 else 0, dt_ns=dt[k], n_points=len(pts), n_drawn=0, file_bytes=0)
        blob = picture = None
        if j >= 0:
            if j not in bgr:
                bgr[j] = np.ascontiguousarray(paired_ref.image_to_bgr8(images[j][1], images[j][2], cam)).reshape(cam.height, 3 * cam.width)
            canvases, n = overlay_batch(pts, [0, len(pts)], [bgr[j]], [0], proj, dis)
            picture = canvases[0]
            blob = jpeg_write_ref.encode(picture, quality, (2, 2))
            rec["n_drawn"], rec["file_bytes"] = int(n[0]), len(blob)
        out.append((rec, blob, picture))
    return out
