"""numpy restatement of include/ilcc_paired.h: the pairing of clouds and images by header stamp (brute force, python ints), the
bytes of the binary PCD file, the batched colourise as a loop of project_cases.colourise over the scans, and the chain
(overlay_ref's / bayer_ref's conversion to B,G,R and undistortion, then the above).  No GPU is needed here.

Neither message_filters::ApproximateTime nor PCL is available to the tests, so -- as camera_image_ref.py for K11 -- this file IS
the specification of the pairing rule and of the PCD header.

  pairing   for cloud i, j = the image with the least |image_ns[j] - cloud_ns[i]|, a tie going to the lower j;
            |dt| <= max_dt_ns: image_of[i] = j, else -1; dt_ns[i] = image - cloud of that nearest image (0 without images)."""
import numpy as np

import bayer_ref
import overlay_ref
import project_cases
from lidar_camera_calibration_amd import project

PCD_HEADER = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
              "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n")


def stamp_ns(stamp):
    return int(stamp[0]) * 1000000000 + int(stamp[1])


def pair_by_stamp(cloud_ns, image_ns, max_dt_ns):
    """-> (image_of, dt_ns): python lists of ints; O(n m), on purpose."""
    image_of, dt = [], []
    for c in (int(v) for v in cloud_ns):
        best = None
        for j, m in enumerate(int(v) for v in image_ns):
            if best is None or abs(m - c) < abs(best[1]):            # strict: a tie stays with the lower j
                best = (j, m - c)
        if best is None:
            image_of.append(-1)
            dt.append(0)
        else:
            image_of.append(best[0] if abs(best[1]) <= int(max_dt_ns) else -1)
            dt.append(best[1])
    return image_of, dt


MAX_BATCH_POINTS = 2 ** 32 - 2


class CutRefused(Exception):
    """kind: "CAPACITY" or "BAD_ARGUMENT"."""
    def __init__(self, kind):
        Exception.__init__(self, kind)
        self.kind = kind


def cut_paired(scans, image_raw, bgr_bytes, staging, image, device=0, per_member=0, member_cap=0, stage_unpaired=False):
    """The batch cut of the paired chains (csrc/paired_cut.h), restated from the two loops the chains had.
    scans: [(data_bytes, points, pair)] per selected scan, pair -1 for an unpaired one; image_raw[j], bgr_bytes: multiples of 256.
    stage_unpaired: ilcc_bag_rgblidar_all_scans stages and unpacks every scan; ilcc_bag_pcd2image_all_pairs (False) counts an unpaired
    scan's data[] against `staging` but neither stages it nor counts its points, and has the device budget and the member cap.
    -> (batches, largest): a batch is a dict(first_scan, scans, members, blob_bytes, points, raw_bytes, bgr_bytes,
    images=[(image, raw_at, bgr_at)]); largest a dict of the maxima.  Raises CutRefused."""
    up16 = lambda v: (v + 15) // 16 * 16
    if device and per_member > device:
        raise CutRefused("CAPACITY")
    batches, s = [], 0
    while s < len(scans):
        first, members, blob, points, counted, seen = s, [], 0, 0, 0, []
        while s < len(scans):
            data, pts, j = scans[s]
            member = stage_unpaired or j >= 0
            new_image = j >= 0 and j not in seen
            extra = image_raw[j] + bgr_bytes if new_image else 0
            if data > staging or extra > image:
                raise CutRefused("CAPACITY")
            if member and points + pts > MAX_BATCH_POINTS:
                if not members:
                    raise CutRefused("BAD_ARGUMENT")
                break
            cost = sum(image_raw[i] + bgr_bytes for i in seen)
            full = member and ((device and (len(members) + 1) * per_member > device) or (member_cap and len(members) >= member_cap))
            if s > first and (up16(counted) + data > staging or cost + extra > image or full):
                break
            counted = up16(counted) + data
            if member:
                blob = up16(blob) + data
                points += pts
                members.append(s)
            if new_image:
                seen.append(j)
            s += 1
        b = dict(first_scan=first, scans=s - first, members=members, blob_bytes=blob, points=points, raw_bytes=0, bgr_bytes=0, images=[])
        for j in seen:                                           # an image shared with another batch is charged to both
            b["images"].append((j, b["raw_bytes"], b["bgr_bytes"]))
            b["raw_bytes"] += image_raw[j]
            b["bgr_bytes"] += bgr_bytes
        batches.append(b)
    largest = dict(members=max(len(b["members"]) for b in batches) if batches else 0)
    for key in ("blob_bytes", "points", "raw_bytes", "bgr_bytes"):
        largest[key] = max((b[key] for b in batches), default=0)
    return batches, largest


def pcd_bytes(xyzrgb):
    """The file ilcc_save_pcd_xyzrgb writes for (n, 4) float32 records."""
    a = np.ascontiguousarray(xyzrgb, dtype=np.float32).reshape(-1, 4)
    return (PCD_HEADER % (len(a), len(a))).encode() + a.tobytes()


def read_pcd(path):
    """(n, 4) float32 records of a file pcd_bytes describes; asserts the header."""
    blob = open(path, "rb").read()
    head, sep, body = blob.partition(b"DATA binary\n")
    assert sep, blob[:200]
    n = int(head.split(b"POINTS ")[1].split(b"\n")[0])
    assert blob[:len(head) + len(sep)] == (PCD_HEADER % (n, n)).encode() and len(body) == 16 * n
    return np.frombuffer(body, np.float32).reshape(n, 4)


def colourise_batch(xyzi, offsets, images, image_of_scan, cam, dis):
    """K8b: xyzi (N, 4) float32, offsets [n + 1], images: list of uint8 (rows, step) B,G,R, image_of_scan [n] (-1: none).
    -> (records (M, 4) float32, out_offsets [n + 1])."""
    parts, out_offsets = [], [0]
    for s, k in enumerate(image_of_scan):
        pts = xyzi[int(offsets[s]):int(offsets[s + 1])]
        rec = project_cases.colourise(pts, cam, images[k], dis) if k >= 0 and len(pts) else np.zeros((0, 4), np.float32)
        parts.append(rec)
        out_offsets.append(out_offsets[-1] + len(rec))
    return (np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)), np.array(out_offsets, np.uint64)


def image_to_bgr8(pixels, encoding, cam=None):
    """K11c of any encoding the chain takes: (H, W, 3) B,G,R, undistorted when a camera (camera_image_ref.Camera) is given."""
    if encoding in bayer_ref.BAYER_ENCODINGS:
        return bayer_ref.to_bgr8(pixels, encoding, cam)
    return overlay_ref.convert_bgr8(pixels, encoding, cam)


def projection(cam, T):
    """K8's camera of the lens `cam` (camera_image_ref.Camera) and the 4 x 4 extrinsic."""
    return project.Projection.from_extrinsic(np.asarray(T, np.float64), (cam.fx, cam.cx, cam.fy, cam.cy), (cam.width, cam.height))


def chain(clouds, images, cam, T, dis, max_dt_ns, sample_raw=False, first=0, stride=1, max_scans=0):
    """clouds: [(stamp, (n, 4) float32)] in topic order; images: [(stamp, pixels, encoding)] in topic order.
    -> [(record dict, (m, 4) float32)] per selected scan, what ilcc_bag_rgblidar_all_scans hands its sink."""
    picked = list(range(first, len(clouds), stride))
    if max_scans:
        picked = picked[:max_scans]
    image_ns = [stamp_ns(st) for st, _, _ in images]
    image_of, dt = pair_by_stamp([stamp_ns(clouds[i][0]) for i in picked], image_ns, max_dt_ns)
    nearest, _ = pair_by_stamp([stamp_ns(clouds[i][0]) for i in picked], image_ns, 2 ** 64)
    proj = projection(cam, T)
    bgr = {}
    out = []
    for k, i in enumerate(picked):
        stamp, pts = clouds[i]
        j = image_of[k]
        rec = dict(message=i, stamp_sec=stamp[0], stamp_nsec=stamp[1], image_message=j,
                   image_stamp_sec=images[nearest[k]][0][0] if nearest[k] >= 0 else 0,
                   image_stamp_nsec=images[nearest[k]][0][1] if nearest[k] >= 0 else 0, dt_ns=dt[k], n_points=len(pts))
        cloud = np.zeros((0, 4), np.float32)
        if j >= 0:
            if j not in bgr:
                px = image_to_bgr8(images[j][1], images[j][2], None if sample_raw else cam)
                bgr[j] = np.ascontiguousarray(px).reshape(cam.height, 3 * cam.width)
            if len(pts):
                cloud = project_cases.colourise(pts, proj, bgr[j], dis)
        rec["n_coloured"] = len(cloud)
        out.append((rec, cloud))
    return out
