"""Constructed inputs for include/ilcc_paired.h: stamp lists for the pairing, batches of scans for K8b, and the recording of the
chain tests.  Every builder is deterministic; no GPU is needed here.

  pairing_cases     ties, the max_dt boundary, unsorted stamps, one image for three clouds, no images, stamps near 2^32 s, and
                    2 000 random clouds x 1 500 images on a coarse grid (many ties and equal stamps)
  keep_batches      one batch per keep pattern: a scan of every length of project_cases.KEEP_N, so that wavefront, workgroup-pass
                    and chunk seams fall at scan boundaries and inside scans; empty and unpaired scans first, in the middle and
                    last; two images with different padded steps, each shared by several scans
  camera_batches    the cameras 1x1, 1x64, 64x1, 37x23 (and the shipped one) with their aimed clouds cut into scans
  many_chunks_*     more chunks than the scan workgroup has threads: 300 one-point scans and one of 3 * 4096 + 1; 1 030 chunks
  recording         7 clouds and 5 images (mono8, bgr8 with padded rows, rgb8, a Bayer encoding, bgr8) of a 64 x 48 camera"""
import functools

import numpy as np

import bayer_ref
import camera_image_ref as R
import project_cases as P
import rosbag_writer as W

CHUNK = P.CHUNK
SEC = 1000000000


# ------------------------------------------------------------------------------------------------------------------- pairing

def pairing_cases():
    """[(name, cloud_ns, image_ns, max_dt_ns)]"""
    rng = np.random.default_rng(2024)
    far = (2 ** 32 - 1) * SEC                                    # the last second a uint32 stamp can hold
    return [
        ("exact tie: the lower image wins", [200, 200], [300, 100, 300, 100], 1000),
        ("equal stamps: the lower image wins", [100, 90, 110], [500, 100, 100, 100], 1000),
        ("dt == max_dt accepted, one ns above rejected", [1000, 1000, 2000, 2000], [1050, 2051, 949, 1949], 50),
        ("dt == max_dt on the early side", [1000, 2000], [950, 1949], 50),
        ("max_dt 0: equal stamps only", [5, 6, 7], [7, 5], 0),
        ("unsorted on both sides", [900, 100, 500, 300, 700], [650, 50, 850, 250, 450], 60),
        ("one image serves three clouds", [1000, 1010, 990, 5000], [1001, 9000], 100),
        ("no images", [1, 2, 3], [], 10),
        ("no clouds", [], [1, 2, 3], 10),
        ("near 2^32 s: the subtraction does not wrap", [far + 5, far + 999999999, far - 3, 17], [far + 999999990, far, far + 7, 2 ** 63 + 11, 0],
         2 ** 62),
        ("near 2^32 s, tight limit", [far + 5, far + 999999999, far - 3], [far + 999999990, far, far + 7], 5),
        ("random 2000 x 1500", (rng.integers(0, 4000, 2000) * 7).tolist(), (rng.integers(0, 4000, 1500) * 7 + rng.integers(0, 2, 1500) * 3).tolist(), 9),
    ]


# ------------------------------------------------------------------------------------------------------------------- K8b batches

def _batch(name, scans, images, cam, dis):
    """scans: [(points (n, 4) float32, image index or -1)].  The points of an unpaired scan are replaced by NaN: K8b must not read
    them into the output."""
    parts, offsets, image_of = [], [0], []
    for pts, k in scans:
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        parts.append(np.full_like(pts, np.nan) if k < 0 else pts)
        offsets.append(offsets[-1] + len(pts))
        image_of.append(k)
    xyzi = np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)
    return dict(name=name, xyzi=xyzi, offsets=np.array(offsets, np.uint64), images=list(images), image_of_scan=np.array(image_of, np.int32),
                cam=cam, dis=dis)


def n_chunks(batch):
    """The chunks K8b cuts the batch into: 4096 points each, never across two scans, none for empty or unpaired scans."""
    n = np.diff(batch["offsets"].astype(np.int64))
    return int(sum((int(v) + CHUNK - 1) // CHUNK for v, k in zip(n, batch["image_of_scan"]) if k >= 0))


@functools.lru_cache(maxsize=None)
def keep_images():
    second = np.random.default_rng(129).integers(0, 256, (P.KEEP_SIDE, 3 * P.KEEP_SIDE + P.CAMERA_PAD), dtype=np.uint8)   # rows at odd addresses
    return [P.keep_image(), second]


N_KEEP_PATTERNS = max(len(P.keep_patterns(n)) for n in P.KEEP_N)
EMPTY = np.zeros((0, 4), np.float32)


def keep_batch(p):
    """Pattern p (modulo the number of patterns of each length) on a scan of every length of KEEP_N.  Pattern 0 is "none": a batch
    in which no point survives."""
    body = []
    for k, n in enumerate(P.KEEP_N):
        pats = P.keep_patterns(n)
        body.append((P.keep_cloud(pats[p % len(pats)][1]), k % 2))
        if k == 5:                                               # in the middle: an empty scan, an unpaired one, an empty unpaired one
            body += [(EMPTY, 1), (np.ones((CHUNK + 1, 4), np.float32), -1), (EMPTY, -1)]
    unpaired = (np.ones((100, 4), np.float32), -1)
    ends = [(EMPTY, 0), unpaired] if p % 2 == 0 else [unpaired, (EMPTY, 0)]      # empty first and last, or unpaired first and last
    return _batch("keep pattern %d" % p, ends + body + ends[::-1], keep_images(), P.keep_camera(), P.KEEP_DIS)


def camera_batches():
    out = []
    for name, cam, pts, tight, padded in P.camera_family():
        scans = [(pts[:700], 0), (pts[700:701], 1), (pts[701:], 1), (pts[:300], 0)]
        out.append(_batch("camera " + name, scans, [tight, padded], cam, P.CAMERA_DIS))
    return out


def _sliced(name, lengths, image_of):
    """One keep cloud over all points (structured mask: chunk ends, a walking lane, every third point), cut into scans."""
    total = int(sum(lengths))
    i = np.arange(total)
    cloud = P.keep_cloud(P.regrowth_mask(total) | (i % 3 == 0))
    scans, at = [], 0
    for n, k in zip(lengths, image_of):
        scans.append((cloud[at:at + n], k))
        at += n
    return _batch(name, scans, keep_images(), P.keep_camera(), P.KEEP_DIS)


def many_chunks_small():
    """300 one-point scans and one of 3 * 4096 + 1 points: 304 chunks, more than the 256 threads of the scan workgroup."""
    lengths = [1] * 150 + [3 * CHUNK + 1] + [1] * 150
    return _sliced("300 one-point scans + 3 * 4096 + 1", lengths, [k % 2 for k in range(len(lengths))])


def many_chunks_1030():
    """1 026 scans of 1 .. 5 points and two of 4097: 1 030 chunks, five passes of the scan workgroup."""
    lengths = [1 + k % 5 for k in range(1026)]
    lengths.insert(400, CHUNK + 1)
    lengths.append(CHUNK + 1)
    return _sliced("1030 chunks", lengths, [(k // 3) % 2 for k in range(len(lengths))])


# ------------------------------------------------------------------------------------------------------------------- the recording

IMAGE_TOPIC, LIDAR_TOPIC = "/camera/image_raw", "/velodyne_points"
IMG = (R.IMAGE_TYPE, R.IMAGE_MD5)
PC2 = ("sensor_msgs/PointCloud2", W.POINTCLOUD2_MD5)
COMPRESSED = ("sensor_msgs/CompressedImage", "8f7a12909da2c9d3332d540a0977563f")
MAX_DT_NS = 50 * 1000000
DISTANCE = 8.0
# lidar x forward, y left, z up -> camera z forward, x right, y down; a small offset
T_LIDAR2CAM = np.array([[0.0, -1.0, 0.0, 0.05], [0.0, 0.0, -1.0, -0.02], [1.0, 0.0, 0.0, 0.1], [0.0, 0.0, 0.0, 1.0]])


def recording_camera():
    return R.camera(40.0, 31.5, 38.0, 24.2, (-0.30, 0.10, 0.002, -0.0015, 0.05), 64, 48)


def _scene(n, seed):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-1.0, 9.0, n), rng.uniform(-4.0, 4.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(0, 255, n)], 1).astype(np.float32)
    pts[::97, 0] = np.nan
    pts[5::101, 1] = np.inf
    pts[7::89] = 0.0
    return pts


@functools.lru_cache(maxsize=None)
def recording():
    """-> (clouds [(stamp, points)], images [(stamp, pixels, encoding, step)]) in topic order.  Header stamps, in ms after 10 s:
    images 0, 100, 200, 300, 400; clouds 1 (image 0), 95 and 104 (both image 1: the shared image), 210 (image 2), 260 (image 3, 40 ms
    away), 700 (300 ms from image 4: beyond max_dt), 410 (image 4; its header stamp is earlier than the message before it)."""
    ms = 1000000
    rng = np.random.default_rng(7)
    w, h = 64, 48
    scene = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    images = [((10, 0), rng.integers(0, 256, (h, w), dtype=np.uint8), "mono8", None),
              ((10, 100 * ms), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "bgr8", 3 * w + 7),
              ((10, 200 * ms), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "rgb8", None),
              ((10, 300 * ms), bayer_ref.mosaic(scene, "bayer_rggb8"), "bayer_rggb8", w + 3),
              ((10, 400 * ms), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "bgr8", None)]
    stamps = [(10, 1 * ms), (10, 95 * ms), (10, 104 * ms), (10, 210 * ms), (10, 260 * ms), (10, 700 * ms), (10, 410 * ms)]
    sizes = [3000, 2500, 3100, 2200, 2900, 2300, 2700]
    clouds = [(stamps[k], _scene(sizes[k], 40 + k)) for k in range(7)]
    return clouds, images


def cloud_msg(stamp, pts, seq=0):
    a, fields, step = W.velodyne_points(np.array(pts))
    return W.pointcloud2(a, fields, step, seq=seq, stamp=stamp)


def write_recording(path, compression="none"):
    """One bag with both topics, messages interleaved in three chunks; record time k s for the k-th message of a topic."""
    clouds, images = recording()
    msgs = [(LIDAR_TOPIC, *PC2, (k + 1, 0), cloud_msg(st, pts, k)) for k, (st, pts) in enumerate(clouds)]
    msgs += [(IMAGE_TOPIC, *IMG, (k + 1, 500), R.image_msg(px, enc, step=step, seq=k, stamp=st)) for k, (st, px, enc, step) in enumerate(images)]
    msgs.sort(key=lambda m: m[3])
    bag = W.BagWriter(str(path), compression)
    for at in range(0, len(msgs), 5):
        bag.add_chunk(msgs[at:at + 5])
    bag.write()
    return bag


def cloud_data_bytes():
    return [32 * len(pts) for _, pts in recording()[0]]


def yaml_text(cam):
    K = [cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1]
    return ("%%YAML:1.0\n\nK: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [%s]\n"
            "d: !!opencv-matrix\n   rows: 5\n   cols: 1\n   dt: d\n   data: [%s]\n\nCamera.width: %d\nCamera.height: %d\n"
            % (", ".join(repr(float(v)) for v in K), ", ".join(repr(float(v)) for v in cam.d), cam.width, cam.height))
