"""LiDAR -> image projection: K8 vs the oracle's restatement of spaceToPlane /
HSVtoRGB / the pcd2image and rgblidar per-point loops, bit for bit (integer pixels, bytes, float bits)."""
import os
import re

import numpy as np
import pytest

from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import project, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CAM = (1061.37439737547, 980.706836288949, 1061.02435228316, 601.685030610243)   # pointgrey.yaml
SIZE = (1920, 1200)


def _camera():
    T = np.fromfile(os.path.join(GOLD, "pointgrey.bin"), dtype=np.float64).reshape(4, 4, order="F")   # the shipped extrinsic
    return project.Projection.from_extrinsic(T, CAM, SIZE), T


def test_project_exports_and_struct():
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "ilcc_project.h")).read()
    body = header[header.index('extern "C"'):]
    declared = set(re.findall(r"\b(ilcc_[a-z0-9_]+)\s*\(", body))
    assert declared == set(project.PROJECT_EXPORTS)
    for name in declared:
        assert hasattr(N.lib(), name)
    assert C.sizeof(project.Projection) == 8 * 16 + 8 and project.HIT_DTYPE.itemsize == 16


def test_oracle_hsv_known_answers(ob):
    # hand-evaluated from HSVtoRGB (ImageCornersEst.cpp:373-428) with s = v = 100: max 255, min 0, adj = 255*difs/60
    assert ob.hsv_to_rgb(0) == (255, 0, 0)
    assert ob.hsv_to_rgb(30) == (255, 127, 0)          # 255*30/60 = 127.5 -> 127
    assert ob.hsv_to_rgb(60) == (255, 255, 0)
    assert ob.hsv_to_rgb(90) == (127, 255, 0)
    assert ob.hsv_to_rgb(120) == (0, 255, 0)
    assert ob.hsv_to_rgb(200) == (0, 170, 255)          # i = 3, difs 20: 255 - 85
    assert ob.hsv_to_rgb(255) == (63, 0, 255)           # i = 4, difs 15: 63.75 -> 63
    assert ob.hsv_to_rgb(359) == (255, 0, 4)            # default branch, difs 59: 255 - 250.75
    assert ob.hsv_to_rgb(425) == (255, 0, 233)          # h > 360 (intensity 100): i = 7 -> default, difs 5


def test_oracle_projection_of_shipped_corners(ob):
    """The shipped LiDAR corners projected with the shipped extrinsic land on the shipped camera corners
    (reprojection ~2 px): pins spaceToPlane's conventions (R, t, fx/cx order) against the reference's data."""
    cam, _ = _camera()
    from lidar_camera_calibration_amd import calib
    tot = []
    for i in range(1, 7):
        p3 = np.loadtxt(os.path.join(GOLD, f"pointgrey_lidar_{i}.txt"), dtype=np.float32)
        p2 = calib.read_cam_corners(os.path.join(GOLD, f"pointgrey{i}.txt"), 35)
        hits = ob.project_intensity(np.concatenate([p3, np.full((35, 1), 30, np.float32)], 1), cam)
        assert len(hits) == 35 and np.array_equal(hits["index"], np.arange(35))
        px = np.stack([hits["x"], hits["y"]], 1).astype(float) + 0.5
        # nearest camera corner (file order differs between sensors before check_order)
        d = np.linalg.norm(px[:, None] - p2[None], axis=2).min(1)
        tot.append(d)
        assert tuple(hits[0][["r", "g", "b"]]) == ob.hsv_to_rgb(int(30 / 60 * 255))
    tot = np.concatenate(tot)
    assert tot.max() < 10.0 and tot.mean() < 3.0      # the reference's own fit leaves ~2 px mean (robust loss, 7.7 px worst corner)


def _scene(n, seed):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-20, 20, (n, 3)), rng.uniform(0, 255, (n, 1))], 1).astype(np.float32)
    pts[:, 2] = rng.uniform(-2, 3, n)
    pts[::97, 0] = np.nan
    pts[5::101, 1] = np.inf
    pts[7::89] = 0.0                       # P_c.z near t.z: exercises the depth gate
    pts[11::113, 3] = np.nan               # NaN intensity -> x86 "integer indefinite" hue
    pts[13::127, 3] = -5.0
    return pts


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 4096, 4097, 131072])
def test_k8_project_intensity_bit_exact(ob, n):
    import torch
    cam, _ = _camera()
    pts = _scene(n, n)
    want = ob.project_intensity(pts, cam, 30.0)
    d_pts = torch.from_numpy(pts).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    m = project.project_intensity_device(d_pts.data_ptr(), n, cam, d_hits.data_ptr(), 30.0)
    got = d_hits.cpu().numpy().view(project.HIT_DTYPE).reshape(-1)[:m]
    assert m == len(want)
    assert got.tobytes() == want.tobytes()
    if n > 1000:
        assert 0 < m < n


@pytest.mark.gpu
def test_k8_colourise_bit_exact(ob):
    import torch
    cam, _ = _camera()
    rng = np.random.default_rng(3)
    n = 60000
    pts = _scene(n, 9)
    img = rng.integers(0, 256, (SIZE[1], SIZE[0] * 3 + 16), dtype=np.uint8)      # padded rows
    want = ob.colourise(pts, cam, img, 30.0)
    d_pts = torch.from_numpy(pts).cuda()
    d_img = torch.from_numpy(img).cuda()
    d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    m = project.colourise_device(d_pts.data_ptr(), n, cam, d_img.data_ptr(), img.strides[0], d_out.data_ptr(), 30.0)
    got = d_out.cpu().numpy()[:m]
    assert m == len(want) and m > 1000
    assert got.tobytes() == want.tobytes()
    with pytest.raises(RuntimeError):
        project.colourise_device(d_pts.data_ptr(), n, cam, d_img.data_ptr(), 100, d_out.data_ptr(), 30.0)


@pytest.mark.gpu
def test_k8_throughput_report():
    import torch
    cam, _ = _camera()
    n = 128 * 28800
    lidar = synth.vlp16()
    clouds, _, _, _ = synth.make_batch(4, lidar, synth.Board(), seed=1)
    pts = np.tile(clouds.reshape(-1, 4), (32, 1))[:n]
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        m = project.project_intensity_device(d_pts.data_ptr(), n, cam, d_hits.data_ptr(), 50.0, stream=s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        project.project_intensity_device(d_pts.data_ptr(), n, cam, d_hits.data_ptr(), 50.0, stream=s)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    gb = (16 * n + 16 * m) / 1e9
    print("K8 project: %.3f ms per %d points (%d hits), %.0f GB/s algorithmic (16 B read/pt + 16 B/hit)"
          % (ms, n, m, gb / ms * 1e3))
    assert m > 0
