"""`ilcc_corners --bag ... --all-scans` (pytest -m gpu): the fused corners in the reference's <camera>_lidar_<n>.txt format, the
per-scan report, and the unchanged behaviour without the switch."""
import os
import subprocess

import numpy as np
import pytest

import sequence_cases as K
from lidar_camera_calibration_amd import LidarCornersBatch, read_lidar_corners, save_corners2txt, sequence
from lidar_camera_calibration_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_corners")


def test_cli_all_scans_writes_the_fused_corners_and_a_report(tmp_path):
    assert os.path.exists(CLI), "build() makes lidar_camera_calibration_amd/ilcc_corners"
    bag = str(tmp_path / "pose0.bag")
    clouds = K.write_sequence_bag(bag)
    click = K.sequence(0)[1]
    est = LidarCornersBatch(16, max(len(c) for c in clouds))
    res, scans = sequence.bag_corners_all_scans(est, bag, K.TOPIC, click)
    est.close()
    assert res.status == N.OK

    out, report = tmp_path / "pointgrey_lidar_1.txt", tmp_path / "report.txt"
    argv = [CLI, "--bag", bag, "--click", *("%.9g" % v for v in click), "--out", str(out)]
    r = subprocess.run(argv + ["--all-scans", "--report", str(report)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "add_corner" in r.stdout
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith("all scans:")]
    assert len(summary) == 1
    f = dict(zip(summary[0].split()[2::2], summary[0].split()[3::2]))
    assert (int(f["status"]), int(f["scans"]), int(f["accepted"]), int(f["used"]), int(f["ref_scan"]), int(f["corners"])) == \
        (N.OK, res.n_scans, res.n_ok, res.n_used, res.ref_scan, res.n_corners)
    assert abs(float(f["spread_rms_mm"]) - res.spread_rms * 1e3) < 1e-3 and abs(float(f["spread_max_mm"]) - res.spread_max * 1e3) < 1e-3
    # the file: what save_corners2txt writes for the fused corners, and what the consumer's reader takes back at the format's precision
    save_corners2txt(res.corners_array(), str(tmp_path / "py.txt"))
    assert out.read_bytes() == (tmp_path / "py.txt").read_bytes()
    back = read_lidar_corners(str(out), res.n_corners)
    assert back.shape == (res.n_corners, 3) and np.allclose(back, res.corners_array(), rtol=5e-6, atol=0)    # 6 significant digits
    # the report: one line per scan
    lines = report.read_text().splitlines()
    assert len(lines) == res.n_scans == 14
    for k, ln in enumerate(lines):
        g = dict(zip(ln.split()[0::2], ln.split()[1::2]))
        assert (int(g["scan"]), int(g["message"]), int(g["status"]), int(g["flags"]), int(g["used"])) == \
            (k, scans[k].message, scans[k].result.status, scans[k].result.flags, scans[k].used)
        assert g["stamp"] == "%d.%09d" % (scans[k].stamp_sec, scans[k].stamp_nsec)
        assert abs(float(g["distance_mm"]) - (scans[k].distance * 1e3 if scans[k].distance >= 0 else -1.0)) < 1e-3
    # selection switches reach the chain
    r = subprocess.run(argv + ["--all-scans", "--first", "2", "--stride", "3", "--max-scans", "3", "--gate", "0.05", "--report", str(report)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [int(ln.split()[3]) for ln in report.read_text().splitlines()] == [2, 5, 8]

    # without --all-scans: the first cloud alone, as before -- the same bytes as the same cloud given as a raw file
    raw = tmp_path / "frame.bin"
    clouds[0].tofile(raw)
    first, single = tmp_path / "first.txt", tmp_path / "single.txt"
    for src, dst in ((["--bag", bag], first), (["--cloud", str(raw)], single)):
        r = subprocess.run([CLI, *src, "--click", *("%.9g" % v for v in click), "--out", str(dst)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "all scans:" not in r.stdout
    assert first.read_bytes() == single.read_bytes() and first.read_bytes() != out.read_bytes()


def test_cli_all_scans_needs_a_bag(tmp_path):
    r = subprocess.run([CLI, "--cloud", str(tmp_path / "x.bin"), "--click", "0", "0", "0", "--out", str(tmp_path / "o.txt"), "--all-scans"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--all-scans needs --bag" in r.stderr
