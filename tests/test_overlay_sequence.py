"""Every scan of a batch drawn on a copy of its image, on the GPU (include/ilcc_overlay_sequence.h): K12b byte for byte against the
numpy specification in overlay_sequence_ref.py and, scan by scan, against the single-scan entries on the device (a copy of the image,
ilcc_project_intensity_device, ilcc_draw_hits_device); its canvas layout, launch counts, refusals and stream contract; and the chain
from a bag -- library entry, python mirror and the ilcc_pcd2image --all-pairs program -- against overlay_sequence_ref.chain.  The
inputs are paired_cases.py's batches and recording, and overlay_sequence_cases.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import overlay_sequence_cases as OC
import overlay_sequence_ref as R
import paired_cases as K
import project_cases as P
import stream_contract as SC
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import calib, overlay, project
from lidar_camera_calibration_amd import camera_image as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lidar_camera_calibration_amd", "ilcc_pcd2image")
FILL = 0xAB
TAIL = 64                                       # bytes of FILL behind the last canvas
LO, HI = 0.0, 60.0


class OnDevice:
    """A batch on the device: cloud, images, a canvas array of FILL bytes with TAIL bytes of slack, and a scratch of 0xCD bytes."""

    def __init__(self, b, stride_extra=0, pitch_slack=0, stamp=None):
        import torch
        self.b, self.stamp = b, stamp
        self.cam = b["cam"]
        self.w, self.h = self.cam.width, self.cam.height
        self.n_scans = len(b["image_of_scan"])
        self.xyzi = torch.from_numpy(np.ascontiguousarray(b["xyzi"]).view(np.uint8).reshape(-1).copy()).cuda() if len(b["xyzi"]) else \
            torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.images = [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in b["images"]]
        self.stride = 3 * self.w + stride_extra
        self.pitch = self.stride * (self.h - 1) + 3 * self.w + pitch_slack
        self.total = self.pitch * self.n_scans + TAIL
        self.canvas = torch.full((self.total,), FILL, dtype=torch.uint8, device="cuda")
        self.scratch_bytes = overlay.overlay_batch_scratch_bytes(self.w, self.h, self.n_scans)
        self.scratch = torch.full((max(16, self.scratch_bytes),), 0xCD, dtype=torch.uint8, device="cuda")

    def run(self, plan, **kw):
        b = self.b
        overlay.overlay_batch_device(self.xyzi.data_ptr(), b["offsets"], [im.data_ptr() for im in self.images], [im.shape[1] for im in b["images"]],
                                     b["image_of_scan"], self.cam, self.canvas.data_ptr(), self.stride, self.pitch, self.scratch.data_ptr(),
                                     self.scratch_bytes, plan, distance_valid=b["dis"], inten_low=LO, inten_high=HI, stamp=self.stamp, **kw)
        return plan.finish(self.n_scans)

    def bytes(self):
        return self.canvas.cpu().numpy()

    def want(self):
        b = self.b
        return R.overlay_batch(b["xyzi"], b["offsets"], b["images"], b["image_of_scan"], self.cam, b["dis"], LO, HI,
                               self.stamp if self.stamp is not None else R.REFERENCE_STAMP)


def _check_against_the_specification(dev, n_drawn):
    """Every byte of the array: the drawn rows where the contract puts them, FILL between them, behind them and in unpaired canvases."""
    canvases, want_n = dev.want()
    assert n_drawn.tolist() == want_n.tolist(), dev.b["name"]
    want = R.canvas_bytes(canvases, dev.cam, dev.stride, dev.pitch, dev.total, FILL)
    got = dev.bytes()
    assert got.tobytes() == want.tobytes(), (dev.b["name"], int((got != want).sum()))
    return canvases, want_n


def _check_against_the_single_entries(dev, n_drawn):
    """copy of the image -> ilcc_project_intensity_device -> ilcc_draw_hits_device on every paired scan alone: the same rows"""
    import torch
    b, w, h = dev.b, dev.w, dev.h
    got = dev.bytes()
    longest = max(1, int(np.diff(b["offsets"].astype(np.int64)).max(initial=0)))
    hits = torch.zeros(16 * longest, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(project.draw_hits_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    for s, k in enumerate(b["image_of_scan"]):
        if k < 0:
            assert n_drawn[s] == 0
            continue
        lo, hi = int(b["offsets"][s]), int(b["offsets"][s + 1])
        alone = dev.images[k][:, :3 * w].clone(memory_format=torch.contiguous_format)
        m = project.project_intensity_device(dev.xyzi.data_ptr() + 16 * lo, hi - lo, dev.cam, hits.data_ptr(), b["dis"], LO, HI)
        project.draw_hits_device(alone.data_ptr(), w, h, 3 * w, hits.data_ptr(), m, scratch.data_ptr(), stamp=dev.stamp)
        torch.cuda.synchronize()
        assert m == int(n_drawn[s]), (b["name"], s)
        rows = np.lib.stride_tricks.as_strided(got[s * dev.pitch:], (h, 3 * w), (dev.stride, 1))
        assert rows.tobytes() == alone.cpu().numpy().tobytes(), (b["name"], s)


@pytest.fixture(scope="module")
def plan():
    p = overlay.OverlayPlan(1100, 80000)
    yield p
    p.close()


# ------------------------------------------------------------------------------------------ K12b against both references

@pytest.mark.gpu
@pytest.mark.parametrize("p", range(K.N_KEEP_PATTERNS))
def test_k12b_keep_patterns_at_every_seam(plan, p):
    dev = OnDevice(K.keep_batch(p), stride_extra=p % 3, pitch_slack=5 * (p % 2))
    n_drawn = dev.run(plan)
    assert plan.launches == 3
    canvases, _ = _check_against_the_specification(dev, n_drawn)
    _check_against_the_single_entries(dev, n_drawn)
    b = dev.b
    for s, k in enumerate(b["image_of_scan"]):                                 # an empty paired scan: a plain copy of its image
        if k >= 0 and b["offsets"][s] == b["offsets"][s + 1]:
            assert canvases[s].tobytes() == R.packed(b["images"][k], dev.cam).tobytes() and n_drawn[s] == 0
    assert (p == 0) == (int(n_drawn.sum()) == 0)


@pytest.mark.gpu
def test_k12b_cameras_clip_the_stamp_at_all_four_borders(plan):
    for b in K.camera_batches():
        dev = OnDevice(b, stride_extra=1)
        n_drawn = dev.run(plan)
        assert plan.launches == 3
        canvases, want_n = _check_against_the_specification(dev, n_drawn)
        _check_against_the_single_entries(dev, n_drawn)
        assert 0 < int(want_n.sum()) < len(b["xyzi"]), b["name"]
    # the small cameras do have hits whose stamp leaves the image on every side
    for name, cam, pts, _, _ in P.camera_family():
        if name != "37x23 inside":
            continue
        hits = P.project_intensity(pts, cam, P.CAMERA_DIS)
        assert (hits["x"] == 0).any() and (hits["x"] == cam.width - 1).any() and (hits["y"] == 0).any() and (hits["y"] == cam.height - 1).any(), name


@pytest.mark.gpu
def test_k12b_collisions():
    dev = OnDevice(OC.collision_batch(), stride_extra=13, pitch_slack=3)
    plan = overlay.OverlayPlan(4, len(dev.b["xyzi"]))
    n_drawn = dev.run(plan)
    assert plan.launches == 3 and n_drawn.tolist() == [OC.N_ONE_PIXEL, 400, 150, 150]
    canvases, _ = _check_against_the_specification(dev, n_drawn)
    _check_against_the_single_entries(dev, n_drawn)
    # one pixel, two chunks: the colour of the LAST point, which is not its neighbours' nor the first chunk's last
    pts = OC.one_pixel_scan()
    colour = lambda i: P.hsv_to_rgb(P.hue_of(pts[i:i + 1, 3], LO, HI))[0].tolist()
    x, y = OC.ONE_PIXEL
    assert canvases[0][y, x].tolist() == colour(len(pts) - 1)
    assert colour(len(pts) - 1) not in (colour(len(pts) - 2), colour(P.CHUNK - 1), colour(P.CHUNK), colour(0))
    # two scans on one image: each canvas shows its own dots only
    assert canvases[2].tobytes() != canvases[3].tobytes()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("make", [K.many_chunks_small, K.many_chunks_1030], ids=["304 chunks", "1030 chunks"])
def test_k12b_more_chunks_than_a_workgroup_has_threads(plan, make):
    dev = OnDevice(make())
    n_drawn = dev.run(plan)
    assert plan.launches == 3                                                  # however many scans and chunks
    _, want_n = _check_against_the_specification(dev, n_drawn)
    assert 0 < int(want_n.sum()) < len(dev.b["xyzi"])


@pytest.mark.gpu
def test_k12b_three_hundred_scans_of_a_few_points(plan):
    dev = OnDevice(OC.hundreds(), stride_extra=1, pitch_slack=2)
    n_drawn = dev.run(plan)
    assert plan.launches == 3 and dev.n_scans == 300
    _, want_n = _check_against_the_specification(dev, n_drawn)
    _check_against_the_single_entries(dev, n_drawn)
    assert int((want_n > 0).sum()) > 30 and (dev.b["image_of_scan"] < 0).sum() > 10


@pytest.mark.gpu
@pytest.mark.parametrize("extra, slack", [(0, 0), (1, 0), (13, 0), (0, 7), (13, 29)])
def test_k12b_canvas_layout(plan, extra, slack):
    dev = OnDevice(K.keep_batch(1), stride_extra=extra, pitch_slack=slack)
    n_drawn = dev.run(plan)
    _check_against_the_specification(dev, n_drawn)                              # which holds every byte outside the contract to FILL
    got = dev.bytes()
    for s in np.flatnonzero(dev.b["image_of_scan"] < 0):
        assert (got[s * dev.pitch:(s + 1) * dev.pitch] == FILL).all()
    assert (got[dev.n_scans * dev.pitch:] == FILL).all()


@pytest.mark.gpu
def test_k12b_stamp_of_64_offsets_and_the_null_stamp(plan):
    b = K.camera_batches()[6]                                                   # 37 x 23, principal point inside
    assert "37x23 inside" in b["name"]
    for stamp in (OC.stamp_of_64(), None, [(0, 0)], [(-128, 127)]):
        dev = OnDevice(b, stride_extra=2, stamp=stamp)
        n_drawn = dev.run(plan)
        _check_against_the_specification(dev, n_drawn)
        _check_against_the_single_entries(dev, n_drawn)
    coll = OnDevice(OC.collision_batch(), stamp=OC.stamp_of_64())
    _check_against_the_specification(coll, coll.run(plan))


# ------------------------------------------------------------------------------------------ launches, reuse, refusals

@pytest.mark.gpu
def test_k12b_launch_counts_and_plan_reuse(plan):
    import torch
    big = OnDevice(K.many_chunks_1030())
    big.run(plan)
    assert plan.launches == 3
    small = OnDevice(K.keep_batch(3))                                           # nothing of the larger table or its counts shows
    _check_against_the_specification(small, small.run(plan))
    keep = K.keep_batch(1)
    n = len(keep["image_of_scan"])
    empty = dict(keep, name="all empty", xyzi=np.zeros((0, 4), np.float32), offsets=np.zeros(n + 1, np.uint64))
    unpaired = dict(keep, name="all unpaired", image_of_scan=np.full(n, -1, np.int32))
    none = dict(keep, name="no scans", xyzi=np.zeros((0, 4), np.float32), offsets=np.zeros(1, np.uint64), image_of_scan=np.zeros(0, np.int32))
    for b, launches in ((empty, 1), (unpaired, 0), (none, 0)):
        dev = OnDevice(b)
        n_drawn = dev.run(plan)
        assert plan.launches == launches and n_drawn.tolist() == [0] * len(b["image_of_scan"]), b["name"]
        torch.cuda.synchronize()
        canvases, _ = _check_against_the_specification(dev, n_drawn)            # all empty: every paired canvas is its image
        if launches == 0:
            assert (dev.bytes() == FILL).all() and (dev.scratch.cpu().numpy() == 0xCD).all(), b["name"]
        else:
            assert sum(c is not None for c in canvases) > 10
    _check_against_the_specification(small, small.run(plan))                    # and the plan still works
    assert plan.launches == 3
    s = torch.cuda.Stream()
    again = OnDevice(K.keep_batch(5))
    torch.cuda.synchronize()
    _check_against_the_specification(again, again.run(plan, stream=s.cuda_stream))


@pytest.mark.gpu
def test_k12b_refusals_leave_canvas_and_scratch_untouched():
    import torch
    L = overlay.lib()
    b = K.keep_batch(2)
    dev = OnDevice(b, stride_extra=1, pitch_slack=4)
    n = dev.n_scans
    plan = overlay.OverlayPlan(n, len(b["xyzi"]))
    steps = [im.shape[1] for im in b["images"]]
    ptrs = [im.data_ptr() for im in dev.images]

    def call(xyzi=dev.xyzi.data_ptr(), offsets=b["offsets"], images=ptrs, image_steps=steps, image_of=b["image_of_scan"], cam=dev.cam, canvas=dev.canvas.data_ptr(),
             stride=dev.stride, pitch=dev.pitch, scratch=dev.scratch.data_ptr(), scratch_bytes=dev.scratch_bytes, pl=plan, stamp=None, null=(), n_stamp=None):
        job, keep = overlay.overlay_batch_job(xyzi, offsets, images, image_steps, image_of, cam, canvas, stride, pitch, scratch, scratch_bytes, pl, b["dis"], LO, HI, stamp)
        for field in null:
            setattr(job, field, None)
        if n_stamp is not None:
            job.n_stamp = n_stamp
        return L.ilcc_overlay_batch_device(C.byref(job))

    decreasing = b["offsets"].copy()
    assert decreasing[4] > 0
    decreasing[5] = decreasing[4] - 1
    outside, below = b["image_of_scan"].copy(), b["image_of_scan"].copy()
    outside[4], below[4] = 2, -2
    small_plan = overlay.OverlayPlan(n - 1, len(b["xyzi"]))
    few_points = overlay.OverlayPlan(n, len(b["xyzi"]) - 1)
    side = P.KEEP_SIDE
    bad = [dict(pl=None), dict(null=["cam"]), dict(null=["offsets"]), dict(null=["image_of_scan"]), dict(null=["d_images_bgr"]), dict(null=["image_steps"]),
           dict(xyzi=None), dict(canvas=None), dict(scratch=None), dict(images=[ptrs[0], None]), dict(pl=small_plan), dict(pl=few_points),
           dict(offsets=decreasing), dict(image_of=outside), dict(image_of=below), dict(image_steps=[3 * side - 1, steps[1]]), dict(image_steps=[steps[0], 3 * side - 1]),
           dict(cam=P.camera(width=0, height=side)), dict(cam=P.camera(width=side, height=0)), dict(cam=P.camera(width=-4, height=4)),
           dict(cam=P.camera(width=65537, height=1)), dict(offsets=np.array([0, 2 ** 32 - 1], np.uint64), image_of=[0]),
           dict(stamp=[(0, 0)], n_stamp=0), dict(stamp=[(0, 0)], n_stamp=65), dict(stamp=[(0, 0)], n_stamp=-1),
           dict(stride=3 * side - 1), dict(pitch=dev.stride * (side - 1) + 3 * side - 1), dict(scratch_bytes=dev.scratch_bytes - 1), dict(scratch_bytes=0),
           dict(scratch=dev.scratch.data_ptr() + 4), dict(scratch=dev.scratch.data_ptr() + 8)]
    for kw in bad:
        N.lib().ilcc_last_error(None)
        assert call(**kw) == N.BAD_ARGUMENT, list(kw)
        assert b"overlay batch" in N.lib().ilcc_last_error(None), list(kw)
    assert L.ilcc_overlay_batch_device(None) == N.BAD_ARGUMENT
    out = (C.c_uint32 * n)()
    assert L.ilcc_overlay_plan_finish(plan._p, out) == N.BAD_ARGUMENT          # no call was accepted: there is nothing to finish
    assert L.ilcc_overlay_plan_finish(None, out) == N.BAD_ARGUMENT and L.ilcc_overlay_plan_finish(plan._p, None) == N.BAD_ARGUMENT
    assert plan.launches == 0
    torch.cuda.synchronize()
    assert (dev.bytes() == FILL).all() and (dev.scratch.cpu().numpy() == 0xCD).all()       # nothing was launched
    assert not L.ilcc_overlay_plan_create(0, 10) and not L.ilcc_overlay_plan_create(10, 0) and not L.ilcc_overlay_plan_create(1, 2 ** 32 - 1)
    assert not L.ilcc_overlay_plan_create(65536, 10)
    assert overlay.overlay_batch_scratch_bytes(0, 4, 1) == overlay.overlay_batch_scratch_bytes(4, 65537, 1) == 0
    assert overlay.overlay_batch_scratch_bytes(3, 3, 5) == 5 * 48 and overlay.overlay_batch_scratch_bytes(1920, 1200, 2) == 2 * 4 * 1920 * 1200
    # the same arguments, accepted: a stride, pitch and scratch of exactly what is needed are enough
    assert call() == N.OK and plan.launches == 3
    _check_against_the_specification(dev, plan.finish(n))
    for p in (plan, small_plan, few_points):
        p.close()


# ------------------------------------------------------------------------------------------ the stream contract

class OverlayBatch:
    """A keep_batch as K12b takes it, and its decoy: another keep pattern on the same scan lengths, other pixels in both images, every
    paired scan on the other image, a camera whose principal point lies elsewhere, another stamp.  The images keep their places and
    their row steps, so whatever meets whatever, every read stays inside its buffer and every write inside the canvases."""

    def __init__(self, p, p_decoy, custom):
        self.b, b2 = K.keep_batch(p), K.keep_batch(p_decoy)
        assert self.b["offsets"].tolist() == b2["offsets"].tolist() and self.b["image_of_scan"].tolist() == b2["image_of_scan"].tolist()
        self.images = self.b["images"]
        self.decoy_images = [np.random.default_rng(900 + k).integers(0, 256, im.shape, dtype=np.uint8) for k, im in enumerate(self.images)]
        of = self.b["image_of_scan"]
        self.decoy_of = np.where(of >= 0, 1 - of, of).astype(np.int32)
        self.cam = self.b["cam"]
        self.decoy_cam = P.camera(width=P.KEEP_SIDE, height=P.KEEP_SIDE, cx=-1.0, cy=1.0)
        self.decoy_xyzi = b2["xyzi"]
        self.stamps = [OC.stamp_of_64(), [(b, a) for a, b in OC.stamp_of_64()]] if custom else [None, None]
        self.n_scans = len(of)
        self.stride = 3 * P.KEEP_SIDE + 1
        self.pitch = self.stride * P.KEEP_SIDE
        self.total = self.pitch * self.n_scans
        st = [s if s is not None else R.REFERENCE_STAMP for s in self.stamps]
        canv, self.want_n = R.overlay_batch(self.b["xyzi"], self.b["offsets"], self.images, of, self.cam, self.b["dis"], LO, HI, st[0])
        self.want = R.canvas_bytes(canv, self.cam, self.stride, self.pitch, self.total, SC.SENTINEL)
        canv, _ = R.overlay_batch(self.decoy_xyzi, self.b["offsets"], self.decoy_images, self.decoy_of, self.decoy_cam, self.b["dis"], LO, HI, st[1])
        self.want_decoy = R.canvas_bytes(canv, self.cam, self.stride, self.pitch, self.total, SC.SENTINEL)

    def case(self, name, plan):
        b = self.b
        scratch_bytes = overlay.overlay_batch_scratch_bytes(P.KEEP_SIDE, P.KEEP_SIDE, self.n_scans)
        held = {}

        def call(p, stream):
            job, keep = overlay.overlay_batch_job(p["xyzi"], b["offsets"], [p["image0"], p["image1"]], [im.shape[1] for im in self.images], b["image_of_scan"],
                                                  self.cam, p["canvas"], self.stride, self.pitch, p["scratch"], scratch_bytes, plan, b["dis"], LO, HI,
                                                  self.stamps[0], stream)
            held["job"], held["keep"] = job, keep
            st = overlay.lib().ilcc_overlay_batch_device(C.byref(job))
            assert st == N.OK, (st, N.lib().ilcc_last_error(None).decode())

        def scribble():
            off, of, ptrs, steps, xy, cam = held["keep"]
            of[:] = self.decoy_of
            C.memmove(C.addressof(cam), C.addressof(self.decoy_cam), C.sizeof(cam))
            ptrs[0], ptrs[1] = ptrs[1], ptrs[0]
            if xy is not None:
                flat = [int(v) for pair in self.stamps[1] for v in pair]
                C.memmove(C.addressof(xy), C.addressof((C.c_int8 * len(flat))(*flat)), len(flat))
            held["job"].inten_high = 1.0
            held["job"].d_canvas = None

        # the gaps between the rows and the unpaired canvases hold the sentinel whatever the inputs are: no decoy can change them
        unwritten = R.canvas_bytes([None if k < 0 else np.zeros((P.KEEP_SIDE, P.KEEP_SIDE, 3), np.uint8) for k in b["image_of_scan"]], self.cam,
                                   self.stride, self.pitch, self.total, 1) == 1
        return SC.Case(name, [SC.Buf("xyzi", b["xyzi"], self.decoy_xyzi), SC.Buf("image0", self.images[0], self.decoy_images[0]),
                              SC.Buf("image1", self.images[1], self.decoy_images[1]), SC.Buf("canvas", nbytes=self.total, out=True),
                              SC.Buf("scratch", nbytes=scratch_bytes, scratch=True)], call,
                       {"canvas": self.want}, {"canvas": self.want_decoy}, scribble=scribble, finish=lambda _: plan.finish(self.n_scans).tolist(),
                       host_want=self.want_n.tolist(), fixed={"canvas": unwritten})


@pytest.mark.gpu
@pytest.mark.parametrize("custom", [False, True], ids=["reference stamp", "stamp of 64 offsets"])
def test_k12b_on_a_delayed_stream(custom):
    plan = overlay.OverlayPlan(64, 80000)
    SC.check_entry(OverlayBatch(3, 1, custom).case("K12b keep_batch(3)", plan))
    plan.close()


@pytest.mark.gpu
def test_k12b_plan_reuse_on_two_streams():
    plan = overlay.OverlayPlan(64, 80000)
    first, second = OverlayBatch(3, 1, False).case("K12b keep_batch(3)", plan), OverlayBatch(5, 1, False).case("K12b keep_batch(5)", plan)
    (got_a, _), (got_b, ret_b) = SC.plan_reuse(first, second)
    SC.same(first, got_a, first.want, "the restatement")
    SC.same(second, got_b, second.want, "the restatement")
    assert ret_b == second.host_want
    plan.close()


# ------------------------------------------------------------------------------------------ the chain

QUALITY = 90


def _expected(**kw):
    clouds, images = K.recording()
    return R.chain(clouds, [(s, px, enc) for s, px, enc, _ in images], K.recording_camera(), K.T_LIDAR2CAM, K.DISTANCE, K.MAX_DT_NS, QUALITY, **kw)


def _same_items(got, want, pixels=True):
    assert len(got) == len(want)
    for (rec, blob, px), (wrec, wblob, wpx) in zip(got, want):
        assert {k: getattr(rec, k) for k in wrec} == wrec
        assert blob == wblob, wrec
        if wpx is None or not pixels:
            assert px is None
        else:
            assert px.tobytes() == wpx.tobytes(), wrec


@pytest.fixture(scope="module")
def bag(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlay_bag")
    K.write_recording(d / "rec.bag", "lz4")
    open(d / "cam.yaml", "w").write(K.yaml_text(K.recording_camera()))
    calib.extrinsic_write(str(d / "pose.bin"), K.T_LIDAR2CAM)
    return d


def _params(**kw):
    sp = overlay.default_overlay_sequence_params()
    sp.max_dt_ns = K.MAX_DT_NS
    sp.keep_pixels = 1
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def _run(bag, **kw):
    cam = CI.read_camera_yaml(str(bag / "cam.yaml"))
    return list(overlay.bag_pcd2image_all_pairs(str(bag / "rec.bag"), K.IMAGE_TOPIC, K.LIDAR_TOPIC, cam, K.T_LIDAR2CAM, distance_valid=K.DISTANCE,
                                                quality=QUALITY, sp=_params(**kw)))


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1], ids=["K17", "host encoder"])
def test_chain_equals_the_specification_in_every_batching(bag, route):
    want = _expected()
    assert [r["image_message"] for r, _, _ in want] == [0, 1, 1, 2, 3, -1, 4]
    sizes = K.cloud_data_bytes()
    assert sum(sizes[:4]) + 64 <= 350000 < sum(sizes[:5]) and sum(sizes[4:]) + 64 <= 350000
    per_scan = overlay.overlay_sequence_bytes(64, 48)
    # one batch; two (scans 0 .. 3 and 4 .. 6); seven, one scan each (the unpaired one a batch without device work); one paired scan a
    # batch by the device budget (the unpaired scan rides with scan 4); one image a batch; two of the limits at once
    for budgets in (dict(), dict(staging_bytes=350000), dict(staging_bytes=max(sizes)), dict(device_bytes=per_scan), dict(image_bytes=20000),
                    dict(staging_bytes=200000, device_bytes=2 * per_scan)):
        got = _run(bag, route=route, **budgets)
        _same_items(got, want)
        assert [rec.route for rec, _, _ in got] == [route] * 5 + [0] + [route], budgets
    # without keep_pixels: the same files, no pictures
    _same_items(_run(bag, route=route, keep_pixels=0, staging_bytes=350000), want, pixels=False)
    # first / stride / max_scans select as ilcc_sequence_params does
    got = _run(bag, route=route, first=1, stride=2, max_scans=3, staging_bytes=200000)
    _same_items(got, _expected(first=1, stride=2, max_scans=3))
    assert [r.message for r, _, _ in got] == [1, 3, 5]


@pytest.mark.gpu
def test_chain_capacity_fallback_gives_the_same_bytes(bag):
    """An out_bytes_per_image so small that K17's output holds the first pictures of the batch only: the others are finished by the
    host encoder from their coefficients, and nobody can tell from the bytes."""
    import jpeg_write_ref as JW
    want = _expected()
    head = len(JW.headers(JW.make_info(64, 48, (2, 2), QUALITY)))
    scans = [r["file_bytes"] - head - 2 for r, _, _ in want if r["image_message"] >= 0]
    room = (sum(-(-s // 16) * 16 for s in scans[:4]) + 8) // 6 // 16 * 16            # six pictures share 6 * room bytes: four fit, the fifth does not
    at, routes = 0, []
    for s in scans:                                                                 # K17's rule: an image past the end, and every image behind it
        routes.append(1 if (routes and routes[-1]) or at + s > 6 * room else 0)
        at += -(-s // 16) * 16
    assert routes == [0, 0, 0, 0, 1, 1]
    got = _run(bag, out_bytes_per_image=room)
    _same_items(got, want)
    assert [rec.route for rec, _, _ in got if rec.image_message >= 0] == routes
    # one picture a batch: each has `room` bytes to itself
    got = _run(bag, out_bytes_per_image=room, device_bytes=overlay.overlay_sequence_bytes(64, 48, room))
    _same_items(got, want)
    assert [rec.route for rec, _, _ in got if rec.image_message >= 0] == [1 if s > room else 0 for s in scans]
    assert 0 < sum(s > room for s in scans)


@pytest.mark.gpu
def test_program_and_python_mirror_write_the_specification_s_files(bag, tmp_path):
    import overlay_ref as O
    want = _expected()
    args = [CLI, "--all-pairs", "--bag", str(bag / "rec.bag"), "--image-topic", K.IMAGE_TOPIC, "--lidar-topic", K.LIDAR_TOPIC, "--yaml", str(bag / "cam.yaml"),
            "--extrinsic", str(bag / "pose.bin"), "--max-dt-ms", "50", "--distance-valid", str(K.DISTANCE), "--quality", str(QUALITY)]
    r = subprocess.run(args + ["--jpg-out-all", str(tmp_path / "o_"), "--ppm-out-all", str(tmp_path / "p_")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    paired_scans = [(rec, blob, px) for rec, blob, px in want if rec["image_message"] >= 0]
    assert sorted(os.listdir(tmp_path)) == sorted(["%s_%06d.%s" % (a, rec["message"], e) for rec, _, _ in paired_scans for a, e in (("o", "jpg"), ("p", "ppm"))])
    for rec, blob, px in paired_scans:
        assert open(tmp_path / ("o_%06d.jpg" % rec["message"]), "rb").read() == blob, rec
        assert O.read_ppm(str(tmp_path / ("p_%06d.ppm" % rec["message"]))).tobytes() == px[..., ::-1].tobytes(), rec      # B,G,R written as R,G,B
    lines = r.stdout.splitlines()
    assert len(lines) == 7 + 1 and "7 scans, 6 paired" in lines[-1]
    assert lines[1].startswith("cloud 1: image 1, dt 5.000 ms, 2500 points, %d drawn" % want[1][0]["n_drawn"]) and lines[1].endswith("gpu)")
    assert lines[5].startswith("cloud 5: no image within the limit (nearest dt -300.000 ms)")
    # the python helper writes the same files
    os.mkdir(tmp_path / "py")
    files = overlay.write_pcd2image_files(_run(bag), str(tmp_path / "py" / "o_"), str(tmp_path / "py" / "p_"))
    assert len(files) == 12 and all(open(f, "rb").read() == open(tmp_path / os.path.basename(f), "rb").read() for f in files)
    # --huffman host, a selection, no pictures: the same file
    os.mkdir(tmp_path / "host")
    r = subprocess.run(args + ["--jpg-out-all", str(tmp_path / "host" / "o_"), "--huffman", "host", "--first", "3", "--max-scans", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(tmp_path / "host") == ["o_000003.jpg"] and open(tmp_path / "host" / "o_000003.jpg", "rb").read() == want[3][1]
    assert r.stdout.splitlines()[0].endswith("host)")


@pytest.mark.gpu
def test_chain_refusals(bag, tmp_path):
    import camera_image_ref as IR
    import rosbag_writer as W
    cam = CI.read_camera_yaml(str(bag / "cam.yaml"))
    clouds, images = K.recording()
    run = lambda path, **kw: list(overlay.bag_pcd2image_all_pairs(str(path), K.IMAGE_TOPIC, K.LIDAR_TOPIC, cam, K.T_LIDAR2CAM, distance_valid=K.DISTANCE,
                                                                  sp=_params(**kw)))
    # a topic that carries only CompressedImage
    w = W.BagWriter(str(tmp_path / "compressed.bag"))
    w.add_chunk([(K.LIDAR_TOPIC, *K.PC2, (1, 0), K.cloud_msg(*clouds[0])), (K.IMAGE_TOPIC, *K.COMPRESSED, (1, 5), b"\0" * 40)])
    w.write()
    with pytest.raises(overlay.OverlayError) as e:
        run(tmp_path / "compressed.bag")
    assert e.value.status == N.BAD_ARGUMENT and "carries only sensor_msgs/CompressedImage" in str(e.value)
    # a wrong-sized image: the text names the message
    w = W.BagWriter(str(tmp_path / "odd.bag"))
    w.add_chunk([(K.LIDAR_TOPIC, *K.PC2, (1, 0), K.cloud_msg(*clouds[0])),
                 (K.IMAGE_TOPIC, *K.IMG, (1, 5), IR.image_msg(images[0][1], "mono8", stamp=images[0][0])),
                 (K.IMAGE_TOPIC, *K.IMG, (2, 5), IR.image_msg(images[0][1][:, :60], "mono8", stamp=images[1][0]))])
    w.write()
    with pytest.raises(overlay.OverlayError) as e:
        run(tmp_path / "odd.bag")
    assert e.value.status == N.BAD_ARGUMENT and "image message 1 is 60 x 48" in str(e.value)
    # a single scan, image or picture above its budget
    for kw in (dict(staging_bytes=1000), dict(image_bytes=9000), dict(device_bytes=overlay.overlay_sequence_bytes(64, 48) - 1)):
        with pytest.raises(overlay.OverlayError) as e:
            run(bag / "rec.bag", **kw)
        assert e.value.status == N.CAPACITY, kw
    for kw, text in ((dict(first=7), "select no message"), (dict(route=2), "route must be 0")):
        with pytest.raises(overlay.OverlayError) as e:
            run(bag / "rec.bag", **kw)
        assert e.value.status == N.BAD_ARGUMENT and text in str(e.value)
    # a failing sink: ILCC_IO_ERROR, after the second call (a batch is in flight behind it)
    calls = []

    def sink(_user, rec, _jpeg, _bytes, _bgr):
        calls.append(rec.contents.message)
        return 1 if len(calls) == 2 else 0

    T = np.ascontiguousarray(K.T_LIDAR2CAM, np.float64).reshape(16)
    n_scans, n_paired = C.c_uint32(0), C.c_uint32(0)
    sp = _params(staging_bytes=200000)
    path = str(bag / "rec.bag").encode()
    call = lambda bag_path, sp, sink: overlay.lib().ilcc_bag_pcd2image_all_pairs(0, bag_path, K.IMAGE_TOPIC.encode(), path, K.LIDAR_TOPIC.encode(), C.byref(cam),
                                                                                  T.ctypes.data_as(C.POINTER(C.c_double)), K.DISTANCE, QUALITY, sp, sink, None,
                                                                                  C.byref(n_scans), C.byref(n_paired))
    assert call(path, C.byref(sp), overlay.OVERLAY_SINK(sink)) == N.IO_ERROR and calls == [0, 1] and b"the sink refused scan 1" in N.lib().ilcc_last_error(None)
    assert (n_scans.value, n_paired.value) == (7, 6)
    # no sink: the counts alone; sp == NULL: the defaults (50 ms)
    assert call(path, None, overlay.OVERLAY_SINK(0)) == N.OK and (n_scans.value, n_paired.value) == (7, 6)
    assert call(None, None, overlay.OVERLAY_SINK(0)) == N.BAD_ARGUMENT
