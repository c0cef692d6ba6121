"""LiDAR points drawn on the undistorted colour image: ctypes mirror of ``include/ilcc_overlay.h`` -- the
reference's pcd2image node (/root/reference/ilcc2/test/pcd2image.cpp:33-89) from bags, without ROS or OpenCV.
The stages it chains are in ``camera_image`` (K11c ``to_bgr8``), ``ingest`` (K0) and ``project`` (K8, K12
``draw_hits_device``).  The camera is the lens (``camera_image.CameraModel``), the extrinsic a 4 x 4; the library
makes K8's ``project.Projection`` of the two."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import CameraImageError, CameraModel

OVERLAY_EXPORTS = ["ilcc_bag_pcd2image", "ilcc_save_ppm_bgr"]

_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        i32p = C.POINTER(C.c_int32)
        L.ilcc_bag_pcd2image.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(CameraModel),
                                         C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_uint64, i32p, i32p,
                                         C.POINTER(C.c_uint32)]
        L.ilcc_bag_pcd2image.restype = C.c_int32
        L.ilcc_save_ppm_bgr.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]
        L.ilcc_save_ppm_bgr.restype = C.c_int32
        _ready = True
    return L


def _check(st):
    if st != _native.OK:
        raise CameraImageError(st)


def bag_pcd2image(image_bag, image_topic, lidar_topic, camera, T_lidar2cam, lidar_bag=None, distance_valid=5.0, device=0):
    """(image, n_drawn): the (rows, cols, 3) uint8 B,G,R picture pcd2image shows for the first Image on image_topic and
    the first PointCloud2 on lidar_topic (of lidar_bag, or of the same bag), and the number of points drawn.  Bytes 0, 1, 2
    of a drawn pixel hold (r, g, b), as in the reference."""
    L = lib()
    T = np.ascontiguousarray(T_lidar2cam, dtype=np.float64).reshape(16)
    w, h, n = C.c_int32(0), C.c_int32(0), C.c_uint32(0)
    args = (device, os.fsencode(image_bag), image_topic.encode(), os.fsencode(lidar_bag if lidar_bag is not None else image_bag),
            lidar_topic.encode(), C.byref(camera), T.ctypes.data_as(C.POINTER(C.c_double)), distance_valid)
    st = L.ilcc_bag_pcd2image(*args, None, 0, C.byref(w), C.byref(h), C.byref(n))
    if st not in (_native.OK, _native.CAPACITY):
        raise CameraImageError(st)
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _check(L.ilcc_bag_pcd2image(*args, out.ctypes.data_as(C.c_void_p), out.size, C.byref(w), C.byref(h), C.byref(n)))
    return out, n.value


def save_ppm_bgr(filename, bgr):
    """Binary PPM (P6) of a (rows, cols, 3) B,G,R image, written as R,G,B."""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected (rows, cols, 3) uint8, got %s" % (a.shape,))
    _check(lib().ilcc_save_ppm_bgr(os.fsencode(filename), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))
