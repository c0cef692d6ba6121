"""Camera images from bags or raw frames: ctypes mirror of ``include/ilcc_camera_image.h`` -- the
intrinsics of an OpenCV YAML, the layout of a serialized sensor_msgs/Image, conversion to mono8 and
cv::undistort in one GPU kernel (K11; K11c keeps the colour: B, G, R; both demosaic the raw bayer_*8 frames of a colour camera
on the way, as cv_bridge does), and the two bag entries that end in host pixels or in the
chessboard's corners.  What comes out of ``to_mono8(..., camera)`` is what
``image_corners.find_chessboard`` takes."""
import ctypes as C
import os

import numpy as np

from . import _native
from .image_corners import BoardNotFound

IMAGE_MD5 = "060021388200f6f0f447d0fcd9c64743"
ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")       # index = ilcc_image_encoding
BAYER_ENCODINGS = {"bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19}   # raw colour-camera frames
BYTES_PER_PIXEL = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, **{name: 1 for name in BAYER_ENCODINGS}}
MAP_OUTSIDE = -2 ** 31                                         # code of an output pixel without a source

CAMERA_IMAGE_EXPORTS = ["ilcc_read_camera_yaml", "ilcc_image_parse", "ilcc_image_parse_any", "ilcc_image_to_mono8_device",
                        "ilcc_image_to_bgr8_device", "ilcc_undistort_map_device", "ilcc_bag_first_image", "ilcc_bag_find_chessboard"]


def encoding_code(name) -> int:
    """ilcc_image_encoding of an encoding's name: 0 .. 4 for ENCODINGS, 16 .. 19 for BAYER_ENCODINGS."""
    if name in BAYER_ENCODINGS:
        return BAYER_ENCODINGS[name]
    if name in ENCODINGS:
        return ENCODINGS.index(name)
    raise ValueError("unsupported encoding %r (supported: %s)" % (name, ", ".join(ENCODINGS + tuple(BAYER_ENCODINGS))))


class CameraModel(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("d", C.c_double * 5),
                ("width", C.c_int32), ("height", C.c_int32)]

    @classmethod
    def make(cls, fx, cx, fy, cy, d, width, height):
        """Intrinsics in pointgrey.yaml's reading order (K's first row, then its second); d = (k1, k2, p1, p2[, k3])."""
        d = tuple(d) + (0.0,) * (5 - len(d))
        return cls(fx, fy, cx, cy, (C.c_double * 5)(*d), width, height)


class ImageLayout(C.Structure):
    _fields_ = [("height", C.c_uint32), ("width", C.c_uint32), ("step", C.c_uint32), ("encoding", C.c_uint32),
                ("is_bigendian", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("seq", C.c_uint32),
                ("data_offset", C.c_uint64), ("data_bytes", C.c_uint64), ("frame_id", C.c_char * 64)]

    @property
    def encoding_name(self):
        for name, code in BAYER_ENCODINGS.items():
            if code == self.encoding:
                return name
        return ENCODINGS[self.encoding]


class CameraImageError(RuntimeError):
    def __init__(self, status):
        self.status = status
        super().__init__("%s: %s" % (_native.strerror(status), _native.lib().ilcc_last_error(None).decode()))


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        i32p, cam = C.POINTER(C.c_int32), C.POINTER(CameraModel)
        L.ilcc_read_camera_yaml.argtypes = [C.c_char_p, cam]
        L.ilcc_read_camera_yaml.restype = C.c_int32
        L.ilcc_image_parse.argtypes = [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(ImageLayout)]
        L.ilcc_image_parse.restype = C.c_int32
        L.ilcc_image_parse_any.argtypes = L.ilcc_image_parse.argtypes
        L.ilcc_image_parse_any.restype = C.c_int32
        L.ilcc_image_to_mono8_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, cam, C.c_void_p,
                                                 C.c_int32, C.c_void_p]
        L.ilcc_image_to_mono8_device.restype = C.c_int32
        L.ilcc_image_to_bgr8_device.argtypes = L.ilcc_image_to_mono8_device.argtypes
        L.ilcc_image_to_bgr8_device.restype = C.c_int32
        L.ilcc_undistort_map_device.argtypes = [cam, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ilcc_undistort_map_device.restype = C.c_int32
        L.ilcc_bag_first_image.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, cam, C.c_void_p, C.c_uint64, i32p, i32p]
        L.ilcc_bag_first_image.restype = C.c_int32
        L.ilcc_bag_find_chessboard.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, cam, C.c_int32, C.c_int32, i32p, i32p,
                                               C.POINTER(C.c_double)]
        L.ilcc_bag_find_chessboard.restype = C.c_int32
        _ready = True
    return L


def _check(st):
    if st in (_native.BOARD_NOT_FOUND, _native.AMBIGUOUS):
        raise BoardNotFound(st, "%s: %s" % (_native.strerror(st), _native.lib().ilcc_last_error(None).decode()))
    if st != _native.OK:
        raise CameraImageError(st)


def _camera_ref(camera):
    return C.byref(camera) if camera is not None else None


def read_camera_yaml(path) -> CameraModel:
    """K, d and Camera.width / Camera.height of an OpenCV-FileStorage YAML (ImageCornersEst::getRectifyParam)."""
    cam = CameraModel()
    _check(lib().ilcc_read_camera_yaml(os.fsencode(path), C.byref(cam)))
    return cam


def parse_image(msg: bytes) -> ImageLayout:
    """Layout of a serialized sensor_msgs/Image."""
    lay = ImageLayout()
    arr = (C.c_uint8 * max(1, len(msg))).from_buffer_copy(msg if msg else b"\0")
    _check(lib().ilcc_image_parse(arr, len(msg), C.byref(lay)))
    return lay


def parse_image_any(msg: bytes) -> ImageLayout:
    """parse_image, and the four Bayer encodings as well (layout.encoding 16 .. 19): what the bag entries read with."""
    lay = ImageLayout()
    arr = (C.c_uint8 * max(1, len(msg))).from_buffer_copy(msg if msg else b"\0")
    _check(lib().ilcc_image_parse_any(arr, len(msg), C.byref(lay)))
    return lay


def _device_pixels(image, encoding):
    """The pixels as a device tensor (rows, cols, bytes per pixel) K11 can read in place, and its row pitch."""
    import torch
    encoding_code(encoding)                                    # ValueError for a name that is none of the nine
    bpp = BYTES_PER_PIXEL[encoding]
    t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if t.dim() == 2 and bpp == 1:
        t = t.unsqueeze(2)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != bpp:
        raise ValueError("expected uint8 pixels of shape (rows, cols%s) for %s, got %s %s"
                         % ("" if bpp == 1 else ", %d" % bpp, encoding, tuple(image.shape), t.dtype))
    h, w = int(t.shape[0]), int(t.shape[1])
    on_device = t.is_cuda and t.device.index == torch.cuda.current_device()
    rows_ok = t.stride(2) == 1 and t.stride(1) == bpp and (h == 1 or t.stride(0) >= w * bpp)
    if not (on_device and rows_ok):
        t = t.to("cuda").contiguous()
    return t, (int(t.stride(0)) if h > 1 else w * bpp)


def to_mono8(image, encoding, camera=None):
    """K11: (rows, cols) mono8 or Bayer, or (rows, cols, channels) colour uint8 pixels, numpy or torch, ->
    (rows, cols) uint8 tensor on the current HIP device: cv::undistort(mono8(image), K, d, K) with a
    camera, mono8(image) without.  A device tensor whose pixels are contiguous is read in place with
    stride(0) as the row pitch (a view of a pitched frame is not copied); asynchronous on the current stream."""
    import torch
    t, step = _device_pixels(image, encoding)
    h, w = int(t.shape[0]), int(t.shape[1])
    out = torch.empty((h, w), dtype=torch.uint8, device=t.device)
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    _check(lib().ilcc_image_to_mono8_device(C.c_void_p(t.data_ptr()), w, h, step, encoding_code(encoding), _camera_ref(camera),
                                            C.c_void_p(out.data_ptr()), w, stream))
    return out


def to_bgr8(image, encoding, camera=None):
    """K11c: the same pixels -> (rows, cols, 3) uint8 tensor, B, G, R: cv::undistort(bgr8(image), K, d, K) with a
    camera, bgr8(image) without (what pcd2image draws on).  Reads device views in place like to_mono8."""
    import torch
    t, step = _device_pixels(image, encoding)
    h, w = int(t.shape[0]), int(t.shape[1])
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=t.device)
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    _check(lib().ilcc_image_to_bgr8_device(C.c_void_p(t.data_ptr()), w, h, step, encoding_code(encoding), _camera_ref(camera),
                                           C.c_void_p(out.data_ptr()), 3 * w, stream))
    return out


def undistort_map(camera):
    """K11's stage output: (iu, iv) int32 tensors (height, width), the 1/32-pixel source coordinates of every
    output pixel; MAP_OUTSIDE where there is none."""
    import torch
    iu = torch.empty((max(camera.height, 0), max(camera.width, 0)), dtype=torch.int32, device="cuda")
    iv = torch.empty_like(iu)
    stream = C.c_void_p(torch.cuda.current_stream(iu.device).cuda_stream)
    _check(lib().ilcc_undistort_map_device(C.byref(camera), C.c_void_p(iu.data_ptr()), C.c_void_p(iv.data_ptr()), stream))
    return iu, iv


def bag_first_image(bag_path, topic, camera=None, device=0) -> np.ndarray:
    """(rows, cols) uint8: the first sensor_msgs/Image on `topic` as mono8, undistorted when a camera is given
    (get_image_corners_bag.cpp:67-112 up to the imwrite)."""
    L = lib()
    w, h = C.c_int32(0), C.c_int32(0)
    args = (device, os.fsencode(bag_path), topic.encode(), _camera_ref(camera))
    st = L.ilcc_bag_first_image(*args, None, 0, C.byref(w), C.byref(h))
    if st not in (_native.OK, _native.CAPACITY):
        raise CameraImageError(st)
    out = np.zeros((h.value, w.value), np.uint8)
    _check(L.ilcc_bag_first_image(*args, out.ctypes.data_as(C.c_void_p), out.size, C.byref(w), C.byref(h)))
    return out


def bag_find_chessboard(bag_path, topic, camera, board=(7, 5), device=0) -> np.ndarray:
    """The chessboard of the bag's first image as image_corners.find_chessboard returns it: (rows, cols, 2)
    0-based (u, v).  Raises BoardNotFound when there is none or more than one."""
    xy = np.zeros(board[0] * board[1] * 2)
    r, k = C.c_int32(0), C.c_int32(0)
    _check(lib().ilcc_bag_find_chessboard(device, os.fsencode(bag_path), topic.encode(), _camera_ref(camera), board[0], board[1],
                                          C.byref(r), C.byref(k), xy.ctypes.data_as(C.POINTER(C.c_double))))
    return xy.reshape(r.value, k.value, 2)
