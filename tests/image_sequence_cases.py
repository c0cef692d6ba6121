"""Fixtures of the image-sequence tests: constructed boards for the fusion (each case named for what it is; the CPU tests check
that it is that), K10b's batches of mixed content and of hundreds of small images, and the nine-image bag of the chain."""
import functools

import numpy as np

import camera_image_ref as CR
import image_sequence_ref as R
import rosbag_writer as W
from test_image_corners import _board_in, _noise, _squares, _tie_heavy_two_level, render_board

Q = 2.0 ** -10          # the constructed coordinates are multiples of this: their differences and medians are exact
SQUARE = 32.0
TOPIC = "/camera/image_raw"
IMG = (CR.IMAGE_TYPE, CR.IMAGE_MD5)


def lattice(rows, cols, origin=(100.0, 80.0), square=SQUARE):
    """(rows, cols, 2): entry (i, j) at origin + square (j, i) plus a small fixed shear, so that no two variants tie"""
    i, j = np.mgrid[0:rows, 0:cols].astype(np.float64)
    return np.stack([origin[0] + square * j + 2.0 * i, origin[1] + square * i + 1.0 * j], -1)


def numbered(board, v):
    """the board as an image numbered by variant v reports it: alignment to `board` picks v back"""
    R_, C_ = board.shape[:2]
    flat = board.reshape(-1, 2)
    out = np.zeros_like(flat)
    out[R.variant_perm(R_, C_, v)] = flat
    return out.reshape((C_, R_, 2) if v & 4 else (R_, C_, 2))


def jitter(board, k, scale=8):
    """deterministic offsets of at most `scale` Q per coordinate, different for every k"""
    rng = np.random.default_rng(1000 + k)
    return board + Q * rng.integers(-scale, scale + 1, board.shape)


def fusion_cases():
    """[(name, boards, accepted, a, b, gate_px)]"""
    cases = []
    b75 = lattice(5, 7)                                   # rows x cols = 5 x 7 for the 7 x 5 board
    # every variant a non-square board has: 0-3 in the reference's shape, 4-7 transposed; odd and even counts
    for n in (9, 8):
        boards = [numbered(jitter(b75, k) if k else b75, k % 8) for k in range(n)]
        cases.append(("variants_7x5_n%d" % n, boards, [1] * n, 7, 5, 0.0))
    b55 = lattice(5, 5)
    boards = [numbered(jitter(b55, k) if k else b55, k % 8) for k in range(9)]
    cases.append(("variants_5x5_square", boards, [1] * 9, 5, 5, 0.0))
    # the reference image itself is transposed: the fused board has ITS shape
    boards = [numbered(b75, 4)] + [jitter(b75, k) for k in range(1, 5)]
    cases.append(("transposed_reference", boards, [1] * 5, 7, 5, 0.0))
    # one image reads the board one square off along its long axis
    off = b75 + np.array([SQUARE, 1.0])                    # entry (i, j) of the shifted reading = entry (i, j + 1) of the board
    boards = [jitter(b75, k) for k in range(6)]
    boards[3] = off
    cases.append(("one_square_off", boards, [1] * 6, 7, 5, 0.0))
    # on the gate: the one moved corner of image 2 lies exactly gate away from the median, d2 == gate^2 -> used
    boards = [b75.copy() for _ in range(5)]
    boards[2] = b75.copy()
    boards[2][1, 2] += np.array([3.0, 4.0])                # 3-4-5: distance 5 exactly
    cases.append(("at_gate", boards, [1] * 5, 7, 5, 5.0))
    boards = [bd.copy() for bd in boards]
    cases.append(("gate_one_ulp_below", boards, [1] * 5, 7, 5, float(np.nextafter(5.0, 0.0))))
    # exactly half within the gate: no majority
    boards = [b75, b75 + Q, b75 + np.array([10.0, 0.0]), b75 + np.array([-10.0, 0.0])]
    cases.append(("exactly_half", boards, [1] * 4, 7, 5, 6.0))
    cases.append(("none_used", [b75, b75 + np.array([40.0, 0.0])], [1, 1], 7, 5, 1.0))
    cases.append(("none_accepted", [b75, b75], [0, 0], 7, 5, 0.0))
    cases.append(("no_images", [], [], 7, 5, 0.0))
    nan = np.full((5, 7, 2), np.nan)
    cases.append(("nan_not_accepted", [nan, jitter(b75, 1), nan, jitter(b75, 2), jitter(b75, 3)], [0, 1, 0, 1, 1], 7, 5, 0.0))
    cases.append(("single", [b75], [1], 7, 5, 0.0))
    return cases


def refusal_cases():
    b75 = lattice(5, 7)
    bad = b75.copy()
    bad[2, 3, 1] = np.inf
    return [
        ("a_below_3", [lattice(5, 2)], [1], 2, 5, 0.0),
        ("b_below_3", [lattice(2, 7)], [1], 7, 2, 0.0),
        ("too_many_corners", [lattice(17, 16)], [1], 16, 17, 0.0),
        ("shape_neither", [b75, lattice(4, 7)], [1, 1], 7, 5, 0.0),
        ("gate_nan", [b75], [1], 7, 5, float("nan")),
        ("gate_inf", [b75], [1], 7, 5, float("inf")),
        ("accepted_non_finite", [b75, bad], [1, 1], 7, 5, 0.0),
    ]


# ---- K10b batches ----------------------------------------------------------------------------------------------------------------
W0, H0 = 160, 128


@functools.lru_cache(maxsize=None)
def mixed_images():
    """160 x 128, each with its own min / max; the noise image gives hundreds of candidates out of 1 008 scan blocks"""
    return dict(noise=_noise(W0, H0, 11), squares=_squares(W0, H0, 12), board=_board_in(60, 190),
                range1=_board_in(127, 128, noise=0), range3=_board_in(127, 130, noise=0), constant=np.full((H0, W0), 77, np.uint8),
                noise2=_noise(W0, H0, 13), squares2=_squares(W0, H0, 14), tie_heavy=_tie_heavy_two_level())


def mixed_batch(names):
    return [mixed_images()[n] for n in names]


BATCHES = {
    "n1": ["noise"],
    "n2": ["squares", "board"],
    "n3_constant_first": ["constant", "noise", "board"],
    "n3_constant_middle": ["squares", "constant", "range3"],
    "n3_constant_last": ["range1", "noise2", "constant"],
    "n9": ["noise", "squares", "board", "range1", "constant", "range3", "noise2", "squares2", "tie_heavy"],
    "constant_only": ["constant", "constant", "constant"],
}


def seam_batch(w, h):
    """three images of w x h with different content on both sides of every seam"""
    return [_noise(w, h, 21), _squares(w, h, 22), _noise(w, h, 23)]


# ---- K10b batches of hundreds of images ---------------------------------------------------------------------------------------------
# k10b_offsets scans the batch's n * cpi chunk counts 256 at a time with a carry between the tiles (cpi: chunks of 256 scan blocks per
# image), and one loop writes cand_offsets[0 .. n].  Square images of three sides give cpi 1, 2 and 3; each batch is drawn from eight
# distinct images of its side, in a random -- so aperiodic -- order.
MANY_SIDES = {1: 34, 2: 84, 3: 108}                     # cpi -> side; 34 is the smallest side the entry takes
MANY_MEMBERS = ("noise_a", "noise_b", "noise_c", "noise_d", "squares_a", "squares_b", "constant_a", "constant_b")
WITH_CANDIDATES = MANY_MEMBERS[:6]


@functools.lru_cache(maxsize=None)
def many_images(side):
    return dict(noise_a=_noise(side, side, 40), noise_b=_noise(side, side, 41), noise_c=_noise(side, side, 42), noise_d=_noise(side, side, 43),
                squares_a=_squares(side, side, 50), squares_b=_squares(side, side, 53),
                constant_a=np.full((side, side), 77, np.uint8), constant_b=np.full((side, side), 200, np.uint8))


def _draw(seed, names, n, with_candidates_at=()):
    """n names in random order; at the given places (the two sides of a tile seam), images that have candidates"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    out = [names[i] for i in rng.integers(0, len(names), n)]
    for k in with_candidates_at:
        out[k] = WITH_CANDIDATES[int(rng.integers(0, len(WITH_CANDIDATES)))]
    return out


def _constant_run():
    """600 images: chunks 256 .. 511, the whole second tile of the scan, are constant images' (and some on both sides of it), with
    images that have candidates before and behind the run"""
    return _draw(5, WITH_CANDIDATES, 250) + _draw(6, MANY_MEMBERS[6:], 270) + _draw(7, WITH_CANDIDATES, 80)


# name -> (cpi, member names)
MANY_BATCHES = {
    "cpi1_n256_all_with_candidates": (1, _draw(1, WITH_CANDIDATES, 256)),       # exactly one tile; cand_offsets[256] by the loop's second trip
    "cpi1_n257": (1, _draw(2, MANY_MEMBERS, 257, (255, 256))),                              # a second tile of one chunk
    "cpi1_n600": (1, _draw(3, MANY_MEMBERS, 600, (255, 256, 511, 512, 599))),                              # three tiles: the carry is applied twice
    "cpi1_n600_constant_run": (1, _constant_run()),                             # a tile whose total is 0: the carry passes through it
    "cpi1_n600_first_only": (1, ["noise_b"] + _draw(8, MANY_MEMBERS[6:], 599)),
    "cpi1_n600_last_only": (1, _draw(9, MANY_MEMBERS[6:], 599) + ["noise_c"]),
    "cpi3_n86": (3, _draw(4, MANY_MEMBERS, 86, (84, 85))),                                # 258 chunks: the seam lies inside image 85
    "cpi2_n129": (2, _draw(10, MANY_MEMBERS, 129, (127, 128))),                             # 258 chunks: the seam lies between images 127 and 128
}


def many_batch(name):
    cpi, names = MANY_BATCHES[name]
    return [many_images(MANY_SIDES[cpi])[n] for n in names]


# ---- the chain's bag ---------------------------------------------------------------------------------------------------------------
CHAIN_SIZE, CHAIN_SQUARE, CHAIN_THETA = (480, 400), 36.0, 0.2
# seeds 0 .. 8 of render_board; image 3 is shifted one square along the board's long axis, image 6 has an occluded corner
CHAIN_SEEDS = list(range(9))
CHAIN_SHIFTED, CHAIN_OCCLUDED = 3, 6


@functools.lru_cache(maxsize=None)
def chain_images():
    """[(uint8 image, true corners [5][7] -> (u, v))] -- the truth of the shifted image is its own (shifted) board"""
    out = []
    c, s = np.cos(CHAIN_THETA), np.sin(CHAIN_THETA)
    for k, seed in enumerate(CHAIN_SEEDS):
        centre = (CHAIN_SIZE[0] / 2, CHAIN_SIZE[1] / 2)
        if k == CHAIN_SHIFTED:
            centre = (centre[0] + CHAIN_SQUARE * c, centre[1] + CHAIN_SQUARE * s)
        occlude = None
        if k == CHAIN_OCCLUDED:
            _, truth = render_board(CHAIN_SIZE, square=CHAIN_SQUARE, theta=CHAIN_THETA, seed=seed)
            occlude = (truth[2, 3, 0], truth[2, 3, 1], 9.0)
        out.append(render_board(CHAIN_SIZE, square=CHAIN_SQUARE, theta=CHAIN_THETA, seed=seed, centre=centre, occlude=occlude))
    return out


def chain_messages(encoding="mono8", images=None):
    """the serialized Image messages of the chain's bag: stamp (100 + k, 7 k)"""
    images = images if images is not None else [im for im, _ in chain_images()]
    return [CR.image_msg(encode(im, encoding), encoding, seq=k, stamp=(100 + k, 7 * k)) for k, im in enumerate(images)]


def encode(gray, encoding):
    """pixels of `encoding` whose mono8 conversion is `gray`: the gray value in every channel (Y of (g, g, g) is g)"""
    if encoding == "mono8" or encoding.startswith("bayer_"):
        return gray
    ch = 4 if encoding.endswith("a8") else 3
    out = np.repeat(gray[..., None], ch, axis=2)
    if ch == 4:
        out[..., 3] = 255
    return out


def write_bag(path, messages, topic=TOPIC, per_chunk=4, compression="none", conn=IMG, t0=50):
    """the messages in record-time order, `per_chunk` to a chunk; -> the path"""
    bag = W.BagWriter(str(path), compression)
    for c in range(0, len(messages), per_chunk):
        bag.add_chunk([(topic,) + conn + ((t0 + k, 0), messages[k]) for k in range(c, min(c + per_chunk, len(messages)))])
    bag.write()
    return str(path)


def chain_camera():
    """a mildly distorting camera of the chain's image size"""
    return CR.camera(520.0, 236.5, 515.0, 203.25, (-0.06, 0.02, 0.0005, -0.0004, 0.0), *CHAIN_SIZE)


def yaml_text(cam, board=(7, 5)):
    K_ = [cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1]
    return ("%%YAML:1.0\n\nK: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [%s]\n"
            "d: !!opencv-matrix\n   rows: 5\n   cols: 1\n   dt: d\n   data: [%s]\n\nCamera.width: %d\nCamera.height: %d\n\n"
            "grid_length: 0.15\ncorner_in_x: %d\ncorner_in_y: %d\n"
            % (", ".join(repr(float(v)) for v in K_), ", ".join(repr(float(v)) for v in cam.d), cam.width, cam.height, board[0], board[1]))
