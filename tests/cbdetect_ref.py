"""fp64 numpy restatement of libcbdetect's corner detector (findCorners.m and the stages it calls),
written from the algorithm for the stage-parity tests of K10 (include/ilcc_image_corners.h).

Coordinates follow the reference: 1-based (MATLAB) inside the stages, ``find_corners`` returns
0-based positions (findCorners.m:124-125).  Images are indexed [row = v, col = u].
"""
import math

import numpy as np

RADII = (4, 8, 12)
# (angle_1, angle_2, radius) of the six template classes, findCorners.m:52
TEMPLATE_PROPS = [(0.0, math.pi / 2, 4), (math.pi / 4, -math.pi / 4, 4), (0.0, math.pi / 2, 8),
                  (math.pi / 4, -math.pi / 4, 8), (0.0, math.pi / 2, 12), (math.pi / 4, -math.pi / 4, 12)]
NMS_N, NMS_TAU, NMS_MARGIN = 3, 0.025, 5
REFINE_R = 10
SCORE_TAU = 0.01


def mround(x):
    """MATLAB round: half away from zero."""
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def template(angle_1, angle_2, radius):
    """createCorrelationPatch.m: four quadrant kernels (a1, a2, b1, b2), each summing to 1.
    Pixels within 0.1 of either edge line belong to none."""
    w = 2 * radius + 1
    u = np.arange(1, w + 1, dtype=np.float64)[None, :] - (radius + 1)
    v = np.arange(1, w + 1, dtype=np.float64)[:, None] - (radius + 1)
    u, v = np.broadcast_to(u, (w, w)), np.broadcast_to(v, (w, w))
    dist = np.sqrt(u * u + v * v)
    s1 = u * -math.sin(angle_1) + v * math.cos(angle_1)
    s2 = u * -math.sin(angle_2) + v * math.cos(angle_2)
    sigma = radius / 2
    g = np.exp(-0.5 * (dist / sigma) ** 2) / (math.sqrt(2 * math.pi) * sigma)
    masks = [(s1 <= -0.1) & (s2 <= -0.1), (s1 >= 0.1) & (s2 >= 0.1),
             (s1 <= -0.1) & (s2 >= 0.1), (s1 >= 0.1) & (s2 <= -0.1)]
    out = []
    for m in masks:
        k = np.where(m, g, 0.0)
        out.append(k / k.sum())
    return out


def conv2_same(img, k):
    """conv2(img, k, 'same'): zero padding, flipped kernel (odd kernel sizes)."""
    r = k.shape[0] // 2
    h, w = img.shape
    pad = np.zeros((h + 2 * r, w + 2 * r))
    pad[r:r + h, r:r + w] = img
    out = np.zeros((h, w))
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            c = k[r + dy, r + dx]
            if c != 0.0:
                out += c * pad[r - dy:r - dy + h, r - dx:r - dx + w]
    return out


def gradients(img_u8):
    """Integer numerators of img_du / img_dv (findCorners.m:31-37 on im2double = I / 255)."""
    I = np.asarray(img_u8, dtype=np.int32)
    h, w = I.shape
    P = np.zeros((h + 2, w + 2), dtype=np.int32)
    P[1:h + 1, 1:w + 1] = I
    # du = [-1 0 1] in every row; conv2 flips it: left column minus right column
    du = sum(P[y:y + h, 0:w] - P[y:y + h, 2:w + 2] for y in range(3))
    dv = sum(P[0:h, x:x + w] - P[2:h + 2, x:x + w] for x in range(3))
    return du.astype(np.int32), dv.astype(np.int32)


def angle_weight(du_num, dv_num):
    du, dv = du_num / 255.0, dv_num / 255.0
    ang = np.arctan2(dv, du)
    ang = np.where(ang < 0, ang + math.pi, ang)
    ang = np.where(ang > math.pi, ang - math.pi, ang)
    return du, dv, ang, np.sqrt(du * du + dv * dv)


def normalised(img_u8):
    I = np.asarray(img_u8, dtype=np.float64)
    lo, hi = I.min(), I.max()
    return (I - lo) / (hi - lo)


def likelihood(img_u8):
    """findCorners.m:56-85: max over the six classes of the two-case min/max response."""
    img = normalised(img_u8)
    best = np.zeros(img.shape)
    for a1_, a2_, r in TEMPLATE_PROPS:
        a1, a2, b1, b2 = [conv2_same(img, k) for k in template(a1_, a2_, r)]
        mu = (a1 + a2 + b1 + b2) / 4
        c1 = np.minimum(np.minimum(a1 - mu, a2 - mu), np.minimum(mu - b1, mu - b2))
        c2 = np.minimum(np.minimum(mu - a1, mu - a2), np.minimum(b1 - mu, b2 - mu))
        best = np.maximum(best, np.maximum(c1, c2))
    return best


def nms(L, n=NMS_N, tau=NMS_TAU, margin=NMS_MARGIN):
    """nonMaximumSuppression.m: 1-based (u, v), x outer, y inner, and each kept maximum's value."""
    h, w = L.shape
    out, vals = [], []
    for i in range(n + 1 + margin, w - n - margin + 1, n + 1):
        for j in range(n + 1 + margin, h - n - margin + 1, n + 1):
            maxi, maxj, maxval = i, j, L[j - 1, i - 1]
            for i2 in range(i, i + n + 1):
                for j2 in range(j, j + n + 1):
                    if L[j2 - 1, i2 - 1] > maxval:
                        maxi, maxj, maxval = i2, j2, L[j2 - 1, i2 - 1]
            failed = False
            for i2 in range(maxi - n, min(maxi + n, w - margin) + 1):
                for j2 in range(maxj - n, min(maxj + n, h - margin) + 1):
                    if L[j2 - 1, i2 - 1] > maxval and (i2 < i or i2 > i + n or j2 < j or j2 > j + n):
                        failed = True
                        break
                if failed:
                    break
            if maxval >= tau and not failed:
                out.append((maxi, maxj))
                vals.append(maxval)
    return out, vals


def mean_shift_modes(hist, sigma=1.0):
    """findModesMeanShift.m: (modes [(1-based bin, smoothed value)] by value descending, smoothed)."""
    n = len(hist)
    r = mround(2 * sigma)
    js = np.arange(-r, r + 1)
    wts = np.exp(-0.5 * (js / sigma) ** 2) / (math.sqrt(2 * math.pi) * sigma)
    hs = np.array([sum(hist[(i + j) % n] * wts[k] for k, j in enumerate(js)) for i in range(n)])
    # the reference's `if abs(h - h(1)) < 1e-5` is true only when it holds for every bin
    if np.all(np.abs(hs - hs[0]) < 1e-5):
        return [], hs
    modes = []
    for i in range(n):
        j = i
        while True:
            h0, j1, j2 = hs[j], (j + 1) % n, (j - 1) % n
            h1, h2 = hs[j1], hs[j2]
            if h1 >= h0 and h1 >= h2:
                j = j1
            elif h2 > h0 and h2 > h1:
                j = j2
            else:
                break
        if all(m[0] != j + 1 for m in modes):
            modes.append((j + 1, hs[j]))
    modes.sort(key=lambda m: -m[1])      # stable, as MATLAB's sort
    return modes, hs


def edge_orientations(ang, wt):
    """refineCorners.m edgeOrientations: two dominant edge directions, or zeros."""
    z = (np.zeros(2), np.zeros(2))
    a = ang.reshape(-1, order="F") + math.pi / 2
    a = np.where(a > math.pi, a - math.pi, a)
    wv = wt.reshape(-1, order="F")
    hist = np.zeros(32)
    for ai, wi in zip(a, wv):
        b = max(min(int(math.floor(ai / (math.pi / 32))), 31), 0)
        hist[b] += wi
    modes, _ = mean_shift_modes(hist, 1.0)
    if len(modes) <= 1:
        return z
    m = sorted([(b - 1) * math.pi / 32 for b, _ in modes[:2]])
    if min(m[1] - m[0], m[0] + math.pi - m[1]) <= 0.3:
        return z
    return np.array([math.cos(m[0]), math.sin(m[0])]), np.array([math.cos(m[1]), math.sin(m[1])])


def smallest_eigvec(A):
    """Unit eigenvector of the smaller eigenvalue of a symmetric 2 x 2 (sign is irrelevant here)."""
    w, V = np.linalg.eigh(A)
    return V[:, 0]


def refine(du, dv, ang, wt, pts, r=REFINE_R):
    """refineCorners.m.  pts: 1-based integer (u, v).  Returns p (1-based, float), v1, v2."""
    h, w = du.shape
    P = np.array(pts, dtype=np.float64).reshape(-1, 2)
    V1, V2 = np.zeros_like(P), np.zeros_like(P)
    for i, (cu, cv) in enumerate(pts):
        u0, u1, v0, v1_ = max(cu - r, 1), min(cu + r, w), max(cv - r, 1), min(cv + r, h)
        sl = (slice(v0 - 1, v1_), slice(u0 - 1, u1))
        e1, e2 = edge_orientations(ang[sl], wt[sl])
        V1[i], V2[i] = e1, e2
        if (e1[0] == 0 and e1[1] == 0) or (e2[0] == 0 and e2[1] == 0):
            continue
        gu, gv = du[sl], dv[sl]
        nrm = np.sqrt(gu * gu + gv * gv)
        ok = nrm >= 0.1
        ou, ov = np.where(ok, gu / np.where(ok, nrm, 1), 0), np.where(ok, gv / np.where(ok, nrm, 1), 0)
        in1 = ok & (np.abs(ou * e1[0] + ov * e1[1]) < 0.25)
        in2 = ok & (np.abs(ou * e2[0] + ov * e2[1]) < 0.25)
        A1 = np.array([[np.sum(gu * gu * in1), np.sum(gu * gv * in1)], [np.sum(gv * gu * in1), np.sum(gv * gv * in1)]])
        A2 = np.array([[np.sum(gu * gu * in2), np.sum(gu * gv * in2)], [np.sum(gv * gu * in2), np.sum(gv * gv * in2)]])
        e1, e2 = smallest_eigvec(A1), smallest_eigvec(A2)
        V1[i], V2[i] = e1, e2
        U = np.arange(u0, u1 + 1, dtype=np.float64)[None, :] - cu
        W = np.arange(v0, v1_ + 1, dtype=np.float64)[:, None] - cv
        U, W = np.broadcast_to(U, gu.shape), np.broadcast_to(W, gu.shape)
        p1 = U * e1[0] + W * e1[1]
        d1 = np.sqrt((U - p1 * e1[0]) ** 2 + (W - p1 * e1[1]) ** 2)
        p2 = U * e2[0] + W * e2[1]
        d2 = np.sqrt((U - p2 * e2[0]) ** 2 + (W - p2 * e2[1]) ** 2)
        sel = ok & ~((U == 0) & (W == 0)) & (((d1 < 3) & (np.abs(ou * e1[0] + ov * e1[1]) < 0.25)) |
                                             ((d2 < 3) & (np.abs(ou * e2[0] + ov * e2[1]) < 0.25)))
        gu_, gv_ = gu[sel], gv[sel]
        uu, vv = U[sel] + cu, W[sel] + cv
        G = np.array([[np.sum(gu_ * gu_), np.sum(gu_ * gv_)], [np.sum(gu_ * gv_), np.sum(gv_ * gv_)]])
        b = np.array([np.sum(gu_ * gu_ * uu + gu_ * gv_ * vv), np.sum(gu_ * gv_ * uu + gv_ * gv_ * vv)])
        s = np.linalg.svd(G, compute_uv=False)
        if s[1] > 2 * np.spacing(s[0]):
            pn = np.linalg.solve(G, b)
            P[i] = pn
            if math.hypot(pn[0] - cu, pn[1] - cv) >= 4:
                V1[i], V2[i] = 0, 0
        else:
            V1[i], V2[i] = 0, 0
    return P, V1, V2


def correlation_score(img, wt, v1, v2):
    """cornerCorrelationScore.m on one (2r+1)^2 window."""
    n = wt.shape[0]
    c = (n + 1) / 2
    x = np.arange(1, n + 1, dtype=np.float64)[None, :] - c
    y = np.arange(1, n + 1, dtype=np.float64)[:, None] - c
    x, y = np.broadcast_to(x, (n, n)), np.broadcast_to(y, (n, n))
    q1 = x * v1[0] + y * v1[1]
    q2 = x * v2[0] + y * v2[1]
    near = (np.hypot(x - q1 * v1[0], y - q1 * v1[1]) <= 1.5) | (np.hypot(x - q2 * v2[0], y - q2 * v2[1]) <= 1.5)
    f = np.where(near, 1.0, -1.0).reshape(-1, order="F")
    wv = wt.reshape(-1, order="F")
    wv = (wv - wv.mean()) / wv.std(ddof=1)
    f = (f - f.mean()) / f.std(ddof=1)
    g = np.sum(wv * f) / (len(wv) - 1)
    g = g if g > 0 else 0.0                    # MATLAB max(NaN, 0) is 0
    with np.errstate(invalid="ignore"):
        ks = template(math.atan2(v1[1], v1[0]), math.atan2(v2[1], v2[0]), int(c - 1))
    a1, a2, b1, b2 = [np.sum(k * img) for k in ks]
    if not all(np.isfinite([a1, a2, b1, b2])):
        # an empty quadrant divides 0 by 0; MATLAB's max(NaN, 0) then makes the intensity score 0
        return 0.0
    mu = (a1 + a2 + b1 + b2) / 4
    s1 = min(min(a1 - mu, a2 - mu), min(mu - b1, mu - b2))
    s2 = min(min(mu - a1, mu - a2), min(b1 - mu, b2 - mu))
    si = max(max(s1, s2), 0.0)
    return g * si


def score(img, wt, P, V1, V2, radii=RADII):
    """scoreCorners.m: best score over the radii (a radius whose window leaves the image scores 0)."""
    h, w = img.shape
    out = np.zeros(len(P))
    for i in range(len(P)):
        u, v = mround(P[i, 0]), mround(P[i, 1])
        best = None
        for r in radii:
            s = 0.0
            if u > r and u <= w - r and v > r and v <= h - r:
                sl = (slice(v - r - 1, v + r), slice(u - r - 1, u + r))
                s = correlation_score(img[sl], wt[sl], V1[i], V2[i])
            best = s if best is None else max(best, s)
        out[i] = best
    return out


def find_corners(img_u8, tau=SCORE_TAU, stages=False):
    """findCorners(img, tau, 1): 0-based p, v1, v2, score in the reference's order."""
    du_n, dv_n = gradients(img_u8)
    du, dv, ang, wt = angle_weight(du_n, dv_n)
    L = likelihood(img_u8)
    cand, cand_val = nms(L)
    P, V1, V2 = refine(du, dv, ang, wt, cand)
    keep = ~((V1[:, 0] == 0) & (V1[:, 1] == 0))
    P, V1, V2 = P[keep], V1[keep], V2[keep]
    S = score(normalised(img_u8), wt, P, V1, V2)
    keep2 = ~(S < tau)
    P, V1, V2, S = P[keep2], V1[keep2], V2[keep2], S[keep2]
    neg = V1[:, 0] + V1[:, 1] < 0
    V1[neg] = -V1[neg]
    flip = -np.sign(V1[:, 1] * V2[:, 0] - V1[:, 0] * V2[:, 1])
    V2 = V2 * flip[:, None]
    res = dict(p=P - 1, v1=V1, v2=V2, score=S)
    if stages:
        res.update(L=L, cand=cand, cand_val=cand_val, refined_all=refine(du, dv, ang, wt, cand), keep=keep)
    return res
