"""A NumPy restatement of the rule of a voxel map's visibility evidence (include/icet_hip.h icet_voxel_map_evidence_*; the device compiles
icet_amd/csrc/icet_map_evidence.h), on top of the extract of tests/map_model.py: float64 element-wise for what the rule does in double, the float32 casts where
the rule has them, range words as uint32 and the sums as integers."""
import numpy as np

from map_query_model import pose_ok

EMPTY = np.uint32(0xFFFFFFFF)
NONE, MISS, AGREE, OCCLUDED = 0, 1, 2, 3


def pixel(x, y, z, image_log2):
    """A.3 to A.5 for float64 arrays of directions (not all zero): (u, v) as int64 arrays."""
    W = 1 << int(image_log2)
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    with np.errstate(all="ignore"):
        a = (np.abs(x) + np.abs(y)) + np.abs(z)
        px, py = x / a, y / a
        fx = np.where(px < 0, -(1.0 - np.abs(py)), 1.0 - np.abs(py))
        fy = np.where(py < 0, -(1.0 - np.abs(px)), 1.0 - np.abs(px))
        px, py = np.where(z < 0, fx, px), np.where(z < 0, fy, py)
        fu = np.floor((px + 1.0) * float(W // 2)); fv = np.floor((py + 1.0) * float(W // 2))
        fu = np.where(fu >= 0, np.minimum(fu, W - 1.0), 0.0); fv = np.where(fv >= 0, np.minimum(fv, W - 1.0), 0.0)
    return fu.astype(np.int64), fv.astype(np.int64)


def scan_rows(scan, min_range, image_log2):
    """Per row of ``scan`` (N x 3 float32): takes part (bool), pixel v W + u (int64), range word (uint32).  Pixel and word only mean something for a part-taker."""
    p = np.asarray(scan, np.float32).reshape(-1, 3).astype(np.float64)
    mn = float(np.float32(min_range))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d2 = (x * x + y * y) + z * z
        part = finite & (d2 > mn * mn)
        xs, ys, zs = (np.where(part, v, 1.0) for v in (x, y, z))
        u, v = pixel(xs, ys, zs, image_log2)
        word = np.sqrt(np.where(part, d2, 1.0)).astype(np.float32).view(np.uint32)
    return part, (v << int(image_log2)) + u, word


def range_image(scan, min_range, image_log2):
    """A: the W x W image of range words of one scan (uint32, EMPTY where no row fell), and the rows that took part."""
    W = 1 << int(image_log2)
    part, pix, word = scan_rows(scan, min_range, image_log2)
    img = np.full(W * W, EMPTY, np.uint32)
    np.minimum.at(img, pix[part], word[part])
    return img.reshape(W, W), int(part.sum())


def near_image(img, window):
    """B: the minimum over the window [v - w, v + w] x [u - w, u + w] clipped to the image."""
    w = int(window)
    W = img.shape[0]
    pad = np.full((W + 2 * w, W + 2 * w), EMPTY, np.uint32)
    pad[w:w + W, w:w + W] = img
    out = np.full((W, W), EMPTY, np.uint32)
    for dv in range(2 * w + 1):
        for du in range(2 * w + 1):
            out = np.minimum(out, pad[dv:dv + W, du:du + W])
    return out


def cell_pixels(cents, pose, min_range, max_range, image_log2):
    """C.2 to C.4 for centroids (N x 3 float32) against a usable pose: takes part (bool), pixel (int64), d2 (float64)."""
    m = np.asarray(cents, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    mn, mx = float(np.float32(min_range)), float(np.float32(max_range))
    with np.errstate(all="ignore"):
        d = m - T[:3, 3][None, :]
        p = [(T[0, a] * d[:, 0] + T[1, a] * d[:, 1]) + T[2, a] * d[:, 2] for a in range(3)]
        d2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
        part = (d2 > mn * mn) & (d2 <= mx * mx)
        u, v = pixel(*(np.where(part, q, 1.0) for q in p), image_log2)
    return part, (v << int(image_log2)) + u, d2


def classes(d2, near, margin):
    """C.5: the class per (d2, near word)."""
    d2 = np.asarray(d2, np.float64); near = np.asarray(near, np.uint32)
    mg = float(np.float32(margin))
    with np.errstate(all="ignore"):
        rc = np.sqrt(d2)
        rn = near.view(np.float32).astype(np.float64)
        cls = np.where(rn > rc + mg, MISS, np.where(rn >= rc - mg, AGREE, OCCLUDED))
    return np.where(near == EMPTY, NONE, cls)


def cell_classes(cents, pose, near, min_range, max_range, margin, image_log2):
    """C: per centroid the class against the scan with near image ``near`` (W x W uint32) at ``pose``."""
    n = np.asarray(cents).reshape(-1, 3).shape[0]
    if not pose_ok(pose):
        return np.zeros(n, np.int64)
    part, pix, d2 = cell_pixels(cents, pose, min_range, max_range, image_log2)
    cls = classes(d2, np.asarray(near, np.uint32).reshape(-1)[pix], margin)
    return np.where(part, cls, NONE)


def decide(miss, agree, min_miss, agree_factor):
    """D, in Python integers: no product overflows."""
    need = max(1, int(min_miss))
    return np.array([int(m) >= need and int(m) > int(agree_factor) * int(a) for m, a in zip(miss, agree)], bool).reshape(-1)


def evidence_extract(ext, scans, poses, max_range, margin, min_range=0.0, image_log2=8, window=1, min_miss=2, agree_factor=1):
    """The evidence of an extract at min_points 1 (tests/map_model.py Map.extract()): dict(miss, agree (int32), transient (uint8), key, stats)."""
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    assert len(scans) == poses.shape[0] and max_range > 0 and margin >= 0 and 4 <= image_log2 <= 10 and window in (0, 1, 2)
    cents = np.asarray(ext["xyz"], np.float32).reshape(-1, 3)
    n = cents.shape[0]
    miss = np.zeros(n, np.int64); agree = np.zeros(n, np.int64)
    rows, bad = 0, 0
    for scan, T in zip(scans, poses):
        img, r = range_image(scan, min_range, image_log2)
        rows += r
        if not pose_ok(T):
            bad += 1
            continue
        cls = cell_classes(cents, T, near_image(img, window), min_range, max_range, margin, image_log2)
        miss += cls == MISS; agree += cls == AGREE
    tr = decide(miss, agree, min_miss, agree_factor)
    stats = dict(rows_imaged=rows, cells=n, cells_transient=int(tr.sum()), scans_used=len(scans) - bad, scans_bad_pose=bad)
    return dict(miss=miss.astype(np.int32), agree=agree.astype(np.int32), transient=tr.astype(np.uint8), key=np.asarray(ext["key"], np.uint64).copy(), stats=stats)


def evidence(model, scans, poses, max_range, margin=None, **kw):
    """evidence_extract on a map_model.Map; margin None: three cells."""
    mg = 3.0 * float(np.float32(model.cell)) if margin is None else margin
    return evidence_extract(model.extract(1), scans, poses, max_range, mg, **kw)


def static_extract(ext, ev):
    """The extract without its transient cells."""
    keep = np.asarray(ev["transient"]) == 0
    return dict(xyz=ext["xyz"][keep], count=ext["count"][keep], key=ext["key"][keep])
