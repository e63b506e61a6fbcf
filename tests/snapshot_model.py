"""A NumPy model of the keyframe-store snapshot file, written from the format's description and not from icet_snapshot.h: a writer,
a reader and a validator.  tests/test_snapshot.py holds the library and the stand-alone C++ program against it, in both directions.

Little-endian.  header 160 B | directory n x 128 B | payloads back to back.  Every part of a payload is padded with zero bytes to 16.
An image is described by a dict:
    shape = dict(bins_phi, bins_theta, n, thresh_bits, buff_bits, flags), layout_version,
    appearance / coarse = the 8 uint32 words of the parameter block, or None,
    entries = [dict(slot, stamp, pose = 12 uint32 words or None, hot (ns, 12) uint32, fit (ns, 20) uint32, sov (V + 1 & ~1) int16,
                    desc (A * Rp) uint32 and weights (A) uint32, or None; grid (G * G / 32) uint32 or None)], ascending slots.
"""
import numpy as np

MAGIC = b"ICETKFS1"
HEADER, ENTRY = 160, 128
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
U64 = np.uint64


def checksum(raw):
    """sum_i mix(w_i + (i + 1) GOLDEN) mod 2^64 over the little-endian u64 words of raw (wrapping uint64 arithmetic); mix: the splitmix64 finaliser."""
    w = np.frombuffer(bytes(raw), "<u8")
    with np.errstate(over="ignore"):
        z = w + (np.arange(1, w.size + 1, dtype=np.uint64) * GOLDEN)
        z ^= z >> U64(30); z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27); z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        return int(np.add.reduce(z, dtype=np.uint64)) if w.size else 0


def _pad16(b):
    return b + bytes(-len(b) % 16)


def _payload(e):
    ns = len(e["hot"])
    assert e["hot"].shape == (ns, 12) and e["fit"].shape == (ns, 20)
    b = np.ascontiguousarray(e["hot"], "<u4").tobytes() + np.ascontiguousarray(e["fit"], "<u4").tobytes() + _pad16(np.ascontiguousarray(e["sov"], "<i2").tobytes())
    if e.get("desc") is not None:
        b += _pad16(np.ascontiguousarray(e["desc"], "<u4").tobytes()) + _pad16(np.ascontiguousarray(e["weights"], "<u4").tobytes())
    if e.get("grid") is not None:
        b += np.ascontiguousarray(e["grid"], "<u4").tobytes()
    return b


def write(img):
    """The file's bytes."""
    sh, ents = img["shape"], img["entries"]
    V = sh["bins_phi"] * sh["bins_theta"]
    pay = [_payload(e) for e in ents]
    at = HEADER + ENTRY * len(ents)
    d = b""
    for e, p in zip(ents, pay):
        flags = (1 if e.get("pose") is not None else 0) | (2 if e.get("desc") is not None else 0) | (4 if e.get("grid") is not None else 0)
        pose = np.asarray(e["pose"], "<u4") if e.get("pose") is not None else np.full(12, 0xFFFFFFFF, "<u4")
        rec = np.array([e["slot"], len(e["hot"]), flags, 0], "<i4").tobytes() + np.array([e["stamp"]], "<i8").tobytes() + pose.tobytes()
        rec += np.array([at, len(p), checksum(p)], "<u8").tobytes() + bytes(32)
        assert len(rec) == ENTRY
        d += rec
        at += len(p)
    feat = (1 if img.get("appearance") is not None else 0) | (2 if img.get("coarse") is not None else 0)
    blk = lambda w: np.asarray(w, "<u4").tobytes() if w is not None else bytes(32)
    h = MAGIC + np.array([1, HEADER, sh["bins_phi"], sh["bins_theta"], sh["n"]], "<i4").tobytes() + np.array([sh["thresh_bits"], sh["buff_bits"], sh["flags"]], "<u4").tobytes()
    h += np.array([V, 48, 80, img["layout_version"], len(ents), feat], "<u4").tobytes() + blk(img.get("appearance")) + blk(img.get("coarse"))
    h += np.array([at], "<u8").tobytes()
    assert len(h) == 136
    front = h + bytes(8) + bytes(16) + d
    front = front[:136] + np.array([checksum(front)], "<u8").tobytes() + front[144:]
    return front + b"".join(pay)


class Refused(ValueError):
    pass


def _need(ok, why):
    if not ok:
        raise Refused(why)


def read(raw, layout_version=1):
    """The image dict of a file's bytes, after every check of the format; Refused otherwise.  Also returns, per entry, ``sum`` (the stored payload checksum)."""
    raw = bytes(raw)
    _need(len(raw) >= HEADER and raw[:8] == MAGIC, "magic")
    i4 = lambda o, n=1: np.frombuffer(raw, "<i4", n, o)
    u4 = lambda o, n=1: np.frombuffer(raw, "<u4", n, o)
    u8 = lambda o, n=1: np.frombuffer(raw, "<u8", n, o)
    _need(i4(8)[0] == 1 and i4(12)[0] == HEADER, "version / header size")
    bins_phi, bins_theta, n = (int(v) for v in i4(16, 3))
    thresh_bits, buff_bits, flags = (int(v) for v in u4(28, 3))
    V, hot_b, fit_b, lv, n_ent, feat = (int(v) for v in u4(40, 6))
    _need(hot_b == 48 and fit_b == 80 and lv == layout_version, "record sizes / layout version")
    _need(bins_phi >= 1 and bins_theta >= 1 and n >= 1 and bins_phi * bins_theta == V and V <= 10000 and not flags & ~10 and not feat & ~3, "shape")
    _need(raw[144:160] == bytes(16), "reserved header bytes")
    app = u4(64, 8).copy() if feat & 1 else None
    coarse = u4(96, 8).copy() if feat & 2 else None
    _need(feat & 1 or raw[64:96] == bytes(32), "appearance block without its bit")
    _need(feat & 2 or raw[96:128] == bytes(32), "coarse block without its bit")
    if app is not None:
        _need(8 <= app[0] <= 360 and app[0] % 2 == 0 and 1 <= app[1] <= 64 and not app[5:].any(), "appearance parameters")
    if coarse is not None:
        _need(64 <= coarse[0] <= 512 and coarse[0] % 32 == 0 and not coarse[5:].any(), "coarse parameters")
    size = int(u8(128)[0])
    _need(size == len(raw), "file size")
    _need(n_ent <= (len(raw) - HEADER) // ENTRY, "entry count")
    end = HEADER + ENTRY * n_ent
    _need(checksum(raw[:136] + bytes(8) + raw[144:end]) == int(u8(136)[0]), "header / directory checksum")
    A, Rp = (int(app[0]), (int(app[1]) + 3) // 4) if app is not None else (0, 0)
    G = int(coarse[0]) if coarse is not None else 0
    row = (V + 1) & ~1
    at, prev, ents = end, -1, []
    for k in range(n_ent):
        o = HEADER + ENTRY * k
        slot, ns, fl, rsv = (int(v) for v in i4(o, 4))
        stamp = int(np.frombuffer(raw, "<i8", 1, o + 16)[0])
        pose = u4(o + 24, 12).copy()
        off, nbytes, csum = (int(v) for v in u8(o + 72, 3))
        _need(rsv == 0 and raw[o + 96:o + 128] == bytes(32), "reserved directory bytes")
        _need(slot > prev, "slots ascending"); prev = slot
        _need(0 <= ns <= V and not fl & ~7, "n_slots / flags")
        _need(not fl & 2 or app is not None, "descriptor without parameters")
        _need(not fl & 4 or coarse is not None, "grid without parameters")
        _need(bool(fl & 1) != bool((pose == 0xFFFFFFFF).all()), "pose flag")
        parts = [48 * ns, 80 * ns, 2 * row] + ([4 * A * Rp, 4 * A] if fl & 2 else []) + ([G * G // 8] if fl & 4 else [])
        want = sum(p + (-p % 16) for p in parts)
        _need(off % 16 == 0 and off == at and nbytes == want and off + nbytes <= len(raw), "payload offset / size")
        at += nbytes
        p = raw[off:off + nbytes]
        _need(checksum(p) == csum, "payload checksum")
        cur = [0]

        def take(nb, dt):
            a = np.frombuffer(p, dt, nb // np.dtype(dt).itemsize, cur[0]).copy()
            _need(p[cur[0] + nb:cur[0] + nb + (-nb % 16)] == bytes(-nb % 16), "padding")
            cur[0] += nb + (-nb % 16)
            return a
        e = dict(slot=slot, stamp=stamp, pose=pose if fl & 1 else None, hot=take(48 * ns, "<u4").reshape(ns, 12), fit=take(80 * ns, "<u4").reshape(ns, 20),
                 sov=take(2 * row, "<i2"), sum=csum)
        if fl & 2:
            e["desc"] = take(4 * A * Rp, "<u4"); e["weights"] = take(4 * A, "<u4")
        if fl & 4:
            e["grid"] = take(G * G // 8, "<u4")
        sov = e["sov"][:V]
        _need(((sov >= -1) & (sov < ns)).all(), "slot_of_voxel range")
        for rec, col in ((e["hot"], 9), (e["fit"], 19)):
            v = rec[:, col].view("<i4") if ns else np.zeros(0, "<i4")
            _need(((v >= 0) & (v < V)).all(), "voxel range")
            _need((sov[v] == np.arange(ns)).all(), "slot_of_voxel[voxel_i] == i")
        ents.append(e)
    _need(at == len(raw), "sizes add up")
    return dict(shape=dict(bins_phi=bins_phi, bins_theta=bins_theta, n=n, thresh_bits=thresh_bits, buff_bits=buff_bits, flags=flags), layout_version=lv,
                appearance=app, coarse=coarse, entries=ents)


def pack_descriptor(D):
    """(rings, sectors) uint8 -> the store's row: per sector Rp = ceil(rings / 4) words, byte r & 3 of word r >> 2 is ring r."""
    rings, A = D.shape
    Rp = (rings + 3) // 4
    b = np.zeros((A, Rp * 4), np.uint8)
    b[:, :rings] = D.T
    return b.view("<u4").reshape(A * Rp)


def synthetic(V_shape=(7, 3), n_slots=(0, 1, 21), app=None, coarse=None, seed=0, slots=None):
    """A valid image with random record contents (a 64-bit LCG), entry k holding n_slots[k] records."""
    state = [seed * 2654435761 + 12345 & (2 ** 64 - 1)]

    def rnd():
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (state[0] >> 32) & 0xFFFFFFFF
    V = V_shape[0] * V_shape[1]
    img = dict(shape=dict(bins_phi=V_shape[1], bins_theta=V_shape[0], n=25, thresh_bits=0x3DCCCCCD, buff_bits=0x3DCCCCCD, flags=0), layout_version=1,
               appearance=np.array(app, "<u4") if app is not None else None, coarse=np.array(coarse, "<u4") if coarse is not None else None, entries=[])
    for k, ns in enumerate(n_slots):
        hot = np.array([[rnd() for _ in range(12)] for _ in range(ns)], "<u4").reshape(ns, 12)
        fit = np.array([[rnd() for _ in range(20)] for _ in range(ns)], "<u4").reshape(ns, 20)
        sov = np.full((V + 1) & ~1, -1, "<i2")
        for i in range(ns):                                      # record i sits in voxel (7 i + k) mod V: distinct voxels where 7 and V are coprime
            v = (i * 7 + k) % V if np.gcd(7, V) == 1 else (i + k) % V
            hot[i, 9] = v; fit[i, 19] = v; sov[v] = i
        e = dict(slot=3 * k + 1 if slots is None else slots[k], stamp=1000 + k if k % 2 == 0 else -1, pose=np.array([rnd() & 0x7FFFFFFF for _ in range(12)], "<u4") if k % 2 == 0 else None,
                 hot=hot, fit=fit, sov=sov)
        if app is not None and k != 1:
            A, Rp = int(app[0]), (int(app[1]) + 3) // 4
            e["desc"] = np.array([rnd() for _ in range(A * Rp)], "<u4"); e["weights"] = np.array([rnd() for _ in range(A)], "<u4")
        if coarse is not None and k != 0:
            G = int(coarse[0])
            e["grid"] = np.array([rnd() for _ in range(G * G // 32)], "<u4")
        img["entries"].append(e)
    return img
