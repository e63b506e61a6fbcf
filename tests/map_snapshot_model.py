"""A NumPy model of the voxel map's snapshot file, written from the format's description and not from icet_map_snapshot.h: a writer, a
reader / validator, and the merge of a file into a model map.  It works on map_model.Map / map_shape_model.ShapeMap, which hold key -> integer words.

Little-endian.  header 128 B | W columns of n u64 words, a column of odd length padded with one zero word.  W = 5 (key, count, sum x, sum y, sum z) or, shaped,
14 (and S_x S_y S_z M_xx M_xy M_xz M_yy M_yz M_zz).  An image is a dict:
    cell_bits, min_range_bits, max_range_bits (uint32 bit patterns), shaped, totals (the five running totals, Python integers),
    keys (n,) uint64 strictly ascending, words (n, W - 1) uint64 (two's complement).
"""
import numpy as np

import snapshot_model as sm

MAGIC = b"ICETVXM1"
HEADER = 128
MASK = (1 << 64) - 1
TOTALS = ("points_in", "points_kept", "points_nonfinite", "points_outside", "points_dropped")
MAX_ENTRIES = 1 << 30

checksum = sm.checksum


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def unbits(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def image_of(model, shaped=None):
    """The image of a model map: every key with a non-zero word, ascending.  shaped: by default whether the model carries moments."""
    if shaped is None:
        shaped = hasattr(model, "mom")
    rows = []
    for k in sorted(model.cells):
        w = [int(v) & MASK for v in model.cells[k]]
        if shaped:
            w += [int(v) & MASK for v in model.mom.get(k, [0] * 9)]
        if any(w):
            rows.append((k, w))
    W = 14 if shaped else 5
    return dict(cell_bits=bits(model.cell), min_range_bits=bits(model.min_range), max_range_bits=bits(model.max_range), shaped=bool(shaped),
                totals=[int(model.totals[t]) for t in TOTALS], keys=np.array([k for k, _ in rows], np.uint64),
                words=np.array([w for _, w in rows], np.uint64).reshape(len(rows), W - 1))


def payload(img):
    n = img["keys"].shape[0]
    cols = [np.asarray(img["keys"], "<u8")] + [np.ascontiguousarray(img["words"][:, c], "<u8") for c in range(img["words"].shape[1])]
    pad = bytes(8) if n & 1 else b""
    return b"".join(c.tobytes() + pad for c in cols)


def header(img, pay, flags=None, words=None, n=None, file_bytes=None, reserved=0):
    """The sealed header for a payload; the keyword arguments let a test write a header that lies."""
    W = img["words"].shape[1] + 1
    h = MAGIC + np.array([1, HEADER, img["cell_bits"], img["min_range_bits"], img["max_range_bits"], (1 if img["shaped"] else 0) if flags is None else flags,
                          W if words is None else words, reserved], "<u4").tobytes()
    h += np.array([img["keys"].shape[0] if n is None else n], "<u8").tobytes()
    h += np.array([t & MASK for t in img["totals"]], "<u8").tobytes()
    h += np.array([HEADER + len(pay) if file_bytes is None else file_bytes, checksum(pay), 0], "<u8").tobytes() + bytes(16)
    assert len(h) == HEADER
    return h[:104] + np.array([checksum(h)], "<u8").tobytes() + h[112:]


def write_image(img, **lies):
    pay = payload(img)
    return header(img, pay, **lies) + pay


def write(model, shaped=None):
    """The file's bytes for a model map."""
    return write_image(image_of(model, shaped))


def read(raw):
    """The image of a file's bytes; ValueError names the first check that fails."""
    raw = bytes(raw)

    def need(ok, why):
        if not ok:
            raise ValueError(why)
    need(len(raw) >= HEADER, "shorter than a header")
    need(raw[:8] == MAGIC, "magic")
    u4 = np.frombuffer(raw[8:40], "<u4")
    need(u4[0] == 1, "version")
    need(u4[1] == HEADER, "header size")
    flags, W = int(u4[5]), int(u4[6])
    need(flags in (0, 1), "flags")
    need(W == (14 if flags else 5), "words per entry against the shaped flag")
    need(u4[7] == 0 and raw[112:128] == bytes(16), "reserved bytes")
    u8 = np.frombuffer(raw[40:112], "<u8")
    n, size = int(u8[0]), int(u8[6])
    need(n <= MAX_ENTRIES, "entries")
    need(size == len(raw), "file size")
    cw = (n + 1) & ~1
    need(len(raw) - HEADER == 8 * W * cw, "size against the columns")
    need(checksum(raw[:104] + bytes(8) + raw[112:128]) == int(u8[8]), "header checksum")
    pay = raw[HEADER:]
    need(checksum(pay) == int(u8[7]), "payload checksum")
    cols = np.frombuffer(pay, "<u8").reshape(W, cw)
    need(not cols[:, n:].any(), "padding")
    keys, words = cols[0, :n].copy(), np.ascontiguousarray(cols[1:, :n].T)
    need(not (keys >> np.uint64(63)).any(), "a key of 2^63 or above")
    for a in range(3):
        need((((keys >> np.uint64(21 * a)) & np.uint64(0x1FFFFF)) >= 1).all(), "a zero key field")
    need((keys[1:] > keys[:-1]).all(), "keys not strictly ascending")
    need(words.any(axis=1).all(), "an all-zero entry")
    signed = np.frombuffer(raw[48:88], "<i8")
    return dict(cell_bits=int(u4[2]), min_range_bits=int(u4[3]), max_range_bits=int(u4[4]), shaped=bool(flags), totals=[int(t) for t in signed], keys=keys, words=words)


def _signed(w):
    w = int(w)
    return w - (1 << 64) if w >> 63 else w


def merge(model, img, sign=1):
    """The words and totals of an image into a model map, times sign: what a load does.  A shaped image into a plain model leaves the moments out; a plain image
    into a shaped model is refused."""
    shaped = hasattr(model, "mom")
    if img["cell_bits"] != bits(model.cell):
        raise ValueError("cell mismatch")
    if shaped and not img["shaped"]:
        raise ValueError("a plain file into a shaped map")
    for k, w in zip(img["keys"], img["words"]):
        vals = [_signed(v) for v in w]
        if not any(vals[:13 if shaped else 4]):
            continue
        e = model.cells.setdefault(int(k), [0, 0, 0, 0])
        for j in range(4):
            e[j] += sign * vals[j]
        if shaped:
            mo = model.mom.setdefault(int(k), [0] * 9)
            for j in range(9):
                mo[j] += sign * vals[4 + j]
    for t, v in zip(TOTALS, img["totals"]):
        model.totals[t] += sign * v
    return model
