"""CPU tests of the voxel map's snapshot MODEL (tests/map_snapshot_model.py): what the format promises of a file -- every word comes back,
the bytes are a function of the map's contents alone, an emptied cell is absent and a negative one present, and maps are additive file by file.  These measure
the model, never the device code; the device is held to the model byte for byte in tests/test_map_snapshot.py."""
import numpy as np
import pytest

import map_model as mm
import map_shape_model as shm
import map_snapshot_model as msm

CELL = 0.5


def _scans(n=4, rows=600, seed=31):
    rs = np.random.RandomState(seed)
    scans = [(rs.randn(rows, 3) * [3, 3, 0.5]).astype(np.float32) for _ in range(n)]
    poses = np.stack([mm.pose(t=(0.4 * k, -0.3 * k, 0.1), r=(0.01, 0.02, 0.25 * k)) for k in range(n)])
    return scans, poses


def _new(shaped, **kw):
    return (shm.ShapeMap if shaped else mm.Map)(CELL, **kw)


@pytest.mark.parametrize("shaped", [False, True])
def test_write_then_read_returns_every_word(shaped):
    scans, poses = _scans()
    m = _new(shaped, min_range=0.5, max_range=9.0).add(scans, poses)
    raw = msm.write(m)
    img = msm.read(raw)
    W = 14 if shaped else 5
    assert len(raw) == 128 + 8 * W * ((len(m.cells) + 1) & ~1) and len(raw) % 16 == 0
    assert img["shaped"] == shaped and img["words"].shape == (len(m.cells), W - 1) and len(m.cells) > 100
    assert [msm.unbits(img[k]) for k in ("cell_bits", "min_range_bits", "max_range_bits")] == [0.5, 0.5, 9.0]
    assert img["totals"] == [m.totals[t] for t in msm.TOTALS] and m.totals["points_in"] == 2400 > m.totals["points_kept"] > 0
    assert list(img["keys"]) == sorted(m.cells)
    for k, w in zip(img["keys"], img["words"]):
        assert [int(v) for v in w[:4]] == m.cells[int(k)]
        if shaped:
            assert [int(v) for v in w[4:]] == m.words(k)
    assert msm.write_image(img) == raw
    assert msm.write(_new(shaped)) == msm.write_image(msm.read(msm.write(_new(shaped)))) and len(msm.write(_new(shaped))) == 128


@pytest.mark.parametrize("shaped", [False, True])
def test_the_bytes_do_not_depend_on_the_order_of_the_scans(shaped):
    scans, poses = _scans()
    want = msm.write(_new(shaped).add(scans, poses))
    assert msm.write(_new(shaped).add(scans[::-1], poses[::-1])) == want
    one_by_one = _new(shaped)
    for k in (2, 0, 3, 1):
        one_by_one.add(scans[k:k + 1], poses[k:k + 1])
    assert msm.write(one_by_one) == want


@pytest.mark.parametrize("shaped", [False, True])
def test_an_emptied_cell_is_absent_and_a_negative_cell_is_present(shaped):
    scans, poses = _scans()
    a = _new(shaped).add(scans[:2], poses[:2])
    both = _new(shaped).add(scans, poses).remove(scans[2:], poses[2:])
    assert len(both.cells) > len(a.cells)                             # the removed scans' own cells are still keys of the model, all zero
    img = msm.read(msm.write(both))
    assert list(img["keys"]) == sorted(a.cells)
    assert img["words"].tobytes() == msm.read(msm.write(a))["words"].tobytes()
    assert img["totals"][0] == 3 * a.totals["points_in"] and img["totals"][1] == a.totals["points_kept"]      # a remove keeps counting the rows it reads: 4 + 2 scans
    neg = _new(shaped).remove(scans[:1], poses[:1])
    img = msm.read(msm.write(neg))
    assert list(img["keys"]) == sorted(neg.cells) and (img["words"][:, 0].astype(np.int64) < 0).all()
    # a zero count beside non-zero sums: one row added at an offset, one removed at another offset of the same cell
    z = _new(shaped).add([np.array([[0.1, 0.1, 0.1]], np.float32)], [mm.pose()]).remove([np.array([[0.3, 0.2, 0.4]], np.float32)], [mm.pose()])
    img = msm.read(msm.write(z))
    assert img["keys"].shape == (1,) and img["words"][0, 0] == 0 and img["words"][0, 1:4].all()


@pytest.mark.parametrize("shaped", [False, True])
def test_files_are_additive_and_minus_one_gives_the_first_file_back(shaped):
    scans, poses = _scans(8)
    a, b = _new(shaped).add(scans[:4], poses[:4]), _new(shaped).add(scans[4:], poses[4:])
    fa, fb = msm.write(a), msm.write(b)
    c = msm.merge(msm.merge(_new(shaped), msm.read(fa)), msm.read(fb))
    assert msm.write(c) == msm.write(_new(shaped).add(scans, poses))
    assert set(a.cells) & set(b.cells) and set(b.cells) - set(a.cells)
    assert msm.write(msm.merge(c, msm.read(fb), -1)) == fa            # totals in the header included: all five are subtracted
    if shaped:
        plain = msm.merge(mm.Map(CELL), msm.read(fa))                 # a shaped file into a plain map: the moment columns are left out
        assert msm.write(plain) == msm.write(mm.Map(CELL).add(scans[:4], poses[:4]))
    else:
        with pytest.raises(ValueError):
            msm.merge(shm.ShapeMap(CELL), msm.read(fa))
    with pytest.raises(ValueError):
        msm.merge(_new(shaped).__class__(0.25), msm.read(fa))


def test_the_reader_refuses_what_the_format_forbids():
    scans, poses = _scans(2)
    img = msm.image_of(shm.ShapeMap(CELL).add(scans, poses))
    img["keys"], img["words"] = img["keys"][:37], img["words"][:37]
    raw = msm.write_image(img)
    assert msm.read(raw)["keys"].shape == (37,)
    for cut in (0, 64, 127, 128, len(raw) - 8):
        with pytest.raises(ValueError):
            msm.read(raw[:cut])
    rs = np.random.RandomState(5)
    for at in list(range(128)) + list(rs.randint(128, len(raw), 200)):
        bad = bytearray(raw); bad[at] ^= 1 << rs.randint(8)
        with pytest.raises(ValueError):
            msm.read(bad)

    def broken(**kw):
        j = dict(img); j.update(kw)
        return j
    k = img["keys"].copy(); k[[3, 4]] = k[[4, 3]]
    w0 = img["words"].copy(); w0[5] = 0
    kz = img["keys"].copy(); kz[0] &= ~np.uint64(0x1FFFFF)
    kh = img["keys"].copy(); kh[-1] |= np.uint64(1 << 63)
    for j in (broken(keys=k), broken(words=w0), broken(keys=kz), broken(keys=kh)):
        with pytest.raises(ValueError):
            msm.read(msm.write_image(j))
    for lies in (dict(flags=0), dict(words=5), dict(n=36), dict(n=39), dict(n=(1 << 30) + 1), dict(reserved=1), dict(file_bytes=len(raw) + 16)):
        with pytest.raises(ValueError):
            msm.read(msm.write_image(img, **lies))
