"""CPU tests of the voxel map's snapshot format (include/icet_hip.h icet_voxel_map_save / _load / _snapshot_info / _merge_device): the header
the library and its kernels compile (icet_amd/csrc/icet_map_snapshot.h), built with g++ into a stand-alone program (tests/cpp/test_map_snapshot.cpp), is held to
itself -- once with -O2 -Wall -Werror, once under AddressSanitizer + UBSan -- and to the NumPy model (tests/map_snapshot_model.py) in both directions; the golden
file pins format version 1; the entry points are exported and refuse NULL; the info record has the size and the offsets of its ctypes mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_model as mm
import map_shape_model as shm
import map_snapshot_model as msm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_map_snapshot.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_snapshot_v1.bin")
NEW_SYMBOLS = ("icet_voxel_map_save", "icet_voxel_map_load", "icet_voxel_map_snapshot_info", "icet_voxel_map_merge_device")


def golden_model():
    """The map of the golden file: a shaped map of a few dozen cells, with a negative cell and an emptied one."""
    rs = np.random.RandomState(27)
    scans = [(rs.randn(160, 3) * [0.8, 0.8, 0.2] + [1.5, 0.5, 0.3]).astype(np.float32) for _ in range(3)]
    poses = np.stack([mm.pose(t=(0.5 * k, 0.25 * k, 0.0), r=(0.0, 0.01, 0.2 * k)) for k in range(3)])
    m = shm.ShapeMap(0.75, min_range=0.25, max_range=6.0).add(scans, poses)
    far = [np.array([[4.0, 4.0, 1.0]], np.float32)]
    return m.add(far, [mm.pose()]).remove(far, [mm.pose()]).remove([np.array([[-4.0, 4.0, 1.0], [-4.0, 4.1, 1.0]], np.float32)], [mm.pose()])


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_snapshot") / "test_map_snapshot")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def prog_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_snapshot_san") / "test_map_snapshot_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("which", ["prog", "prog_san"])
def test_header_round_trips_and_refuses_prefixes_byte_changes_and_bad_contents(which, request, tmp_path):
    exe = request.getfixturevalue(which)
    out = subprocess.run([exe, "selftest"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "map snapshot ok: 8 images" in out.stdout, out.stderr[-2000:]


def _models():
    rs = np.random.RandomState(33)
    scans = [(rs.randn(500, 3) * [3, 3, 0.5]).astype(np.float32) for _ in range(2)]
    poses = np.stack([mm.pose(t=(0.4 * k, 0.0, 0.1), r=(0.0, 0.02, 0.3 * k)) for k in range(2)])
    yield "plain", mm.Map(0.5, 0.5, 9.0).add(scans, poses)
    yield "shaped", shm.ShapeMap(0.5).add(scans, poses)
    yield "negative", shm.ShapeMap(0.5).add(scans[:1], poses[:1]).remove(scans[1:], poses[1:])
    yield "one", mm.Map(0.1).add([np.array([[1, 2, 3]], np.float32)], [mm.pose()])
    yield "empty", shm.ShapeMap(0.1)
    yield "golden", golden_model()


@pytest.mark.parametrize("which", ["prog", "prog_san"])
def test_header_and_model_write_the_same_bytes_both_ways(which, request, tmp_path):
    exe = request.getfixturevalue(which)
    for name, m in _models():                                         # the model's file, parsed and written again by the header
        src, dst = tmp_path / (name + ".vxm"), tmp_path / (name + ".out")
        src.write_bytes(msm.write(m))
        r = subprocess.run([exe, "rewrite", str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)
        assert dst.read_bytes() == src.read_bytes(), name
        img = msm.read(src.read_bytes())
        info = [int(v) for v in subprocess.check_output([exe, "info", str(src)]).split()]
        assert info == [img["cell_bits"], img["min_range_bits"], img["max_range_bits"], int(img["shaped"]), 14 if img["shaped"] else 5, img["keys"].shape[0]] + \
            img["totals"] + [len(src.read_bytes()), msm.checksum(src.read_bytes()[128:])], name
    own = tmp_path / "own.vxm"                                        # the header's file, parsed and written again by the model
    assert subprocess.run([exe, "write", str(own)]).returncode == 0
    img = msm.read(own.read_bytes())
    assert img["keys"].shape == (37,) and img["shaped"] and img["words"][1, 0] == np.uint64((-5) & msm.MASK) and img["words"][2, 0] == 0
    assert msm.write_image(img) == own.read_bytes()
    bad = bytearray(own.read_bytes()); bad[300] ^= 4                  # what the model refuses the header refuses
    (tmp_path / "bad.vxm").write_bytes(bad)
    with pytest.raises(ValueError):
        msm.read(bad)
    assert subprocess.run([exe, "rewrite", str(tmp_path / "bad.vxm"), str(tmp_path / "bad.out")], capture_output=True).returncode == 2


def test_golden_file_pins_format_version_one(prog, tmp_path):
    raw = open(GOLDEN, "rb").read()
    m = golden_model()
    assert msm.write(m) == raw                                        # the model still writes these bytes
    img = msm.read(raw)
    n = img["keys"].shape[0]
    assert 24 <= n <= 96 and len(raw) < 16384 and img["shaped"] and raw[:12] == b"ICETVXM1\x01\x00\x00\x00"
    assert (img["words"][:, 0].astype(np.int64) < 0).sum() == 1 and n == sum(1 for e in m.cells.values() if any(e)) == len(m.cells) - 1
    r = subprocess.run([prog, "rewrite", GOLDEN, str(tmp_path / "g.out")], capture_output=True, text=True)      # the header accepts it
    assert r.returncode == 0 and (tmp_path / "g.out").read_bytes() == raw, r.stderr


def test_snapshot_entry_points_are_exported_and_refuse_null(tmp_path):
    from icet_amd import api
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    B = api.ICET_ERR_BAD_ARG
    info = api.MapSnapshotInfo()
    assert lib.icet_voxel_map_save(None, b"x") == B and lib.icet_voxel_map_load(None, b"x", 1) == B
    assert lib.icet_voxel_map_merge_device(None, None, 1) == B
    assert lib.icet_voxel_map_snapshot_info(None, C.byref(info)) == B and lib.icet_voxel_map_snapshot_info(b"x", None) == B
    assert lib.icet_voxel_map_snapshot_info(os.fsencode(str(tmp_path / "missing.vxm")), C.byref(info)) == B
    with pytest.raises(api.IcetError):
        api.VoxelMap.snapshot_info(str(tmp_path / "missing.vxm"))
    # the library's reader (no device needed) against the model, and against a damaged file
    got = api.VoxelMap.snapshot_info(GOLDEN)
    img = msm.read(open(GOLDEN, "rb").read())
    assert got == dict(cell=0.75, min_range=0.25, max_range=6.0, shaped=True, words_per_entry=14, entries=img["keys"].shape[0], points_in=img["totals"][0],
                       points_kept=img["totals"][1], points_nonfinite=img["totals"][2], points_outside=img["totals"][3], points_dropped=img["totals"][4],
                       file_bytes=os.path.getsize(GOLDEN), payload_checksum=msm.checksum(open(GOLDEN, "rb").read()[128:]))
    bad = bytearray(open(GOLDEN, "rb").read()); bad[200] ^= 1
    (tmp_path / "bad.vxm").write_bytes(bad)
    assert lib.icet_voxel_map_snapshot_info(os.fsencode(str(tmp_path / "bad.vxm")), C.byref(info)) == B


def test_info_record_size_and_offsets_match_the_ctypes_mirror(tmp_path):
    from icet_amd import api
    fields = ("cell", "min_range", "max_range", "shaped", "words_per_entry", "reserved0", "entries", "points_in", "points_kept", "points_nonfinite", "points_outside",
              "points_dropped", "file_bytes", "payload_checksum", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icet_hip.h"\nint main(void){ printf("%d", (int)sizeof(struct icet_voxel_map_snapshot_info));\n'
                   + "".join('printf(" %%d", (int)offsetof(struct icet_voxel_map_snapshot_info, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert got == [C.sizeof(api.MapSnapshotInfo)] + [getattr(api.MapSnapshotInfo, f).offset for f in fields]
    assert got == [96, 0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88]
