"""The HIP-free rules around the context's staging (icet_amd/csrc/icet_staging.h) on the host: tests/cpp/test_staging.cpp lays host scans out in a staging buffer,
sets and compares the halves of a pair descriptor, lays a call's descriptors out (offsets, segment table, totals), unpacks n x 48 result floats and checks device scans.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_standalone_under_sanitizers(tmp_path):
    """Built plain and with -fsanitize=address,undefined: both run clean (a staged block past its buffer or an unpack past an output ends the sanitised run) and
    print the same lines, one per case, ending in OK."""
    src = os.path.join(ROOT, "tests", "cpp", "test_staging.cpp")
    outs = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_staging_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", ROOT, src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (name, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = r.stdout
    assert outs["plain"] == outs["san"] and outs["plain"].endswith(b"OK\n")
    lines = outs["plain"].decode().splitlines()
    assert sum(l.startswith("layout ") for l in lines) == 7 and sum(l.startswith("scan check: ") for l in lines) == 4
    assert sum(l.startswith("unpack ") for l in lines) == 2 and sum(l.startswith("halves: ") for l in lines) == 1
    assert sum(l.startswith("staging layout: ") for l in lines) == 5
