"""The owner of the context's and the keyframe store's memory, icet::BufferGroup (icet_amd/csrc/icet_buffers.h), on the host: tests/cpp/test_buffer_group.cpp defines
the four icet::mem functions over malloc and refuses the k-th allocation, for every k, of a group of six, of the store's grow-then-swap and of the grow step
(icet::grow) on a one-buffer group and on a pair.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_group_standalone_under_sanitizers(tmp_path):
    """Built plain and with -fsanitize=address,undefined: both run clean (a leak, a second free, a write past a block or a use after release ends the sanitised run)
    and print the same lines, one per case, ending in OK."""
    src = os.path.join(ROOT, "tests", "cpp", "test_buffer_group.cpp")
    outs = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_buffer_group_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", ROOT, src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (name, r.stdout[-2000:], r.stderr[-2000:])
        outs[name] = r.stdout
    assert outs["plain"] == outs["san"] and outs["plain"].endswith(b"OK\n")
    lines = outs["plain"].decode().splitlines()
    assert sum(l.startswith("six, allocation") for l in lines) == 6 and sum(l.startswith("reserve, allocation") for l in lines) == 3
    assert sum(l.startswith("grow one, allocation") for l in lines) == 1 and sum(l.startswith("grow pair, allocation") for l in lines) == 2
