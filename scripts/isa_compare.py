#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of the library, function by function.

    isa_compare.py OLD_OBJ_DIR NEW_OBJ_DIR

Each directory holds the objects of one build (icet_amd/lib/obj, or `make OUT=...`'s obj/).  For every object present in both, the
gfx950 code object is taken out of the .hip_fatbin section, disassembled with llvm-objdump and cut into functions; addresses and
encodings are dropped and the pc-relative targets of calls (s_getpc_b64 + s_add_u32 / s_addc_u32) are replaced by the callee's name,
so that code which merely moved compares equal; the s_nop padding behind a function's last instruction is dropped too (the last
function of a section is padded to the section's end, and stops being the last when kernels are added behind it).  The kernels'
resource metadata (registers, LDS, scratch, kernel-argument size) is compared too.  Functions found in only one build are listed (new kernels are expected there); exit status 1 when a function present
in both differs.  Runs on any machine with ROCm's LLVM tools: no GPU needed.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, tmp):
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, "junk.o")], stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co, "--unbundle"])
    return co


def functions(co):
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    starts, funcs, cur, body = {}, {}, None, []
    lines = txt.split("\n")
    for l in lines:
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", l)
        if m:
            starts[int(m.group(1), 16)] = m.group(2)
    ordered = sorted(starts)

    def name_at(addr):
        lo = None
        for a in ordered:
            if a <= addr:
                lo = a
        return starts.get(lo, "?") + ("" if lo == addr else "+%#x" % (addr - lo if lo is not None else 0))
    pending = None                                   # (address of s_getpc_b64, low half) while resolving a call target
    for l in lines:
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", l)
        if m:
            if cur:
                funcs[cur] = body
            cur, body, pending = m.group(2), [], None
            continue
        if cur is None or not l.startswith("\t"):
            continue
        ins, _, comment = l.strip().partition("//")
        ins = " ".join(ins.split())
        addr = re.match(r"\s*([0-9A-Fa-f]+):", comment)
        addr = int(addr.group(1), 16) if addr else None
        if ins.startswith("s_getpc_b64"):
            pending = [addr, None]
        elif pending and ins.startswith("s_add_u32") and pending[1] is None:
            lit = ins.split(",")[-1].strip()
            try:
                pending[1] = int(lit, 0) & 0xFFFFFFFF
                ins = re.sub(r",[^,]*$", ", <lo>", ins)
            except ValueError:
                pending = None
        elif pending and pending[1] is not None and ins.startswith("s_addc_u32"):
            lit = ins.split(",")[-1].strip()
            try:
                hi = int(lit, 0) & 0xFFFFFFFF
                off = (hi << 32) | pending[1]
                if off >= 1 << 63:
                    off -= 1 << 64
                ins = re.sub(r",[^,]*$", ", <hi of %s>" % name_at(pending[0] + 4 + off), ins)
            except ValueError:
                pass
            pending = None
        body.append(ins)
    if cur:
        funcs[cur] = body
    for body in funcs.values():                      # the s_nop padding behind a function's last instruction (the section's last function carries the most)
        while body and body[-1] == "s_nop 0":
            body.pop()
    return funcs


def kernel_meta(co):
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    meta, cur, name = {}, {}, None
    keys = (".group_segment_fixed_size", ".kernarg_segment_size", ".private_segment_fixed_size", ".sgpr_count", ".vgpr_count", ".agpr_count",
            ".sgpr_spill_count", ".vgpr_spill_count", ".max_flat_workgroup_size")
    for l in txt.split("\n"):                      # a kernel's keys come in alphabetical order: .agpr_count ... .symbol ... .wavefront_size
        s = l.strip().lstrip("- ").strip()
        k, _, v = s.partition(":")
        if k in keys:
            cur[k] = v.strip()
        elif k == ".symbol":
            name = v.strip()[:-3] if v.strip().endswith(".kd") else v.strip()
        elif k == ".wavefront_size" and name:
            meta[name] = dict(cur)
            cur, name = {}, None
    return meta


def main():
    if len(sys.argv) < 3:
        print(__doc__)
        return 2
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    objs = sorted(f for f in os.listdir(old_dir) if f.endswith(".o") and os.path.exists(os.path.join(new_dir, f)))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in objs:
            ta, tb = os.path.join(tmp, "old"), os.path.join(tmp, "new")
            os.makedirs(ta, exist_ok=True); os.makedirs(tb, exist_ok=True)
            try:
                ca, cb = code_object(os.path.join(old_dir, f), ta), code_object(os.path.join(new_dir, f), tb)
            except subprocess.CalledProcessError:
                continue                              # host-only object
            fa, fb = functions(ca), functions(cb)
            ma, mb = kernel_meta(ca), kernel_meta(cb)
            same = [n for n in fa if n in fb and fa[n] == fb[n]]
            diff = [n for n in fa if n in fb and fa[n] != fb[n]]
            mdiff = [n for n in ma if n in mb and ma[n] != mb[n]]
            only_old = [n for n in fa if n not in fb]
            only_new = [n for n in fb if n not in fa]
            print("%-22s %4d functions identical, %d differ, %d kernels' metadata differ, %d only in old, %d only in new"
                  % (f, len(same), len(diff), len(mdiff), len(only_old), len(only_new)))
            for n in diff:
                print("    DIFFERS   %s (%d vs %d instructions)" % (n, len(fa[n]), len(fb[n])))
            for n in mdiff:
                print("    METADATA  %s: %s -> %s" % (n, ma[n], mb[n]))
            for n in only_old:
                print("    only old  %s" % n)
            for n in only_new:
                print("    only new  %s" % n)
            bad += len(diff) + len(mdiff) + len(only_old)
    print("RESULT:", "every function of the old build is unchanged" if bad == 0 else "%d differences" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
