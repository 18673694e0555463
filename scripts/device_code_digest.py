#!/usr/bin/env python3
"""One line per GPU kernel of every .hip unit of a csrc directory: what a host-side refactor must leave unchanged.

    python scripts/device_code_digest.py [--csrc DIR] [--units a.hip b.hip] [--keep DIR] > digest.txt

Each unit's device side is compiled alone (the Makefile's FLAGS + --cuda-device-only --no-gpu-bundle-output -c: a plain
gfx950 ELF, no GPU needed).  Line: unit, kernel, code bytes, sha256 of the function's bytes (first 16 hex digits), vgpr_count,
sgpr_count, group_segment_fixed_size, private_segment_fixed_size (the last four from the code object's metadata note).
Two trees are compared with `diff` of their sorted outputs.  --keep leaves the ELFs in DIR (to disassemble a kernel that differs).
The script digests only; it looks for nothing in the code.
"""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def make_flags(csrc):
    out = subprocess.run(["make", "-s", "-C", csrc, "--eval", "print-flags: ; @echo $(HIPCC) $(FLAGS)", "print-flags"],
                         check=True, capture_output=True, text=True).stdout.split()
    return out[0], out[1:]


def functions(elf):
    """{name: bytes} of the FUNC symbols that have a kernel descriptor (`name.kd`) beside them (ELF64, little endian)."""
    with open(elf, "rb") as f:
        b = f.read()
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", b, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]  # name type flags addr off size link info align entsize
    syms = {}
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        for o in range(s[4], s[4] + s[5], 24):
            name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", b, o)
            end = b.index(b"\0", stroff + name)
            syms[b[stroff + name:end].decode()] = (info & 15, shndx, value, size)
    out = {}
    for name, (typ, shndx, value, size) in syms.items():
        if typ == 2 and name + ".kd" in syms:  # STT_FUNC with a descriptor: a kernel (__hip_cuid_* is an object, never one)
            sec = secs[shndx]
            off = sec[4] + value - sec[3]
            out[name] = b[off:off + size]
    return out


def metadata(elf):
    """{kernel name: {field: int}} from the AMDGPU metadata note as llvm-readelf prints it."""
    txt = subprocess.run([os.path.join(ROCM, "llvm", "bin", "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"^  - (?=\.)", txt, flags=re.M)[1:]:
        m = re.search(r"^\s+\.name:\s+(\S+)", block, flags=re.M)
        if m:
            out[m.group(1).strip("'\"")] = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", block, flags=re.M).group(1)) for k in FIELDS}
    return out


def digest(csrc, unit, hipcc, flags, keep):
    elf = os.path.join(keep, os.path.splitext(unit)[0] + ".elf")
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", elf, unit], check=True, cwd=csrc)
    fn, md = functions(elf), metadata(elf)
    assert set(fn) == set(md), (unit, sorted(set(fn) ^ set(md)))
    return [" ".join([unit, k, str(len(fn[k])), hashlib.sha256(fn[k]).hexdigest()[:16]] + [str(md[k][f]) for f in FIELDS]) for k in sorted(fn)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=os.path.join(HERE, "..", "spiking_fullsubnet_amd", "csrc"))
    ap.add_argument("--units", nargs="*", help="default: every .hip file of the directory")
    ap.add_argument("--keep", help="directory that keeps the device ELFs")
    ap.add_argument("-j", type=int, default=4)
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    units = a.units or sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))
    hipcc, flags = make_flags(csrc)
    with tempfile.TemporaryDirectory() as tmp:
        keep = os.path.abspath(a.keep) if a.keep else tmp
        os.makedirs(keep, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(a.j) as ex:
            for lines in ex.map(lambda u: digest(csrc, u, hipcc, flags, keep), units):
                print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
