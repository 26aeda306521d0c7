#!/usr/bin/env python3
"""Did a change alter a kernel?  Compare the gfx950 code of two source trees.

    tools/codeobj_diff.py OLD [NEW] [--variant alt] [--dump FILE]

OLD and NEW are directories with the .hip sources and their headers (a csrc/
of this project), or a FILE that an earlier --dump wrote for its OLD (without
NEW nothing is compared).  Every *.hip of a
directory is compiled device-only with build.py's flags (plus --variant's),
in one scratch directory of a fixed name for both trees, since the path of a
source enters what hipcc derives from it.  From each translation unit's
gfx950 ELF every FUNC symbol is mapped to its bytes in .text and to its
kernel descriptor (<symbol>.kd).  The trees agree when they have the same
symbols, each with the same code bytes and the same descriptor, whichever
translation unit holds it.  Symbols are reported by name only.

A descriptor's bytes 16..23 are the distance from the descriptor to the
kernel's entry, a property of the object's layout and not of the kernel;
they are left out of the comparison.  Code that differs is disassembled and
compared again with the literals of pc-relative addresses (the s_add_u32 /
s_addc_u32 pair directly after an s_getpc_b64, on its registers) replaced by
the symbol and offset they reach: the distance to read-only data or to
another function moves with the layout, its target must not.  No other
operand is touched.  Such symbols are listed apart, never silently accepted.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--"


def _build_py():
    spec = importlib.util.spec_from_file_location("rp_build", os.path.join(ROOT, "ringpop_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def elf_symbols(path):
    """{name: (section name, offset in file, size, type, address)} of an ELF64 LE object."""
    with open(path, "rb") as f:
        e = f.read()
    assert e[:6] == b"\x7fELF\x02\x01", path
    shoff, = struct.unpack_from("<Q", e, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", e, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", e, shoff + i * shentsize) for i in range(shnum)]

    def cstr(tab, off):
        base = secs[tab][4] + off
        return e[base:e.index(b"\0", base)].decode()

    out = {}
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        for off in range(s[4], s[4] + s[5], s[8]):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", e, off)
            if 0 < shndx < shnum and size:
                sec = secs[shndx]
                out[cstr(s[6], name)] = (cstr(shstrndx, sec[0]), sec[4] + value - sec[3], size, info & 15, value)
    return out, e


GETPC = re.compile(r"s_getpc_b64 s\[(\d+):(\d+)\]\s*// ([0-9A-Fa-f]+):")
ADD = re.compile(r"(s_add_u32 s(\d+), s(\d+), )(0x[0-9a-f]+|-?\d+)(.*)")
ADDC = re.compile(r"(s_addc_u32 s(\d+), s(\d+), )(0x[0-9a-f]+|-?\d+)(.*)")


def _disasm(elf, where):
    """{symbol: its disassembly without addresses}.  The only operands replaced
    are the two literals of a pc-relative address -- s_getpc_b64 s[a:b], then
    s_add_u32 sa, sa, lo and s_addc_u32 sb, sb, hi directly after it -- and
    they are replaced by what the sum addresses, where(address) -> "symbol+offset":
    a call that reaches another function in the other tree is a difference."""
    r = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-leading-addr", elf],
                       capture_output=True, text=True, check=True)
    out, cur, pc = {}, None, None  # pc: (lo register, hi register, address after the s_getpc, lines since)
    for line in r.stdout.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
        if m:
            cur, pc = out.setdefault(m.group(1), []), None
            continue
        if cur is None:
            continue
        g, lo, hi = GETPC.search(line), ADD.search(line), ADDC.search(line)
        if g:
            pc = [int(g.group(1)), int(g.group(2)), int(g.group(3), 16) + 4, None]
        elif pc and pc[3] is None and lo and int(lo.group(2)) == int(lo.group(3)) == pc[0]:
            pc[3] = int(lo.group(4), 0) & 0xFFFFFFFF
            line = lo.group(1) + "LO" + lo.group(5)
        elif pc and pc[3] is not None and hi and int(hi.group(2)) == int(hi.group(3)) == pc[1]:
            target = (pc[2] + pc[3] + ((int(hi.group(4), 0) & 0xFFFFFFFF) << 32)) & 0xFFFFFFFFFFFFFFFF
            line = hi.group(1) + "HI -> " + where(target) + hi.group(5)
            pc = None
        else:
            pc = None
        cur.append(re.sub(r"\s*//.*|<[^>]*>", "", line))
    return {k: "\n".join(v) for k, v in out.items()}


def digest(src, flags, arch, jobs):
    """{symbol: [sha of code, sha of descriptor or None, code bytes, loose sha]} over all *.hip in src."""
    work = os.path.join(tempfile.gettempdir(), "codeobj_diff_%d" % os.getuid())
    shutil.rmtree(work, ignore_errors=True)
    # the tree keeps its depth, so that "../../include" resolves
    csrc = os.path.join(work, "ringpop_amd", "csrc")
    shutil.copytree(src, csrc)
    inc = os.path.normpath(os.path.join(src, "..", "..", "include"))
    if os.path.isdir(inc):
        shutil.copytree(inc, os.path.join(work, "include"))
    units = sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".hip"))

    def compile_one(u):
        bundle, elf = os.path.join(work, u + ".bundle"), os.path.join(work, u + ".elf")
        hipcc = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--offload-device-only", "-c",
                 os.path.join(csrc, u + ".hip"), "-o", bundle]
        r = subprocess.run(hipcc, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(" ".join(hipcc) + "\n" + r.stderr)
        with open(bundle, "rb") as f:
            raw = f.read(4) == b"\x7fELF"
        if raw:
            os.replace(bundle, elf)
        else:
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                            "--targets=" + TARGET + arch, "--input=" + bundle, "--output=" + elf], check=True)
        return elf

    with ThreadPoolExecutor(jobs) as ex:
        elfs = list(ex.map(compile_one, units))
    out = {}
    for elf in elfs:
        syms, e = elf_symbols(elf)

        def where(addr, syms=syms):
            for name, (_, _, size, _, value) in syms.items():
                if value <= addr < value + size:
                    return "%s+%d" % (name, addr - value)
            return "no symbol"

        text = _disasm(elf, where)
        for name, (sec, off, size, typ, _) in syms.items():
            if typ != 2 or sec != ".text":  # STT_FUNC
                continue
            assert name not in out, "symbol %s is defined twice" % name
            if name not in text:
                raise RuntimeError("llvm-objdump printed no label for the FUNC symbol " + name)
            kd = syms.get(name + ".kd")
            kd = e[kd[1]:kd[1] + 16] + e[kd[1] + 24:kd[1] + kd[2]] if kd else None
            out[name] = [hashlib.sha256(e[off:off + size]).hexdigest(),
                         kd and hashlib.sha256(kd).hexdigest(), size,
                         hashlib.sha256(text[name].encode()).hexdigest()]
    shutil.rmtree(work, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--variant", default=None, help="a key of build.py's VARIANTS (default: the product's flags)")
    ap.add_argument("--dump", metavar="FILE", help="keep OLD's digest, to compare against later")
    ap.add_argument("-j", type=int, default=int(os.environ.get("MAX_JOBS", "8")))
    a = ap.parse_args()
    b = _build_py()
    flags = b.FLAGS + (b.VARIANTS[a.variant] if a.variant else [])
    sides = []
    for side in filter(None, (a.old, a.new)):
        if os.path.isdir(side):
            d = digest(os.path.abspath(side), flags, b.ARCH, a.j)
        else:
            with open(side) as f:
                d = json.load(f)
        sides.append(d)
    if a.dump:
        with open(a.dump, "w") as f:
            json.dump(sides[0], f, indent=0, sort_keys=True)
    old, new = sides[0], sides[-1]
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    both = sorted(set(old) & set(new))
    kd = [s for s in both if old[s][1] != new[s][1]]
    code = [s for s in both if old[s][0] != new[s][0]]
    layout = [s for s in code if old[s][2] == new[s][2] and old[s][3] == new[s][3]]
    changed = [s for s in code if s not in layout]
    for title, names in (("only in OLD", gone), ("only in NEW", added), ("descriptor differs", kd),
                         ("code differs", changed),
                         ("code differs in the literals of pc-relative addresses only (same targets)", layout)):
        for s in names:
            print("%s: %s" % (title, s))
    ok = not (gone or added or kd or changed)
    print("%s: %d symbols (%d kernels), %d code bytes; %d identical byte for byte, %d equal up to layout: %s"
          % (a.variant or "default", len(new), sum(1 for s in new.values() if s[1]),
             sum(s[2] for s in new.values()), len(both) - len(code), len(layout), "SAME" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
