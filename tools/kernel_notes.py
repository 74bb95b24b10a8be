#!/usr/bin/env python
"""kernel_notes.py -- register / scratch / LDS figures of the kernels in a compiled object, read from the code object's
notes (no GPU needed):

    python tools/kernel_notes.py [pattern] [object ...]  default objects: aaltoasr_amd/lib/obj/gmm_score*.hip.o
    python tools/kernel_notes.py --digest [object ...]   default objects: the same (the files of the scoring unit)

The first form prints one line per kernel of the objects whose demangled name contains `pattern`.

--digest prints one line per kernel of the given objects (hipcc objects or a linked libaasr.so), sorted by name: the
demangled name, SHA-256 over the kernel's machine code bytes, SHA-256 over its 64-byte kernel descriptor, and the notes
figures.  Two builds produce the same table exactly when they hold the same kernels with the same device code, wherever
the kernels stand in their source files: bytes do not depend on a function's position, assembly text (local label
numbers) does.  The one position-dependent field, the descriptor's kernel_code_entry_byte_offset (bytes 16-23: the
distance from descriptor to code), is zeroed before hashing.  A kernel that addresses data outside itself PC-relatively
(a constant table in .rodata: the feature kernels' FFT and mel kernels; none of the scoring kernels) carries a
position-dependent literal as well: such a kernel is hashed over its disassembly with that literal taken out, and its line
says "asm" where the others say "code"."""
import glob
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
OBJDIR = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj")


def code_objects(obj, workdir):
    """The gfx950 code objects embedded in a hipcc object file (one) or a linked library (one per device source)."""
    tmp = os.path.join(workdir, "x.o")
    with open(obj, "rb") as f, open(tmp, "wb") as g:
        g.write(f.read())
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", tmp], check=True, capture_output=True)
    cos = sorted(os.path.join(workdir, n) for n in os.listdir(workdir) if "amdgcn" in n)
    if not cos:
        raise RuntimeError("no device code object in " + obj)
    return cos


def code_object(obj, workdir):
    return code_objects(obj, workdir)[0]


def _notes_of(co):
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                         text=True).stdout
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        def num(key):
            m = re.search(r"\.%s:\s+(\d+)" % key, blk)
            return int(m.group(1)) if m else 0
        agpr = int(re.match(r"\s*(\d+)", blk).group(1))
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m:
            continue
        out[m.group(1)] = dict(vgpr=num("vgpr_count"), agpr=agpr, sgpr=num("sgpr_count"),
                               spill_vgpr=num("vgpr_spill_count"), spill_sgpr=num("sgpr_spill_count"),
                               scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size"))
    return out


def _demangle(names):
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"^void ", "", d).split("(")[0] for d in dem[:len(names)]]


def kernel_notes(obj):
    """{demangled kernel name: {vgpr, agpr, sgpr, spill_vgpr, spill_sgpr, scratch, lds}} of every kernel in `obj`."""
    with tempfile.TemporaryDirectory() as d:
        out = _notes_of(code_object(obj, d))
    names = list(out)
    return {d: out[n] for n, d in zip(names, _demangle(names))}


def _symbol_bytes(co):
    """{symbol: its bytes in the file} for the sized FUNC and OBJECT symbols of a 64-bit little-endian ELF."""
    data = open(co, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01", co
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _name, typ, _flags, _addr, off, size, link, _info, _align, entsize in secs:
        if typ != 2:   # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for o in range(off, off + size, entsize):
            st_name, st_info, _other, shndx, value, st_size = struct.unpack_from("<IBBHQQ", data, o)
            if (st_info & 0xf) not in (1, 2) or st_size == 0 or shndx == 0 or shndx >= shnum:
                continue
            sec = secs[shndx]
            if sec[1] == 8:   # SHT_NOBITS
                continue
            start = sec[4] + (value - sec[3])
            end = data.index(b"\0", stroff + st_name)
            out[data[stroff + st_name:end].decode()] = data[start:start + st_size]
    return out


def _pc_relative_kernels(co, symbols):
    """{kernel: SHA-256 over its normalised disassembly} for the kernels of `co` that read the program counter: the
    instruction text without addresses and encodings, and without the literal of the s_add_u32 / s_addc_u32 pair behind
    every s_getpc_b64 (the distance to a constant table outside the kernel)."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    body, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1) if m.group(1) in symbols else None
        elif cur and line.strip():
            body.setdefault(cur, []).append(line.split("//")[0].strip())
    out = {}
    for name, ins in body.items():
        if not any(i.startswith("s_getpc_b64") for i in ins):
            continue
        for k, i in enumerate(ins):
            if i.startswith("s_getpc_b64"):
                for j in (k + 1, k + 2):
                    if j < len(ins) and re.match(r"s_addc?_u32 ", ins[j]):
                        ins[j] = ins[j].rsplit(",", 1)[0] + ", <pc-relative>"
        out[name] = hashlib.sha256("\n".join(ins).encode()).hexdigest()
    return out


def kernel_digests(objs):
    """[(demangled name, "code" | "asm", sha256, descriptor sha256, notes)] of every kernel in `objs`, sorted by name; a
    kernel that occurs twice (instantiated in two files) is listed twice.  "asm": a kernel with PC-relative references,
    hashed over its normalised disassembly instead of its bytes."""
    rows = []
    for obj in objs:
        with tempfile.TemporaryDirectory() as d:
            for co in code_objects(obj, d):
                notes = _notes_of(co)
                syms = _symbol_bytes(co)
                pcrel = _pc_relative_kernels(co, set(notes))
                names = sorted(notes)
                for n, dem in zip(names, _demangle(names)):
                    kd = bytearray(syms[n + ".kd"])
                    assert len(kd) == 64, (n, len(kd))
                    kd[16:24] = bytes(8)   # kernel_code_entry_byte_offset: descriptor -> code distance
                    how, h = ("asm", pcrel[n]) if n in pcrel else ("code", hashlib.sha256(syms[n]).hexdigest())
                    rows.append((dem, how, h, hashlib.sha256(bytes(kd)).hexdigest(), notes[n]))
    return sorted(rows, key=lambda r: r[:4])


def digest_lines(objs):
    return ["%s %s %s kd %s vgpr %d agpr %d sgpr %d spill v %d s %d scratch %d lds %d" % (
        name, how, h, kd, k["vgpr"], k["agpr"], k["sgpr"], k["spill_vgpr"], k["spill_sgpr"], k["scratch"], k["lds"])
        for name, how, h, kd, k in kernel_digests(objs)]


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--digest":
        objs = sys.argv[2:] or sorted(glob.glob(os.path.join(OBJDIR, "gmm_score*.hip.o")))
        lines = digest_lines(objs)
        print("\n".join(lines))
        sys.stderr.write("%d kernels, table sha256 %s\n" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))
        sys.exit(0)
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    objs = sys.argv[2:] or sorted(glob.glob(os.path.join(OBJDIR, "gmm_score*.hip.o")))
    for name, k in sorted(((n, k) for obj in objs for n, k in kernel_notes(obj).items()), key=lambda r: r[0]):
        if pat in name:
            print("%-70s vgpr %3d agpr %3d sgpr %3d spill v %3d s %3d scratch %4d B" % (
                name[-70:], k["vgpr"], k["agpr"], k["sgpr"], k["spill_vgpr"], k["spill_sgpr"], k["scratch"]))
