#!/usr/bin/env python3
"""tools/kernel_regs.py -- registers / LDS / scratch of the gfx950 kernels inside an object file or the built library.

    python tools/kernel_regs.py [file.o | liblink_amd.so] [substring ...]
    python tools/kernel_regs.py --digest [file.o | liblink_amd.so] [--against LISTING]

--digest prints one line per kernel: a hash over the function's bytes, its 64-byte kernel descriptor and its entry in the
metadata note (registers, LDS, scratch, kernarg layout) -- what a refactor that must not change device code is checked with
(compare two listings with --against: names on one side only, differing hashes, names in two code objects).  Two things move
with the layout of a code object and are normalised: bytes 16-23 of the descriptor (its distance to the code), and, in a
kernel that calls an out-of-line function, the PC-relative literal of the s_add_u32 / s_addc_u32 pair after s_getpc_b64
(such kernels are hashed on their disassembly with that literal masked).  Local out-of-line functions (sincos_slow) are
listed too, one line per copy.

Reads the code object's metadata notes (llvm-readelf): vgpr, agpr, sgpr, static LDS, scratch bytes, workgroup size.
What the persistent batch kernels' co-residency argument is checked against, and what
tests/test_cpu_abi.py::test_batch_kernels_resource_shape asserts.
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.split("\n")[:len(names)]
    except Exception:
        return names


def code_objects(path, td):
    """Unbundle the gfx950 code object of every translation unit in `path` into `td`; their file names."""
    fat = os.path.join(td, "fat.bin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", path],
                          stderr=subprocess.DEVNULL)
    blob = open(fat, "rb").read()
    # a shared library concatenates the fat binaries of its objects: split at the bundler magic
    # (plain bundles start with the bundler's magic, compressed ones -- hipcc --offload-compress -- with "CCOB"; the bundler inflates them itself)
    starts = sorted(m.start() for m in re.finditer(rb"__CLANG_OFFLOAD_BUNDLE__|CCOB", blob))
    cos = []
    for i, s in enumerate(starts):
        part = os.path.join(td, f"part{i}.bin")
        with open(part, "wb") as f:
            end = starts[i + 1] if i + 1 < len(starts) else len(blob)
            if blob[s:s + 4] == b"CCOB":              # its header holds the bundle's own size: the linker pads behind it
                ver, = struct.unpack_from("<H", blob, s + 4)
                end = s + struct.unpack_from("<Q" if ver >= 3 else "<I", blob, s + 8)[0]
            f.write(blob[s:end])
        co = os.path.join(td, f"part{i}.co")
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
        if r.returncode == 0 and os.path.exists(co):
            cos.append(co)
    return cos


def kernel_table(path):
    """[(demangled name, vgpr, agpr, sgpr, lds_static, scratch, max_wg)] of every gfx950 kernel in `path`."""
    with tempfile.TemporaryDirectory() as td:
        rows = []
        for co in code_objects(path, td):
            txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for e in re.split(r"\n\s+- \.agpr_count", txt)[1:]:
                e = ".agpr_count" + e
                g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, e) or [None, "?"])[1]
                rows.append([g("name"), g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("group_segment_fixed_size"),
                             g("private_segment_fixed_size"), g("max_flat_workgroup_size")])
        names = _demangle([r[0] for r in rows])
        return [(n, *r[1:]) for n, r in zip(names, rows)]


def _elf_symbols(blob):
    """{name: [(bytes, type)]} of the defined symbols of an ELF64 little-endian image."""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for sec in secs:
        if sec[1] != 2:                                     # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for o in range(sec[4], sec[4] + sec[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", blob, o)
            if not 0 < shndx < shnum or not size:
                continue
            at = secs[shndx][4] + value - secs[shndx][3]
            end = blob.index(b"\0", stroff + name)
            out.setdefault(blob[stroff + name:end].decode(), []).append((blob[at:at + size], info & 15))
    return out


def _masked_disassembly(co, name):
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr",
                          f"--disassemble-symbols={name}", co], capture_output=True, text=True, check=True).stdout
    lines, pc = [re.sub(r"\s*//.*$", "", ln) for ln in txt.split("\n")], 0      # the comment is the address and the raw words
    for i, ln in enumerate(lines):
        if "s_getpc_b64" in ln:
            pc = 2
        elif pc and re.search(r"s_addc?_u32", ln):
            lines[i], pc = re.sub(r"(0x[0-9a-f]+|\b\d+)(\s*(//.*)?)$", "LIT", ln), pc - 1
    # "..." is objdump's mark for the zero padding up to the next symbol, which is not part of the function
    return "\n".join(l for l in lines if "file format" not in l and l.strip() != "...")


def digest(path):
    """[(hash, name, unit index)] of every kernel and every local out-of-line function of `path`."""
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for unit, co in enumerate(code_objects(path, td)):
            blob = open(co, "rb").read()
            syms = _elf_symbols(blob)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            meta = {}
            for e in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                e = e.split("\namdhsa.", 1)[0]
                meta[re.search(r"\.symbol:\s+'?([^'\s]+?)\.kd'?\s", e)[1]] = e
            for name, defs in sorted(syms.items()):
                if name + ".kd" in syms:
                    code, kd = defs[0][0], bytearray(syms[name + ".kd"][0][0])
                    kd[16:24] = bytes(8)
                    h = hashlib.sha256(bytes(kd) + meta[name].encode())
                    # s_getpc_b64 (SOP1 op 0x1c): a PC-relative address follows
                    words = struct.unpack_from("<%dI" % (len(code) // 4), code)
                    if any((w & 0xFF80FFFF) == 0xBE801C00 for w in words):
                        h.update(_masked_disassembly(co, name).encode())
                    else:
                        h.update(code)
                    rows.append((h.hexdigest()[:24], name, unit))
                elif defs[0][1] == 2 and not name.endswith(".kd") and "sincos_slow" in name:   # STT_FUNC, local helper
                    rows.append((hashlib.sha256(defs[0][0]).hexdigest()[:24], name + "#copy", unit))
    return rows


def main_digest(args):
    path = os.path.join(ROOT, "link_amd", "lib", "liblink_amd.so")
    against = None
    if "--against" in args:
        i = args.index("--against")
        against, args = args[i + 1], args[:i] + args[i + 2:]
    if args:
        path = args[0]
    rows = digest(path)
    kernels = {}
    dup = 0
    for h, name, unit in rows:
        print(h, unit, name)
        if not name.endswith("#copy"):
            dup += name in kernels
            kernels[name] = h
    helpers = sorted({(n, h) for h, n, _ in rows if n.endswith("#copy")})
    msg = f"kernels: {len(kernels)}, in two code objects: {dup}, out-of-line helpers: {len(helpers)} distinct"
    if against:
        old, old_helpers = {}, set()
        for ln in open(against):
            f = ln.split()
            if len(f) == 3 and f[2].endswith("#copy"):
                old_helpers.add((f[2], f[0]))
            elif len(f) == 3 and not ln.startswith("#"):
                old[f[2]] = f[0]
        only = set(old) ^ set(kernels)
        differing = [n for n in kernels if n in old and old[n] != kernels[n]]
        for n in sorted(only) + differing:
            print("#", "one side only" if n in only else "differs", n)
        msg += (f"; against {os.path.basename(against)}: {len(old)} kernels, on one side only: {len(only)}, differing: {len(differing)}, "
                f"helpers equal: {set(helpers) == old_helpers}")
    print("#", msg)
    return 1 if dup or (against and (only or differing or set(helpers) != old_helpers)) else 0


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        args.remove("--digest")
        sys.exit(main_digest(args))
    path = os.path.join(ROOT, "link_amd", "lib", "liblink_amd.so")
    if args and os.path.exists(args[0]):
        path, args = args[0], args[1:]
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'lds':>7} {'scratch':>7} {'wg':>5}  kernel")
    for name, v, a, s, lds, scr, wg in kernel_table(path):
        if args and not any(k in name for k in args):
            continue
        print(f"{v:>5} {a:>5} {s:>5} {lds:>7} {scr:>7} {wg:>5}  {name[:150]}")


if __name__ == "__main__":
    main()
