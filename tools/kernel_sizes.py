#!/usr/bin/env python3
"""Table of the device code in a built libglim_amd.so (no GPU needed): every gfx950 code object of the library's fat binary, and under it the
kernels it holds with their code size in bytes.  Two builds hold the same device code when their tables are equal.
  python tools/kernel_sizes.py glim_amd/libglim_amd.so > profiles/r09/kernel_sizes_this.txt
One line per code object (`object <sha256> <kernels>`, in the order of the sorted kernel lists, so the table does not depend on the link
order) followed by one line per kernel (`<bytes of code> <mangled name>`, sorted by name).  The hash is taken over the disassembly of .text and
the contents of .rodata (the kernel descriptors) and .data, not over the file: a code object also holds a symbol `__hip_cuid_<hash>`, and that
hash is the compiler's digest of the unit's path and command line, so it differs between two builds of the same code."""
import hashlib
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    with tempfile.NamedTemporaryFile(suffix=".fatbin") as f:
        subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + f.name, lib, "/dev/null"])
        fat = open(f.name, "rb").read()
    at = fat.find(MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", fat, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(count):
            offset, size, triple_len = struct.unpack_from("<QQQ", fat, pos)
            triple = fat[pos + 24:pos + 24 + triple_len].decode()
            pos += 24 + triple_len
            if "gfx950" in triple and size > 0:
                yield fat[at + offset:at + offset + size]
        at = fat.find(MAGIC, at + 1)


def kernels(obj):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj)
        f.flush()
        return kernels_of_file(f.name)


def kernels_of_file(path):
    rows = [l.split() for l in subprocess.check_output([LLVM + "llvm-readelf", "-sW", path], text=True).splitlines()]
    rows = [r for r in rows if len(r) == 8 and r[0].endswith(":")]
    descriptors = {r[7][:-3] for r in rows if r[3] == "OBJECT" and r[7].endswith(".kd")}
    code = subprocess.check_output([LLVM + "llvm-objdump", "-d", "-j", ".text", path]) + subprocess.check_output([LLVM + "llvm-objdump", "-s", "-j", ".rodata", "-j", ".data", path])
    code = b"\n".join(l for l in code.splitlines() if b"file format" not in l)  # (the first line names the file)
    return sorted({(r[7], int(r[2])) for r in rows if r[3] == "FUNC" and r[7] in descriptors}), hashlib.sha256(code).hexdigest()


def main():
    for ks, digest in sorted(kernels(o) for o in code_objects(sys.argv[1])):
        print(f"object {digest} {len(ks)}")
        for name, code in ks:
            print(f"{code} {name}")


if __name__ == "__main__":
    main()
