"""One line per kernel of a built library's gfx950 code object, sorted by symbol:
    symbol <tab> instruction count <tab> sha1 of the kernel's instruction text
with addresses, raw encodings and comments removed, so a digest does not depend on where the kernel sits in .text (kernels are
laid out in order of first instantiation: a host-only change can move them).  Two builds whose tables are equal carry the same
machine code for every kernel - the claim "kernel machine code is unchanged" as a diff.  The code object is extracted as
tools/check_opsel.py does it.
Usage: python tools/codeobj_digest.py path/to/libfnoengine.so > table.txt"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def digest(lib):
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        os.symlink(os.path.abspath(lib), local)
        subprocess.check_call([OBJDUMP, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert co, "no gfx950 code object in " + lib
        dis = subprocess.check_output([OBJDUMP, "-d", "--no-leading-addr", "--no-show-raw-insn", os.path.join(tmp, co[0])], text=True)
    tab, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:", line)
        if m:
            cur = tab[m.group(1)] = [hashlib.sha1(), 0]
            continue
        line = line.split("//")[0].strip()
        if cur is not None and line:
            cur[0].update(line.encode() + b"\n")
            cur[1] += 1
    return tab


if __name__ == "__main__":
    for sym, (h, n) in sorted(digest(sys.argv[1]).items()):
        print(f"{sym}\t{n}\t{h.hexdigest()}")
