"""Compare the kernels of two sets of gfx950 code objects byte for byte (no GPU needed).

  python tools/kernel_diff.py --a <old ELF> [...] --b <new ELF> [...] [--rename OLD=NEW ...]

Each ELF is a device-only, unbundled code object: a source compiled with the flags build_ext.py gives it plus
`--cuda-device-only --no-gpu-bundle-output -c`.  A kernel is a function symbol <name> with a descriptor
symbol <name>.kd; per kernel name the tool compares the function's bytes in .text and the 64-byte descriptor
(registers, LDS, scratch, ...).  The descriptor's bytes 16..23 are the distance from the descriptor to the
code, a property of the file's layout and not of the kernel: they are checked to point at the function and
left out of the comparison.  `--rename OLD=NEW` compares the old side's kernels whose names begin with OLD with the
new side's whose names begin with NEW (a kernel that became a template instantiation keeps its code and its
descriptor and changes its name).  Prints the kernels that are identical, that differ and that only one side has;
the exit status is 1 when a kernel differs (or an ELF cannot be read), else 0.
"""
import argparse
import os
import shutil
import struct
import subprocess
import sys


def _llvm(tool):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", tool)
    return p if os.path.exists(p) else shutil.which(tool) or tool


def _run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def _sections(path):
    """index -> (address, file offset, size)"""
    secs = {}
    for line in _run(_llvm("llvm-readelf"), "-S", "-W", path).splitlines():
        line = line.strip()
        if not line.startswith("["):
            continue
        idx, rest = line[1:].split("]", 1)
        f = rest.split()
        if not idx.strip().isdigit() or len(f) < 5 or f[1] == "NULL":
            continue
        secs[int(idx)] = (int(f[2], 16), int(f[3], 16), int(f[4], 16))  # Name Type Address Off Size
    return secs


def kernels(path):
    """demangled kernel name -> (code bytes, descriptor bytes without the entry offset)"""
    secs = _sections(path)
    blob = open(path, "rb").read()
    syms = {}
    for line in _run(_llvm("llvm-readelf"), "-s", "-W", "--demangle", path).splitlines():
        f = line.split(None, 7)  # Num: Value Size Type Bind Vis Ndx Name (a demangled name has spaces)
        if len(f) == 8 and f[0].endswith(":") and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            syms[f[7].strip()] = (int(f[1], 16), int(f[2]), int(f[6]))

    def data(value, size, ndx):
        addr, off, _ = secs[ndx]
        return blob[off + value - addr: off + value - addr + size]

    out = {}
    for name, (value, size, ndx) in syms.items():
        kd = syms.get(name + " (.kd)") or syms.get(name + ".kd")  # demangled / plain C name
        if kd is None:
            continue
        desc = data(*kd)
        if len(desc) != 64:
            raise RuntimeError(f"{path}: descriptor of {name} has {len(desc)} bytes")
        if kd[0] + struct.unpack_from("<q", desc, 16)[0] != value:
            raise RuntimeError(f"{path}: descriptor of {name} does not point at its code")
        out[name] = (data(value, size, ndx), desc[:16] + desc[24:])
    return out


def gather(paths):
    all_k = {}
    for p in paths:
        for name, k in kernels(p).items():
            if name in all_k:
                raise RuntimeError(f"kernel {name} is in more than one ELF of a side ({p})")
            all_k[name] = k
    return all_k


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--a", nargs="+", required=True, help="code objects of the old side")
    ap.add_argument("--b", nargs="+", required=True, help="code objects of the new side")
    ap.add_argument("--rename", nargs="*", default=[], metavar="OLD=NEW",
                    help="a kernel whose name begins with OLD on the old side is compared with the one whose name "
                         "has NEW there on the new side (a kernel that became a template instantiation)")
    args = ap.parse_args()
    a, b = gather(args.a), gather(args.b)
    for pair in args.rename:
        old, new = pair.split("=", 1)
        b = {(old + n[len(new):] if n.startswith(new) else n): k for n, k in b.items()}
    names = sorted(set(a) | set(b))
    same = [n for n in names if n in a and n in b and a[n] == b[n]]
    differ = [n for n in names if n in a and n in b and a[n] != b[n]]
    for title, group in (("identical", same), ("differing", differ), ("only in --a", [n for n in names if n not in b]),
                         ("only in --b", [n for n in names if n not in a])):
        print(f"{title}: {len(group)}")
        for n in group:
            what = ""
            if title == "differing":
                what = "  [" + ", ".join(w for w, i in (("code", 0), ("descriptor", 1)) if a[n][i] != b[n][i]) + "]"
            print(f"  {n}{what}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
