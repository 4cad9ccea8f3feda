#!/usr/bin/env python3
"""Compare the gfx950 device code of two trees, kernel by kernel (no GPU needed).

    python tools/isa_compare.py OLD_TREE NEW_TREE [-j N]

Every kernel file of csrc/ is compiled to device-only assembly with the Makefile's flags (the files of each tree's own
HALF_SRCS line also with -DGDX_BF16, the files of its own EXACT_SRCS line with -ffp-contract=off; a tree from before that line
existed has the flag on sampler.hip, as it was built).  Per kernel the instruction stream (comments and the
per-file numbers of local labels dropped) and the .vgpr_count / .sgpr_count / LDS / scratch / kernarg sizes of the metadata are
compared.  Kernels are matched by symbol (and the variant's extra flags) across the whole tree, so one that moved to another file
compares equal and is reported as moved.  The half builds' namespaces gdx::h16:: and gdx::b16:: count as gdx:: (the -DGDX_BF16
flag keeps the two builds apart), so a kernel that left the half build, or a template that left the namespace because its
argument names the element type, is "moved" as well, not one removed and one added.  The two leading template arguments that
older trees gave gemm_kernel are removed, and so are the two trailing ones (ring depth 6, whole-line pipeline) of older trees'
gemmh_kernel.  Prints one line per difference or move and a summary line; exit status 1 if any difference.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-variable -Wno-unused-but-set-variable".split()
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def makefile_list(csrc, var, default):
    """the files of the line `var = ...` of a tree's Makefile; `default` for a tree whose Makefile has no such line"""
    m = re.search(r"^%s\s*=\s*(.*)$" % var, open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split() if m else default


def variants(csrc):
    half = makefile_list(csrc, "HALF_SRCS", [])                 # built a second time with -DGDX_BF16
    exact = makefile_list(csrc, "EXACT_SRCS", ["sampler.hip"])  # built with -ffp-contract=off; older trees: the one file
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip"):
            continue
        if "__global__" not in open(os.path.join(csrc, f)).read():
            continue
        yield f, f, ["-ffp-contract=off"] if f in exact else []
        if f in half:
            yield f + " -DGDX_BF16", f, ["-DGDX_BF16"]


def emit(csrc, src, extra, out):
    subprocess.run([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def drop_half_ns(m):
    """N3gdx3h16<rest> -> N3gdx<rest>: the name loses one component and with it substitution S0_, so S<k+1>_ becomes S<k>_"""
    def shift(s):
        k = int(s.group(1), 36)
        return "S_" if k == 0 else "S%s_" % "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"[k - 1]   # no kernel here has more than 36
    return "N3gdx" + re.sub(r"S([0-9A-Z])_", shift, m.group(1))


def norm(text):
    text = re.sub(r"N3gdx3[hb]16(\w+)", drop_half_ns, text)
    text = re.sub(r"gemm_kernelILi\dELi\dELi(\d)ELi(\d)EEE", r"gemm_kernelILi\1ELi\2EEE", text)
    return re.sub(r"gemmh_kernelILi(\d+)ELi(\d)ELi6ELb1EEE", r"gemmh_kernelILi\1ELi\2EEE", text)


def kernels(text):
    """symbol -> (instruction lines, metadata dict)"""
    text = norm(text)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    meta = {}
    for block in re.split(r"^\s*- \.agpr_count:", text, flags=re.M)[1:]:
        sym = re.search(r"^\s*\.name:\s+(\S+)\s*$", block, re.M)
        for m in re.finditer(r"^\s*\.symbol:\s+(\S+?)\.kd\s*$", block, re.M):
            sym = m
        meta[sym.group(1)] = {k: re.search(r"^\s*%s:\s+(\d+)" % re.escape(k), block, re.M).group(1) for k in META}
    out = {}
    for n in names:
        body = text[text.index("\n%s:" % n):]
        body = body[:body.index(".Lfunc_end")]
        lines = [re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", re.sub(r"\s*;.*$", "", ln)).strip() for ln in body.splitlines()]
        out[n] = ([ln for ln in lines if ln], meta[n])
    return out


def tree_kernels(csrc, ex, tmp, side):
    """(symbol, extra flags) -> (variant it was found in, instruction lines, metadata dict), over every kernel file of the tree"""
    futs = [(tag, extra, ex.submit(emit, csrc, src, extra, os.path.join(tmp, "%s.%s.s" % (tag.replace(" ", "_"), side))))
            for tag, src, extra in variants(csrc)]
    out = {}
    for tag, extra, fut in futs:
        for n, (lines, meta) in kernels(fut.result()).items():
            out[n, " ".join(extra)] = (tag, lines, meta)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-j")]
    jobs = next((int(a[2:]) for a in sys.argv[1:] if a.startswith("-j") and a[2:]), 8)
    old, new = (os.path.join(a, "gesturediffusion_amd", "csrc") for a in args)
    ndiff = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        ko, kn = tree_kernels(old, ex, tmp, "old"), tree_kernels(new, ex, tmp, "new")
    for key in sorted(set(ko) | set(kn)):
        n = key[0]
        if key not in ko or key not in kn:
            print("%s: %s only in the %s tree" % ((ko.get(key) or kn[key])[0], n, "old" if key in ko else "new"))
            ndiff += 1
            continue
        (to, lo, mo), (tag, ln, mn) = ko[key], kn[key]
        if to != tag:
            print("%s: %s: moved here from %s" % (tag, n, to))
        if lo != ln:
            print("%s: %s: instruction streams differ (%d vs %d lines)" % (tag, n, len(lo), len(ln)))
            ndiff += 1
        for k in META:
            if mo[k] != mn[k]:
                print("%s: %s: %s %s -> %s" % (tag, n, k, mo[k], mn[k]))
                ndiff += 1
    print("# %d kernels compared (%d in the old tree, %d in the new), %d differences" % (len(set(ko) | set(kn)), len(ko), len(kn), ndiff))
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
