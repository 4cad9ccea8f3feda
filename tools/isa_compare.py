#!/usr/bin/env python3
"""Compare the gfx950 device code of two trees, kernel by kernel (no GPU needed).

    python tools/isa_compare.py OLD_TREE NEW_TREE [-j N]

Every kernel file of csrc/ is compiled to device-only assembly with the Makefile's flags (the half files also with -DGDX_BF16,
sampler.hip with -ffp-contract=off).  Per kernel the instruction stream (comments dropped) and the .vgpr_count / .sgpr_count /
LDS / scratch / kernarg sizes of the metadata are compared; kernels are matched by symbol, with the two leading template
arguments that older trees gave gemm_kernel removed.  Prints one line per difference and a summary line; exit status 1 if any.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-variable -Wno-unused-but-set-variable".split()
HALF = ("gemmh.hip", "attentionh.hip", "misc.hip")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def variants(csrc):
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip"):
            continue
        if "__global__" not in open(os.path.join(csrc, f)).read():
            continue
        yield f, f, ["-ffp-contract=off"] if f == "sampler.hip" else []
        if f in HALF:
            yield f + " -DGDX_BF16", f, ["-DGDX_BF16"]


def emit(csrc, src, extra, out):
    subprocess.run([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def norm(text):
    return re.sub(r"gemm_kernelILi\dELi\dELi(\d)ELi(\d)EEE", r"gemm_kernelILi\1ELi\2EEE", text)


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
        lines = [re.sub(r"\s*;.*$", "", ln).strip() for ln in body.splitlines()]
        out[n] = ([ln for ln in lines if ln], meta[n])
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-j")]
    jobs = next((int(a[2:]) for a in sys.argv[1:] if a.startswith("-j") and a[2:]), 8)
    old, new = (os.path.join(a, "gesturediffusion_amd", "csrc") for a in args)
    ndiff = nk = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        futs = []
        for tag, src, extra in variants(new):
            if not os.path.exists(os.path.join(old, src)):
                print("only in the new tree (has kernels):", src)
                ndiff += 1
                continue
            base = os.path.join(tmp, tag.replace(" ", "_"))
            futs.append((tag, ex.submit(emit, old, src, extra, base + ".old.s"), ex.submit(emit, new, src, extra, base + ".new.s")))
        for tag, fo, fn in futs:
            ko, kn = kernels(fo.result()), kernels(fn.result())
            for n in sorted(set(ko) | set(kn)):
                nk += 1
                if n not in ko or n not in kn:
                    print("%s: %s only in the %s tree" % (tag, n, "old" if n in ko else "new"))
                    ndiff += 1
                    continue
                if ko[n][0] != kn[n][0]:
                    print("%s: %s: instruction streams differ (%d vs %d lines)" % (tag, n, len(ko[n][0]), len(kn[n][0])))
                    ndiff += 1
                for k in META:
                    if ko[n][1][k] != kn[n][1][k]:
                        print("%s: %s: %s %s -> %s" % (tag, n, k, ko[n][1][k], kn[n][1][k]))
                        ndiff += 1
    print("# %d kernels compared, %d differences" % (nk, ndiff))
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
