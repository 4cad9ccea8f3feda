#!/usr/bin/env python3
"""Count, per kernel of an AMDGPU assembly file, the MFMAs that reuse an accumulator before it is ready.  No GPU needed.

Input: the -S output of a .hip file built with the Makefile's flags, e.g.
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S gemm2.hip -o gemm2.s
    python tools/mfma_reuse.py gemm2.s [--match gemm4_kernel]

v_mfma_f32_16x16x4_f32 issues every 32 cycles and delivers its result after 40, so an MFMA whose C operand was written
by the MFMA issued right before it (fewer than two MFMA issues earlier) stalls its wave.  Instructions are taken in
textual order, which is the execution order inside a basic block; a pair split by a label or a branch is still
counted (K loops fall through their blocks), a pair across a loop's back edge is not seen.

Per kernel, one line:
    mfma    MFMA instructions, and how many of them keep C / D in accumulator registers (a[..])
    reuse   MFMAs whose C overlaps the D of the previous MFMA
    kstep   inside the inner loop with the most MFMAs, between its first and last MFMA: MFMAs, LDS reads, other
            vector-ALU instructions (v_*; each one is matrix-pipe time in a one-wave-per-SIMD kernel), s_nop
    regs    NumVgprs / NumAgprs / ScratchSize as the compiler reports them
"""
import argparse
import collections
import re
import sys

Kernel = collections.namedtuple("Kernel", "name mfma mfma_acc reuse loop_mfma loop_ds loop_valu loop_nop vgprs agprs scratch")

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_FUNC_END = re.compile(r"^\s*\.Lfunc_end\d+:|^\s*\.end_amdhsa_kernel")
_MFMA = re.compile(r"^\s*(v_mfma_\w+)\s+([av])(?:\[(\d+):(\d+)\]|(\d+)),\s*[^,]+,\s*[^,]+,\s*(?:([av])(?:\[(\d+):(\d+)\]|(\d+))|[-\d.x]+)")
_INSN = re.compile(r"^\s+([a-z]\w+)")
_STAT = re.compile(r"^;\s*(NumVgprs|NumAgprs|ScratchSize):\s*(\d+)")
_LOOP_HEADER = re.compile(r"^(\.LBB\d+_\d+):.*Loop Header")
_BLOCK = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")


def _range(kind, lo, hi, single):
    if kind is None:
        return None
    lo, hi = (int(single), int(single)) if single is not None else (int(lo), int(hi))
    return kind, lo, hi


def _overlap(a, b):
    return a is not None and b is not None and a[0] == b[0] and a[1] <= b[2] and b[1] <= a[2]


def _kstep(lines):
    """(MFMAs, LDS reads, other v_* instructions, s_nop) between the first and last MFMA of the inner loop with most MFMAs."""
    best = (0, 0, 0, 0)
    for i, line in enumerate(lines):
        m = _LOOP_HEADER.match(line)
        if not m:
            continue
        # the header block and the blocks laid out behind it that the compiler marks as part of this loop (a rotated loop's
        # latch sits in front of the header and is not needed: the MFMAs of a K step start in the header block)
        mine = f"Header={m.group(1)[2:]} "
        end = i + 1
        while end < len(lines) and not (_BLOCK.match(lines[end]) and mine not in lines[end] + " "):
            end += 1
        body = lines[i:end]
        at = [j for j, l in enumerate(body) if _MFMA.match(l)]
        if len(at) <= best[0]:
            continue
        ops = [o.group(1) for l in body[at[0]:at[-1] + 1] if (o := _INSN.match(l))]
        best = (len(at), sum(o.startswith("ds_read") for o in ops),
                sum(o.startswith("v_") and not o.startswith("v_mfma") for o in ops), sum(o == "s_nop" for o in ops))
    return best


def parse(text):
    """[Kernel] for every function of the assembly that contains an MFMA, in file order."""
    out, name, body = [], None, []
    stats = {}

    def close():
        nonlocal name, body, stats
        if name is not None and any(_MFMA.match(l) for l in body):
            mfma = acc = reuse = 0
            prev_d = None
            for l in body:
                m = _MFMA.match(l)
                if not m:
                    continue
                d = _range(m.group(2), m.group(3), m.group(4), m.group(5))
                c = _range(m.group(6), m.group(7), m.group(8), m.group(9))
                mfma += 1
                acc += d[0] == "a"
                reuse += _overlap(c, prev_d)
                prev_d = d
            out.append(Kernel(name, mfma, acc, reuse, *_kstep(body), stats.get("NumVgprs"), stats.get("NumAgprs"),
                              stats.get("ScratchSize")))
        name, body, stats = None, [], {}

    for line in text.splitlines():
        s = _STAT.match(line)
        if s and name is not None:
            stats.setdefault(s.group(1), int(s.group(2)))
            if len(stats) == 3:
                close()
            continue
        m = _LABEL.match(line)
        if m and not m.group(1).startswith("."):
            close()
            name = m.group(1)
            continue
        if name is not None:
            body.append(line)
    close()
    return out


def short(name):
    """_ZN3gdx12gemm4_kernelILi5ELi1ELi64ELi3ELb1EE... -> gemm4_kernel<5,1,64,3,1>"""
    m = re.match(r"_ZN\d+\w+?\d+([a-z]\w*?)I((?:L[ib]\d+E)+)E", name)
    if not m:
        return name
    args = ",".join(re.findall(r"L[ib](\d+)E", m.group(2)))
    return f"{m.group(1)}<{args}>"


def report(kernels):
    rows = [f"{'kernel':34s} {'mfma':>5s} {'in a[]':>6s} {'reuse':>5s}   kstep: {'mfma':>4s} {'ds_rd':>5s} {'valu':>4s} {'nop':>3s}   "
            f"{'vgpr':>4s} {'agpr':>4s} {'scratch':>7s}"]
    for k in kernels:
        rows.append(f"{short(k.name):34s} {k.mfma:5d} {k.mfma_acc:6d} {k.reuse:5d}          {k.loop_mfma:4d} {k.loop_ds:5d} "
                    f"{k.loop_valu:4d} {k.loop_nop:3d}   {k.vgprs!s:>4s} {k.agprs!s:>4s} {k.scratch!s:>7s}")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--match", default="", help="only kernels whose mangled name contains this")
    args = ap.parse_args()
    with open(args.asm) as f:
        kernels = [k for k in parse(f.read()) if args.match in k.name]
    print(report(kernels))
    return 0


if __name__ == "__main__":
    sys.exit(main())
