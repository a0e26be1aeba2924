#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (a refactor must leave the ISA as it is).

usage: asm_compare.py OLD_DIR NEW_DIR
Both directories hold device assembly of the sweep units, one file per unit and build, with the same names on both
sides (f64.s, f32.s, f64_alt.s, f32_alt.s ...), made with build.py's CXXFLAGS:
    hipcc <CXXFLAGS> -Iinclude --cuda-device-only -S armon.jl_amd/csrc/fused_sweep_f64.hip -o DIR/f64.s   [-DARMON_ALT_KERNELS]
A kernel that has left the sweep units (k_fill_uniform) is looked up in every other .s file of NEW_DIR (placement.s).
Kernels are paired by demangled name: k_sweep_y2<P, T, B, S> with k_sweep_y<P, T, B, S, 2>, k_sweep_y<P, T, B, S> with
k_sweep_y<P, T, B, S, 1>. Compared: the instructions, without comments, directives, local label names and the symbol's
own name; and the resources the assembler reports after each kernel (VGPR, AGPR, SGPR, scratch, LDS, waves/SIMD).
Prints a summary; exit status 1 if any kernel differs or has no counterpart."""
import os
import re
import subprocess
import sys


def kernels(path):
    """{normalised demangled name: (normalised instruction list, resources)} of one assembly file"""
    s = open(path).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", s, re.M)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, name in zip(syms, names):
        start = s.index("\n" + sym + ":")
        end = s.index("\n.Lfunc_end", start)
        body = s[s.index("\n", start + 1):end]
        labels, ins = {}, []
        for line in body.splitlines():
            t = line.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            t = t.replace(sym, "@self")
            t = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), t)
            ins.append(" ".join(t.split()))
        name = re.sub(r"^void |\(anonymous namespace\)::", "", name)
        name = re.sub(r"k_fill_uniform<\w+>", "k_fill_uniform", name)
        m = re.match(r"k_sweep_y(2?)<(.*)>(\(.*)$", name)
        if m and (m.group(1) or re.sub(r"<[^<>]*>", "", m.group(2)).count(",") == 3):
            name = "k_sweep_y<%s, %s>%s" % (m.group(2), "2" if m.group(1) else "1", m.group(3))
        res = tuple(int(re.compile(r"^; %s: (\d+)" % k, re.M).search(s, end).group(1))
                    for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy"))
        out[name] = (ins, res)
    return out


old_dir, new_dir = sys.argv[1:3]
units = sorted(f for f in os.listdir(old_dir) if f.endswith(".s"))
moved = {}
for f in sorted(os.listdir(new_dir)):
    if f.endswith(".s") and f not in units:
        moved.update(kernels(os.path.join(new_dir, f)))
total = same = 0
bad = []
for u in units:
    old, new = kernels(os.path.join(old_dir, u)), kernels(os.path.join(new_dir, u))
    n_same = 0
    for name, ins in old.items():
        other = new.pop(name, None) or moved.get(name)
        if other is None:
            bad.append(f"{u}: {name}: no counterpart")
        elif other != ins:
            bad.append(f"{u}: {name}: differs ({len(ins[0])} -> {len(other[0])} instructions, same opcode counts: "
                       f"{sorted(i.split()[0] for i in ins[0]) == sorted(i.split()[0] for i in other[0])}, "
                       f"VGPR/AGPR/SGPR/scratch/LDS/waves {ins[1]} -> {other[1]})")
        else:
            n_same += 1
    bad += [f"{u}: {name}: new kernel" for name in new]
    print(f"{u}: {len(old)} kernels, {n_same} identical")
    total += len(old)
    same += n_same
print(f"total: {total} kernels, {same} identical, {len(bad)} to look at")
for b in bad:
    print("  " + b)
sys.exit(1 if bad else 0)
