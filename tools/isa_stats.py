#!/usr/bin/env python3
"""Static figures per kernel from gfx950 assembly (hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o x.s):
instructions, VGPRs, SGPRs, private segment bytes and the count of every mnemonic prefix asked for.

    isa_stats.py x.s [y.s ...] [--kernels REGEX] [--count v_cndmask,v_cmp_eq,ds_bpermute,v_add_f64,scratch_,v_div_]

Needs no GPU: it is how DESIGN.md §4's "from the code" figures of k_res_vq / k_couple_fast were taken."""
import re
import sys

args = sys.argv[1:]
paths, kre, count = [], ".", "v_cndmask,v_cmp_eq,ds_bpermute,v_add_f64,scratch_,v_div_"
while args:
    a = args.pop(0)
    if a == "--kernels":
        kre = args.pop(0)
    elif a == "--count":
        count = args.pop(0)
    else:
        paths.append(a)
count = [c for c in count.split(",") if c]
for path in paths:
    txt = open(path).read()
    print(path)
    print(f"  {'kernel':58s} {'insts':>6s} {'vgpr':>5s} {'sgpr':>5s} {'priv':>5s} " + " ".join(f"{c:>11s}" for c in count))
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if not re.search(kre, name):
            continue
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, re.S)
        if not desc:
            continue            # a device function, not a kernel

        def field(f):
            return re.search(r"\.amdhsa_" + f + r" (\d+)", desc.group(1)).group(1)
        insts = [l.split()[0] for l in body.split("\n") if re.match(r"^\s+[a-z]+_[a-z0-9_]+", l)]
        short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:58]
        print(f"  {short:58s} {len(insts):6d} {field('next_free_vgpr'):>5s} {field('next_free_sgpr'):>5s} "
              f"{field('private_segment_fixed_size'):>5s} " + " ".join(f"{sum(i.startswith(c) for i in insts):11d}" for c in count))
