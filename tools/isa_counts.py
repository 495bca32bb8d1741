#!/usr/bin/env python3
"""Static instruction counts of the update kernels, from a device-only cross-compilation of sampler.hip to assembly (no GPU needed):
    hipcc <the product flags of bipymc_amd/csrc/Makefile> --cuda-device-only -S -o sampler.s bipymc_amd/csrc/sampler.hip
usage: isa_counts.py sampler.s [name filter ...]        (default filter: phase_fused_kernel, phase_wide_kernel)
Per kernel: vector / scalar instruction counts, plain v_mov_b32, DPP moves, v_readlane + v_readfirstlane, v_xor / v_bitop3, v_mad_u64_u32, v_cndmask,
s_nop, s_waitcnt, global loads / stores, and the resource lines of the kernel descriptor (VGPR, SGPR, scratch, LDS).
What profiles/issue_slots_isa.txt was written from."""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.check_output(["c++filt"] + names).decode().splitlines()
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """-> {symbol: (instruction lines, {resource: value})}"""
    out, cur, body = {}, None, []
    res = {}
    with open(path) as f:
        for line in f:
            s = line.strip()
            m = re.match(r"^\.amdhsa_kernel (\S+)", s)          # (the descriptor's directives stand inside the function's extent)
            if m:
                last = m.group(1)
                res[last] = {}
            m = re.match(r"^\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size) (\d+)", s)
            if m:
                res[last][m.group(1)] = int(m.group(2))
            m = re.match(r"^(_Z\w+):", s)
            if m and cur is None:
                cur, body = m.group(1), []
                continue
            if cur is not None:
                if s.startswith(".Lfunc_end"):
                    out[cur] = body
                    cur = None
                    continue
                if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
                    continue
                body.append(s.split(";")[0].strip())
    return {k: (v, res.get(k, {})) for k, v in out.items()}


def count(body):
    op = [b.split()[0] for b in body]
    n = lambda pred: sum(1 for i, o in enumerate(op) if pred(o, body[i]))
    return dict(
        total=len(op),
        vector=n(lambda o, b: o.startswith("v_")),
        scalar=n(lambda o, b: o.startswith("s_") and o not in ("s_nop", "s_waitcnt")),
        mov=n(lambda o, b: o == "v_mov_b32_e32" or o == "v_mov_b32_e64"),
        mov64=n(lambda o, b: o.startswith("v_mov_b64")),
        dpp=n(lambda o, b: o.endswith("_dpp")),
        readlane=n(lambda o, b: o.startswith("v_readlane") or o.startswith("v_readfirstlane")),
        xor=n(lambda o, b: o.startswith("v_xor_b32")),
        bitop3=n(lambda o, b: o.startswith("v_bitop3")),
        mad64=n(lambda o, b: o.startswith("v_mad_u64_u32")),
        cndmask=n(lambda o, b: o.startswith("v_cndmask")),
        lshl_add_u64=n(lambda o, b: o.startswith("v_lshl_add_u64")),
        s_nop=n(lambda o, b: o == "s_nop"),
        s_waitcnt=n(lambda o, b: o == "s_waitcnt"),
        s_load=n(lambda o, b: o.startswith("s_load") or o.startswith("s_buffer_load")),
        vmem_load=n(lambda o, b: o.startswith("global_load") or o.startswith("flat_load")),
        vmem_store=n(lambda o, b: o.startswith("global_store") or o.startswith("flat_store")),
        scratch=n(lambda o, b: o.startswith("scratch_") or o.startswith("buffer_")),
        lds=n(lambda o, b: o.startswith("ds_")),
    )


if __name__ == "__main__":
    path = sys.argv[1]
    flt = sys.argv[2:] or ["phase_fused_kernel", "phase_wide_kernel"]
    ks = kernels(path)
    names = demangle(list(ks))
    for sym in sorted(ks, key=lambda s: names[s]):
        nm = names[sym]
        if not any(f in nm for f in flt):
            continue
        body, res = ks[sym]
        c = count(body)
        print(re.sub(r"\(.*", "", nm.replace("void bpm::", "")))
        print("   " + "  ".join("%s=%d" % kv for kv in c.items()))
        print("   " + "  ".join("%s=%d" % kv for kv in sorted(res.items())))
