"""The kernarg lines the planned front of the one-wavefront-per-chain update kernels waits for (bipymc_amd/csrc/kernels.h: PhaseArgs, its hot block),
read from the disassembly of the product library's gfx950 code object -- no GPU needed.

A wavefront of a PLAN flavour gathers the update record and the fields of the argument block it reads on its way to the accept test behind ONE
`s_waitcnt lgkmcnt`.  Every 64-byte line of the kernarg segment is a first touch in a fresh slot behind the packet's acquire, and scalar loads return
out of order: the wait lasts as long as the slowest line.  So a flavour's fields have to lie in as few lines as their bytes need, and be fetched with
few wide loads.  Kernarg slots are 64-byte aligned (aql_queue.h: SLOT_BYTES = 3072), so a line of the segment is a line of memory.

_HOT_BYTES is profiles/arg_lines.txt's table: the bytes of the fields each flavour's front gathers ahead of its first wait (read from the disassembly of
the library before the block was packed; kernels.h: PhaseArgs maps them),
  every flavour  L.G 8, L.ld 4, L.dim 4, ll 8, acc_count 8, tparams 8, counters 8, hist_row 8, llhist_row 8, seed 8, t 8, k 4, upd_off 4, epsilon 8,
                 wt 4, hist_by_pos 4                                                                               = 104
  DREAM          cr_state 8, gamma_tab 8, u_epsilon 8, thr[0..3] 16                                                =  40
  burn-in        w_mean 8, w_m2 8, cr_gate 4, hist_len 4; cr_fold_nb 4, cr_chunk0 4, cr_n1 4, adapt_on 4 (the geometry of the CR sums, which the
                 flavour's workgroups read on every path: the compiler loads it at the kernel's entry)             =  40
  rank of world  lo 4, the rest of the Layout (blk 8, n_local 4, world 4, magic 4, padding 4)                      =  28
  DE-MC          gamma_demc 8, p_snooker 8, M 4, pool_off 4                                                        =  24
and the bound is what that many bytes need when they start where the block starts: ceil((_BLOCK_AT + bytes) / 64) lines."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# phase_fused_kernel<ALGO, TARGET_GAUSS = 1, LPC = 64, DPL = 2, NP, HOT>
_NAME = re.compile(r"<(_ZN3bpm\w*phase_fused_kernelILi(\d+)ELi1ELi64ELi2ELi(\d+)ELi([135])EEE\w*)>:")
_SLOAD = re.compile(r"s_load_dword(?:x(\d+))?\s+\S+,\s*s\[(\d+):\d+\],\s*(0x[0-9a-f]+|\d+)$")
_ADD = re.compile(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+|\d+)$")
_ADDC = re.compile(r"s_addc_u32 s(\d+), s(\d+), 0$")
_SDST = re.compile(r"(?:s_(?!cmp|bitcmp|cbranch|branch|waitcnt|nop|barrier|setprio|sleep)\w+|v_readfirstlane_b32|v_readlane_b32)\s+s(?:\[(\d+):(\d+)\]|(\d+))")
_LINE = 64
_BLOCK_AT = 24      # offsetof(FusedKernarg, a) (sampler.hip): the leading arguments arrive preloaded, the argument block -- its hot block first -- follows
_COMMON, _DREAM, _ADAPT, _SHARD, _DEMC = 104, 40, 40, 28, 24


def _hot_bytes(algo, hot):
    return _COMMON + (_DREAM if algo == 1 else _DEMC) + (_ADAPT if hot == 3 else 0) + (_SHARD if hot == 5 else 0)


_FLAVOURS = [(0, 1, 1), (0, 1, 5), (1, 0, 1), (1, 0, 3), (1, 0, 5), (1, 3, 1), (1, 3, 3), (1, 3, 5)]
_HOT_BYTES = {key: _hot_bytes(key[0], key[2]) for key in _FLAVOURS}


@pytest.fixture(scope="module")
def first_waits():
    """{(algo, np, hot): [(offset, bytes)] of the s_loads off the kernarg pointer behind the preload prologue and ahead of the first scalar wait}"""
    from kernel_resources import LLVM
    so = os.path.join(ROOT, "bipymc_amd", "libbipymc_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bipymc_amd", "csrc")])
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "k.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(td, "x.so")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        asm = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co]).decode()
    out = {}
    for ch in re.split(r"^[0-9a-f]+ (?=<)", asm, flags=re.M):
        m = _NAME.match(ch)
        if not m:
            continue
        key = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
        ins = [ln.split("//")[0].strip() for ln in ch.split("\n")[1:]]
        ins = [x for x in ins if x and not x.startswith("<") and not x.endswith(":")]
        first_branch = next(i for i, x in enumerate(ins) if x.startswith("s_branch"))      # (the end of the preload prologue)
        # the kernarg pointer arrives in s[0:1]; the compiler may keep "pointer + constant" in another pair and load off that: {low register: offset}
        loads, waited, ptrs, pending = [], False, {0: 0}, None
        for x in ins[first_branch + 1:]:
            if x.startswith("s_waitcnt") and "lgkmcnt" in x:
                waited = True
                break
            ld, add, addc = _SLOAD.match(x), _ADD.match(x), _ADDC.match(x)
            if ld and int(ld.group(2)) in ptrs:
                loads.append((ptrs[int(ld.group(2))] + int(ld.group(3), 0), 4 * int(ld.group(1) or 1)))
            new_ptr = None
            if add and int(add.group(2)) in ptrs:
                pending = (int(add.group(1)), int(add.group(2)), ptrs[int(add.group(2))] + int(add.group(3), 0))
            elif addc and pending and (int(addc.group(1)), int(addc.group(2))) == (pending[0] + 1, pending[1] + 1):
                new_ptr, pending = (pending[0], pending[2]), None
            dst = _SDST.match(x)
            if dst:      # whatever this instruction writes is a kernarg pointer no longer
                lo, hi = (int(dst.group(1)), int(dst.group(2))) if dst.group(1) else (int(dst.group(3)), int(dst.group(3)))
                if not (add and pending and pending[0] == lo) and new_ptr is None:
                    ptrs = {r: o for r, o in ptrs.items() if r + 1 < lo or r > hi}
            if new_ptr:
                ptrs[new_ptr[0]] = new_ptr[1]
        assert waited, m.group(1)
        out[key] = sorted(loads)
    return out


def _lines(loads):
    return sorted({ln for off, n in loads for ln in range(off // _LINE, (off + n - 1) // _LINE + 1)})


def test_every_plan_flavour_of_the_shape_is_read(first_waits):
    assert sorted(first_waits) == _FLAVOURS, sorted(first_waits)


@pytest.mark.parametrize("key", _FLAVOURS)
def test_first_wait_touches_no_more_lines_than_its_bytes_need(first_waits, key):
    loads = first_waits[key]
    lines = _lines(loads)
    bound = -(-(_BLOCK_AT + _HOT_BYTES[key]) // _LINE)
    print(key, "hot bytes", _HOT_BYTES[key], "bound", bound, "lines", lines, "loads", ["0x%x+%d" % ld for ld in loads], "bytes loaded", sum(n for _, n in loads))
    assert loads and min(off for off, _ in loads) >= _BLOCK_AT, (key, loads)      # (the leading arguments are preloaded, never loaded)
    assert len(lines) <= bound, (key, lines, bound, loads)
    assert len(loads) <= len(lines) + 1, (key, loads, lines)
