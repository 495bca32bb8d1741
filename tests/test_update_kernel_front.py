"""The planned front of the one-wavefront-per-chain update kernels (bipymc_amd/csrc/kernels.h: plan_front), read from the disassembly of the
product library's gfx950 code object -- no GPU needed.

A wavefront of a PLAN flavour (HOT 1, 3, 5: records are the only path, kernels.h: choose_flavour) has to request its own row and its 2 NP
partner rows after ONE scalar round trip: the record and the first lines of the argument block behind one `s_waitcnt lgkmcnt`, then the
1 + 2 NP `global_load_dwordx4`.  Scalar loads return out of order, so every scalar wait waits for everything outstanding: each further
wait ahead of the rows is a first-touch miss the row fetch stands behind (three of them before the front was reordered).  And the
steady-state flavour carries no in-kernel draw path any more: its `perm_tab` lookup was the only 4-byte vector load ahead of the rows."""
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


@pytest.fixture(scope="module")
def fronts():
    """{(algo, np, hot): mnemonic lines from behind the kernarg-preload prologue up to and including the (1 + 2 NP)-th 16-byte vector load}"""
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
    chunks = re.split(r"^[0-9a-f]+ (?=<)", asm, flags=re.M)
    for ch in chunks:
        m = _NAME.match(ch)
        if not m:
            continue
        algo, np_, hot = int(m.group(2)), int(m.group(3)), int(m.group(4))
        ins = [ln.split("//")[0].strip() for ln in ch.split("\n")[1:]]
        ins = [x for x in ins if x and not x.startswith("<") and not x.endswith(":")]
        # the preload prologue: the block ending in s_branch ahead of the 256-byte alignment
        first_branch = next(i for i, x in enumerate(ins) if x.startswith("s_branch"))
        assert first_branch < 8, (m.group(1), ins[:10])
        body = ins[first_branch + 1:]
        front, rows = [], 0
        for x in body:
            front.append(x)
            if x.startswith("global_load_dwordx4"):
                rows += 1
                if rows == 1 + 2 * np_:
                    break
        assert rows == 1 + 2 * np_, (m.group(1), rows)
        out[(algo, np_, hot)] = front
    return out


def test_every_plan_flavour_of_the_shape_is_in_the_library(fronts):
    # DE-MC (one pair) steady / rank of a world; DREAM with three pairs and with a run-time pair count: steady, adapting, rank of a world
    assert sorted(fronts) == [(0, 1, 1), (0, 1, 5), (1, 0, 1), (1, 0, 3), (1, 0, 5), (1, 3, 1), (1, 3, 3), (1, 3, 5)], sorted(fronts)


def test_rows_are_requested_after_one_scalar_round_trip(fronts):
    for key, front in sorted(fronts.items()):
        waits = [x for x in front if x.startswith("s_waitcnt") and "lgkmcnt" in x]
        print(key, "scalar waits ahead of the row loads:", len(waits), "instructions ahead of them:", len(front))
        assert len(waits) <= 1, (key, waits, front)


def test_steady_state_flavour_has_no_in_kernel_draw_path_ahead_of_the_rows(fronts):
    for key, front in sorted(fronts.items()):
        if key[2] != 1:
            continue
        lookups = [x for x in front if x.startswith("global_load_dword ")]
        assert not lookups, (key, lookups)
