"""The persistent fit kernel's common step carries no register-spill traffic (emitted gfx950 ISA; CPU tier, ~45 s once).

abn_fit_refill_kernel runs its common step — evaluation, decisions, insertion, begin_iteration, the two polls — in an
inner loop between two marker comments (`abn: hot step begin` / `abn: hot step end`, csrc/abn_fit_refill.hpp).  Before
that loop existed the register allocator parked some forty scalar registers per step in lanes of two vector registers
(v_readlane_b32 / v_writelane_b32: 290-478 / 111-136 per instantiation, up to 60 bytes of scratch), because everything
the cold part uses — finish, park, publish, claim, resume, set-up — was live across every step.  The results do not
change with any of this, so only the listing can hold it in place.  For every instantiation:

  1. no v_readlane_b32 / v_writelane_b32 in the hot loop,
  2. no scratch access in the hot loop,
  3. no call (s_swappc_b64) and no indirect jump (s_setpc_b64) anywhere in the kernel,
  4. no more vector registers than before the change (PARENT_VGPRS) and at most 106 scalar registers.

The hot loop is the text between the two markers plus every basic block the assembler's comments assign to the loop whose
header holds the first marker (the loop's exit test is laid out in front of the header).
"""
import re

import pytest

import _device_isa

BEGIN, END = "abn: hot step begin", "abn: hot step end"
# (G, R): vector registers of the instantiation before the step got a loop of its own (docs/experiments.md)
PARENT_VGPRS = {(8, 1): 167, (8, 2): 167, (8, 4): 168, (8, 8): 168, (16, 1): 166, (16, 2): 166, (16, 4): 168, (16, 8): 168,
                (32, 1): 166, (32, 2): 166, (32, 4): 168, (32, 8): 168, (64, 1): 166, (64, 2): 166, (64, 4): 168, (64, 8): 168}
MAX_SGPRS = 106


@pytest.fixture(scope="module")
def kernels():
    """{(G, R): (lines of the kernel's text, comments included; its resource comment block)}"""
    isa = _device_isa.device_isa()
    out = {}
    for m in re.finditer(r"^(_ZN3abn21abn_fit_refill_kernelILi(\d+)ELi(\d+)EEEvNS_7FitArgsE):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?; ScratchSize: \d+)",
                         isa, re.S | re.M):
        out[(int(m.group(2)), int(m.group(3)))] = ([ln.strip() for ln in m.group(4).splitlines() if ln.strip()], m.group(5))
    assert sorted(out) == sorted(PARENT_VGPRS), sorted(out)
    return out


def hot_loop(lines):
    """the instruction lines of the hot loop: between the markers, and in the blocks of the loop the first marker's block heads"""
    b = [i for i, ln in enumerate(lines) if BEGIN in ln]
    e = [i for i, ln in enumerate(lines) if END in ln]
    assert len(b) == 1 and len(e) == 1 and b[0] < e[0], (b, e)
    label = re.compile(r"^\.(LBB\d+_\d+):")
    header = next(label.match(lines[i]).group(1) for i in range(b[0], -1, -1) if label.match(lines[i]))
    member = re.compile(r"in Loop: Header=" + header[1:] + r"\b")
    hot, inside = [], False
    for i, ln in enumerate(lines):
        if label.match(ln):
            inside = bool(member.search(ln))
        if (inside or b[0] <= i <= e[0]) and not ln.startswith((";", ".")):
            hot.append(ln)
    return hot


def test_hot_loop_is_found_and_is_the_step(kernels):
    """the markers enclose the whole evaluation: P2's table, P3's packed reads and the barriers are in the loop found"""
    for key, (lines, _) in kernels.items():
        hot = hot_loop(lines)
        assert 800 < len(hot) < len(lines), (key, len(hot))
        assert sum(ln.startswith("ds_read_b128") for ln in hot) >= 2, key
        assert sum(ln.startswith("v_mul_f64") for ln in hot) > 50, key
        assert any(ln.startswith("v_div_scale_f64") for ln in hot), key     # begin_iteration's division by 5


def test_no_lane_spill_and_no_scratch_in_the_hot_loop(kernels):
    for key, (lines, _) in kernels.items():
        hot = hot_loop(lines)
        lanes = [ln for ln in hot if ln.startswith(("v_readlane_b32", "v_writelane_b32"))]
        assert not lanes, (key, lanes)
        scratch = [ln for ln in hot if ln.startswith("scratch_")]
        assert not scratch, (key, scratch)


def test_no_call_in_the_kernel(kernels):
    for key, (lines, _) in kernels.items():
        calls = [ln for ln in lines if ln.startswith(("s_swappc_b64", "s_setpc_b64"))]
        assert not calls, (key, calls)


def test_registers_not_above_the_parent(kernels):
    for key, (_, resources) in kernels.items():
        vgprs = int(re.search(r"; NumVgprs: (\d+)", resources).group(1))
        sgprs = int(re.search(r"; TotalNumSgprs: (\d+)", resources).group(1))
        print(key, "vgprs", vgprs, "sgprs", sgprs)
        assert vgprs <= PARENT_VGPRS[key], (key, vgprs)
        assert sgprs <= MAX_SGPRS, (key, sgprs)
