"""The emitted gfx950 code of the block bootstrap's kernels (alphabeta_rs_amd/csrc/abn_blocks.hip; compile only): the
product and the counts kernel use no scratch memory, and the product runs on the 8-bit matrix instruction."""
import re

import pytest

from _device_isa import CSRC, device_isa

KERNELS = ("abn_block_gemm_kernel", "abn_block_counts_kernel")


@pytest.fixture(scope="module")
def isa():
    return device_isa(CSRC / "abn_blocks.hip")


def metadata(isa, kernel):
    """the .amdhsa_ directives of the kernel whose mangled name holds `kernel` -> {directive: value}"""
    m = re.search(r"\.amdhsa_kernel (\S*%s\S*)\n(.*?)\.end_amdhsa_kernel" % kernel, isa, flags=re.S)
    assert m, kernel
    return m.group(1), dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))


def body(isa, name):
    start = isa.index(f"\n{name}:")
    return isa[start:isa.index(".end_amdhsa_kernel", start)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(isa, kernel):
    name, meta = metadata(isa, kernel)
    assert int(meta["private_segment_fixed_size"]) == 0, meta
    text = body(isa, name)
    assert not re.search(r"^\s*scratch_", text, flags=re.M)
    note = re.search(r"- \.agpr_count:.*?\.name:\s+%s\n.*?\.vgpr_spill_count:\s+(\d+)" % re.escape(name), isa, flags=re.S)
    assert note and int(note.group(1)) == 0


def test_the_product_is_on_the_matrix_pipe_without_global_atomics(isa):
    name, _ = metadata(isa, "abn_block_gemm_kernel")
    text = body(isa, name)
    assert len(re.findall(r"v_mfma_i32_16x16x64_i8", text)) >= 10
    assert not re.search(r"global_atomic|flat_atomic", text)
