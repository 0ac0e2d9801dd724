"""The compiled transitions kernels (csrc/abn_pairwise_transitions.hpp, built in abn_pairwise.hip) keep their nine
accumulators per tile in registers: no scratch memory, and the products are on the matrix pipe.  A condition on the
emitted gfx950 assembly, not a measurement — accumulators spilled to scratch are how this kernel would silently become
useless."""
import re

from _device_isa import CSRC, device_isa

FAMILY = "abn_pairwise_trans_kernel"


def _kernels(isa):
    """name -> (body, descriptor) of every kernel of the family"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)^\s*\.end_amdhsa_kernel", isa, re.S | re.M):
        if FAMILY in m.group(1):
            out[m.group(1)] = (m.group(2), m.group(3))
    return out


def test_transitions_kernels_use_no_scratch_and_the_matrix_pipe():
    kernels = _kernels(device_isa(src=CSRC / "abn_pairwise.hip"))
    assert len(kernels) == 5, sorted(kernels)          # the off-diagonal kernel and the diagonal ones of 1..4 blocks
    for name, (body, desc) in kernels.items():
        size = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc)
        assert size and int(size.group(1)) == 0, name
        for flag in re.findall(r"\.amdhsa_(?:enable_private_segment|uses_dynamic_stack|"
                               r"system_sgpr_private_segment_wavefront_offset)\s+(\d+)", desc):
            assert int(flag) == 0, name
        assert "v_mfma_i32_16x16x64_i8" in body, name
