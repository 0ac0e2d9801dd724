"""The compiled observation kernel (csrc/abn_sim.hpp, built in abn_sim.hip) and census kernels (csrc/abn_packed_census.hpp,
built in abn_pairwise.hip) keep what they hold in registers: no scratch memory; the observation kernel uses no LDS — its
eighteen threshold words are kernel arguments chosen by selects, not an indexed array — and the census kernel no more than
its reduction buffer.  A condition on the emitted gfx950 metadata, not a measurement."""
import re

from _device_isa import CSRC, device_isa


def _kernels(isa, family):
    """name -> descriptor of every kernel of the family"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (_Z\w+)\n(.*?)^\s*\.end_amdhsa_kernel", isa, re.S | re.M):
        if family in m.group(1):
            out[m.group(1)] = m.group(2)
    return out


def _sizes(desc, name):
    private = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc)
    group = re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc)
    assert private and group, name
    for flag in re.findall(r"\.amdhsa_(?:enable_private_segment|uses_dynamic_stack|"
                           r"system_sgpr_private_segment_wavefront_offset)\s+(\d+)", desc):
        assert int(flag) == 0, name
    return int(private.group(1)), int(group.group(1))


def test_observation_kernel_uses_no_scratch_and_no_lds():
    kernels = _kernels(device_isa(src=CSRC / "abn_sim.hip"), "abn_sim_observe_kernel")
    assert len(kernels) == 2, sorted(kernels)          # lazy, and the variant that always draws the low words
    for name, desc in kernels.items():
        assert _sizes(desc, name) == (0, 0), name


def test_census_kernels_use_no_scratch_and_only_the_reduction_buffer():
    isa = device_isa(src=CSRC / "abn_pairwise.hip")
    source = (CSRC / "abn_packed_census.hpp").read_text()
    assert "kCensusThreads = 256;" in source and "kCensusRedWords = 3 * (kCensusThreads / 64);" in source
    words = 3 * (256 // 64)                            # the reduction buffer: three counts of each of the four wavefronts
    count = _kernels(isa, "abn_packed_census_kernel")
    total = _kernels(isa, "abn_packed_census_sum_kernel")
    assert len(count) == 1 and len(total) == 1, (sorted(count), sorted(total))
    for name, desc in count.items():
        private, group = _sizes(desc, name)
        assert private == 0 and 0 < group <= 4 * words, name
    for name, desc in total.items():
        assert _sizes(desc, name) == (0, 0), name
