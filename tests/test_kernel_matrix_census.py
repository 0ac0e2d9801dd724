"""Census of the compiled fit-path instantiations (CPU tier: the gfx950 assembly cross-compiles without a GPU).

abn_api.hip's C-ABI dispatches to 103 template instantiations of abn_fit_kernel, abn_fit_refill_kernel,
abn_fit_spec_kernel and abn_cost_kernel.  Each one must be in exactly one of tests/_kernel_matrix.py's tables: MATRIX
(a GPU case of tests/test_gpu_kernel_matrix.py whose inputs route to it) or UNREACHABLE (with the host condition that
rules it out).  A new instantiation — a new `case` of a dispatch switch, a new template argument — fails here until it
gets a case or a reason; a table entry the assembly no longer has fails too.
"""
import importlib.util
import re
from pathlib import Path

import pytest


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_device_isa = _load("_device_isa")
KM = _load("_kernel_matrix")
FAMILIES = ("abn_fit_kernel", "abn_fit_refill_kernel", "abn_fit_spec_kernel", "abn_cost_kernel")


def census(isa):
    """{key: mangled name} of every fit-path kernel the assembly defines; a name of these families that does not decode
    is an error (the regexes would otherwise let a new template argument slip past)"""
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", isa, re.M):
        if not any(f in name for f in FAMILIES):
            continue
        key = KM.decode(name)
        assert key is not None, f"undecodable fit-path kernel {name}"
        assert key not in out, (name, out.get(key))
        out[key] = name
    return out


def partition_errors(keys, matrix, unreachable):
    errs = [f"in both tables: {KM.label(k)}" for k in set(matrix) & set(unreachable)]
    errs += [f"no case and no reason: {KM.label(k)}" for k in sorted(set(keys) - set(matrix) - set(unreachable), key=str)]
    errs += [f"not in the assembly: {KM.label(k)}" for k in sorted((set(matrix) | set(unreachable)) - set(keys), key=str)]
    errs += [f"no reason given: {KM.label(k)}" for k, why in unreachable.items() if not (isinstance(why, str) and why.strip())]
    return errs


@pytest.fixture(scope="module")
def kernels():
    return census(_device_isa.device_isa())


def test_every_instantiation_has_a_case_or_a_reason(kernels):
    assert len(kernels) == 103, sorted(map(KM.label, kernels))
    assert partition_errors(kernels, KM.MATRIX, KM.UNREACHABLE) == []
    assert len(KM.MATRIX) + len(KM.UNREACHABLE) == len(kernels)
    fams = {}
    for k in kernels:
        fams[k[0]] = fams.get(k[0], 0) + 1
    assert fams == {KM.FIT: 71, KM.REFILL: 16, KM.SPEC: 12, KM.COST: 4}, fams
    for k, why in KM.UNREACHABLE.items():
        assert "abn_api.hip" in why or "launch_fit" in why, (KM.label(k), why)


def test_census_is_not_vacuous(kernels):
    """the partition check fails on an instantiation without a table entry and on an entry without an instantiation"""
    some_reason = next(iter(KM.UNREACHABLE))
    fewer = {k: v for k, v in KM.UNREACHABLE.items() if k != some_reason}
    assert partition_errors(kernels, KM.MATRIX, fewer) == [f"no case and no reason: {KM.label(some_reason)}"]
    some_case = next(iter(KM.MATRIX))
    assert partition_errors(kernels, {k: v for k, v in KM.MATRIX.items() if k != some_case}, KM.UNREACHABLE) == \
        [f"no case and no reason: {KM.label(some_case)}"]
    ghost = (KM.FIT, 128, 1, False, False, False)
    assert partition_errors(kernels, {**KM.MATRIX, ghost: {}}, KM.UNREACHABLE) == [f"not in the assembly: {KM.label(ghost)}"]
    assert partition_errors(kernels, KM.MATRIX, {**KM.UNREACHABLE, some_reason: ""}) == \
        [f"no reason given: {KM.label(some_reason)}"]
    assert partition_errors(kernels, KM.MATRIX, {**KM.UNREACHABLE, some_case: "x"}) == \
        [f"in both tables: {KM.label(some_case)}"]


def test_decode_reads_the_mangling():
    assert KM.decode("_ZN3abn14abn_fit_kernelILi16ELin1ELb0ELb0EEEvNS_7FitArgsE") == (KM.FIT, 16, -1, False, False, False)
    assert KM.decode("_ZN3abn14abn_fit_kernelILi64ELi16ELb1ELb0EEEvNS_7FitArgsE") == (KM.FIT, 64, 16, True, False, False)
    assert KM.decode("_ZN3abn21abn_fit_refill_kernelILi8ELi4EEEvNS_7FitArgsE") == (KM.REFILL, 8, 4, False, False, False)
    assert KM.decode("_ZN3abn19abn_fit_spec_kernelILi2ELb0ELb1EEEvNS_7FitArgsE") == (KM.SPEC, 64, 2, False, False, True)
    assert KM.decode("_ZN3abn15abn_cost_kernelILi32EEEvNS_8CostArgsE") == (KM.COST, 32, 0, False, False, False)
    assert KM.decode("_ZN3abn17abn_select_kernelENS_10SelectArgsE") is None


def test_case_table_covers_the_edges():
    """the cases together sit on every edge the issue of packed kernels names: ragged and full lane groups, T = 0..3 and
    large odd / even T, odd and even K, strict order on either side of 16 rows, every observation mode"""
    cases = list(KM.MATRIX.values())
    fits = [(k, c) for k, c in KM.MATRIX.items() if k[0] in (KM.FIT, KM.REFILL) and k[2] >= 1]
    assert any(c["n"] == k[1] * k[2] for k, c in fits) and any(c["n"] % k[1] == 1 for k, c in fits)
    ts = {c["tmax"] for c in cases}
    assert {0, 1, 2, 3} <= ts and any(t > 64 and t % 2 for t in ts) and any(t > 64 and t % 2 == 0 for t in ts)
    assert 127 in ts
    ks = {c["k"] % 2 for c in cases}
    assert ks == {0, 1}
    strict_n = [c["n"] for k, c in KM.MATRIX.items() if k[4]]
    assert min(strict_n) <= 16 < max(strict_n)
    modes = {c["opts"].get("stream_mode") for k, c in KM.MATRIX.items() if k[0] == KM.FIT and k[2] <= 0}
    assert modes == {0, 1}
    for k, c in KM.MATRIX.items():
        if c["route"] in ("plan", "twopass", "spec"):   # partly filled last wavefront at every packed width
            assert c["S"] % 8 and c["B"] % 8, KM.label(k)


@pytest.mark.parametrize("key", list(KM.MATRIX), ids=KM.label)
def test_case_routes_to_its_instantiation_and_tree(abn, key):
    """host arithmetic only: the case's pedigree has the T and K the case names, abn.reduction_tree equals the tree the
    case expects, and by the restated dispatch its route launches the instantiation it is filed under"""
    c = KM.MATRIX[key]
    ped = KM.pedigree(c)
    tmax, k, _ = KM.LDS.topology(ped)
    assert (ped.shape[0], tmax, k) == (c["n"], c["tmax"], c["k"])
    o = abn.default_options(**c["opts"])
    assert abn.reduction_tree(ped[:, :3], o) == KM.expected_tree(c["n"], c["tmax"], c["k"], c["opts"])
    assert key in KM.targets(c), [KM.label(t) for t in KM.targets(c)]
