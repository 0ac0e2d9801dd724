"""Builds libabneutral_hip.so (HIP kernels + C-ABI) for gfx950 with hipcc, in-tree.

-ffp-contract=off is REQUIRED: parity with the reference depends on every multiply-add staying
unfused except the explicit __builtin_fma calls (see csrc/abn_device.hpp).
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIB = PKG / "libabneutral_hip.so"
# the one list of the library's sources: scripts/flag_variants.py and scripts/stamps.py build from it too
SOURCES = [CSRC / "abn_api.hip", CSRC / "abn_context.hip", CSRC / "abn_plan.hip",  # the fit path: kernels and launchers, host-only, the plan
           CSRC / "abn_pairwise.hip", CSRC / "abn_windows.hip", CSRC / "abn_analyze.hip",
           CSRC / "abn_multi.hip", CSRC / "abn_sites.hip", CSRC / "abn_genes.hip", CSRC / "abn_codes.hip",
           CSRC / "abn_sites_common.hip", CSRC / "abn_sites_union.hip", CSRC / "abn_tiles.hip", CSRC / "abn_blocks.hip",
           CSRC / "abn_sites_sort.hip", CSRC / "abn_sites_dedup.hip", CSRC / "abn_sim.hip", CSRC / "abn_regions.hip",
           CSRC / "abn_resident.hip",  # host-only too: what the builders from resident parse results share
           CSRC / "abn_pack.cpp"]  # host-only: the packed code format (also built alone under the host sanitizers)
DEPS = [*sorted(CSRC.glob("*.hpp")), CSRC / "abn_philox.h", PKG.parent / "include" / "abneutral.h"]
HIPCC_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-ffp-contract=off",
    "-fno-fast-math",
    "-fPIC",
    "-shared",
    "-Wall",
    "-ldl",
]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found: the ABneutral HIP library cannot be built")


def needs_build() -> bool:
    if not LIB.exists():
        return True
    t = LIB.stat().st_mtime
    return any(p.stat().st_mtime > t for p in SOURCES + DEPS)


def build_hip(force: bool = False, verbose: bool = False) -> Path:
    if not force and not needs_build():
        return LIB
    cmd = [hipcc_path(), *HIPCC_FLAGS, "-o", str(LIB), *map(str, SOURCES)]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=str(PKG))
    return LIB


KNOBS_LIB = PKG.parent / "build" / "libabn_knobs.so"


def build_knobs(force: bool = False, verbose: bool = False) -> Path:
    """The same sources with -DABN_MEASUREMENT_KNOBS (environment switches for the sweeps under scripts/ and the fault
    injection of tests/test_gpu_parity.py::test_lost_fifo_entry_is_an_error_at_sync).  Never loaded by the product: the
    package takes it only through ABNEUTRAL_HIP_LIB."""
    if not force and KNOBS_LIB.exists() and all(p.stat().st_mtime <= KNOBS_LIB.stat().st_mtime for p in SOURCES + DEPS):
        return KNOBS_LIB
    KNOBS_LIB.parent.mkdir(exist_ok=True)
    cmd = [hipcc_path(), *HIPCC_FLAGS, "-DABN_MEASUREMENT_KNOBS", "-o", str(KNOBS_LIB), *map(str, SOURCES)]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=str(PKG))
    return KNOBS_LIB


HOST = PKG / "host"
CLI = PKG / "bin" / "alphabeta"
META_CLI = PKG / "bin" / "metaprofile_alphabeta"
REF_TESTS = PKG / "bin" / "reference_tests"
PEDIGREE_LIB = PKG / "libabneutral_host.so"


def build_host(force: bool = False, verbose: bool = False) -> Path:
    """The C++ host layer: the `alphabeta` CLI (reference flags and output files) and a small shared
    library exposing Pedigree::build to the tests.  Both link libabneutral_hip.so via $ORIGIN rpaths."""
    build_hip()
    srcs = [HOST / "alphabeta_cli.cpp", HOST / "alphabeta.hpp", HOST / "pedigree_build.hpp", HOST / "windows_extract.hpp",
            HOST / "resident.hpp", HOST / "host_capi.cpp", HOST / "block_bootstrap.hpp",
            HOST / "metaprofile.hpp", HOST / "metaprofile_cli.cpp", HOST / "reference_tests.cpp",
            CSRC / "abn_route.hpp", CSRC / "abn_constants.hpp", CSRC / "abn_parse.hpp", CSRC / "abn_genes.hpp",
            CSRC / "abn_sites_merge.hpp", CSRC / "abn_sites_split.hpp", CSRC / "abn_sites_sort.hpp", CSRC / "abn_sites_dedup.hpp", CSRC / "abn_codes.hpp", CSRC / "abn_sites_common.hpp",
            CSRC / "abn_sites_union.hpp", CSRC / "abn_tiles.hpp", HOST / "tiles.hpp", HOST / "region_states.hpp",
            CSRC / "abn_pairwise_transitions.hpp", CSRC / "abn_packed_mask.hpp", HOST / "transitions.hpp", CSRC / "abn_sim.hpp", CSRC / "abn_philox.h",
            CSRC / "abn_packed_census.hpp", CSRC / "abn_regions.hpp",
            HOST / "simulate.hpp"]  # host_capi.cpp exports the launch policy to the tests
    newest = max(p.stat().st_mtime for p in srcs)
    CLI.parent.mkdir(exist_ok=True)
    common = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", str(PKG.parent / "include")]
    if force or not CLI.exists() or CLI.stat().st_mtime < newest:
        cmd = [hipcc_path(), *common, "-o", str(CLI), str(HOST / "alphabeta_cli.cpp"), "-L", str(PKG),
               "-labneutral_hip", "-Wl,-rpath,$ORIGIN/.."]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=str(PKG))
    if force or not META_CLI.exists() or META_CLI.stat().st_mtime < newest:
        cmd = [hipcc_path(), *common, "-o", str(META_CLI), str(HOST / "metaprofile_cli.cpp"), "-L", str(PKG),
               "-labneutral_hip", "-Wl,-rpath,$ORIGIN/.."]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=str(PKG))
    if force or not REF_TESTS.exists() or REF_TESTS.stat().st_mtime < newest:
        cmd = [hipcc_path(), *common, "-o", str(REF_TESTS), str(HOST / "reference_tests.cpp"), "-L", str(PKG),
               "-labneutral_hip", "-Wl,-rpath,$ORIGIN/.."]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=str(PKG))
    if force or not PEDIGREE_LIB.exists() or PEDIGREE_LIB.stat().st_mtime < newest:
        cmd = [hipcc_path(), *common, "-fPIC", "-shared", "-o", str(PEDIGREE_LIB), str(HOST / "host_capi.cpp"), "-L",
               str(PKG), "-labneutral_hip", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=str(PKG))
    return CLI


if __name__ == "__main__":
    print(build_hip(force=True, verbose=True))
    print(build_host(force=True, verbose=True))
