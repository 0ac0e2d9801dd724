"""The description of what a plan's step clears (alphabeta_rs_amd/csrc/abn_prepare.hpp) without a device: the ranges
abn_step_prepare_kernel fills in one launch, against a serial host model of the memsets that launch replaces — for a sweep
of chain counts, FIFO capacities, eligible or not, early run or not, two-pass, sweep counters.  The checks are those of
tests/native/step_prepare_main.cpp (the same union of bytes, each with its fill byte; no byte twice; nothing past a buffer
whose heap block is exactly its length; what each list is said to leave clear against the bytes it wrote; an overflowing
list reported); here the program is built and run, plain and under the host sanitizers."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "step_prepare_main.cpp"


def gxx():
    g = shutil.which("g++")
    if g is None:
        pytest.fail("g++ is needed to build tests/native/step_prepare_main.cpp")
    return g


def test_description_matches_the_memsets_it_replaces(tmp_path):
    exe = tmp_path / "step_prepare_main"
    r = subprocess.run([gxx(), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "list"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "step prepare ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert lines and all(ln.endswith(": ok") for ln in lines), [ln for ln in lines if not ln.endswith(": ok")][:5]
    seen = {tuple(int(v) for v in re.findall(r"(?:eligible|early|two_pass|sweep) (\d)", ln)) for ln in lines}
    assert {(1, 1, 0, 0), (1, 0, 0, 0), (0, 0, 0, 0), (0, 0, 1, 1)} <= seen, sorted(seen)
    # the benchmark's plan (one window, 10 000 bootstraps): the redo's region is what an eligible plan grows by
    caps = {int(m.group(1)): int(m.group(2)) for ln in lines
            for m in [re.search(r"chains 10000 cap (\d+) eligible 1 early 1 two_pass 0 sweep 0 fifo_bytes (\d+)", ln)] if m}
    assert caps == {6596: 2 * 64 * (192 + 6596) * 4}, caps
    # the clean record derived from each list (prep_clean) was set against the bytes that list wrote: prep_step and both
    # prep_phase lists of every case, and the prep_launch lists of the cases that have them; an overflowing list says so
    m = re.search(r"clean record: (\d+) lists checked, (\d+) ranges claimed clear", r.stdout)
    assert m, r.stdout[-1500:]
    launch_cases = [ln for ln in lines if " early 0 two_pass 0 sweep 0 " in ln]
    assert int(m.group(1)) >= 3 * len(lines) + 3 * len(launch_cases) and int(m.group(2)) >= int(m.group(1)), m.group(0)
    assert re.search(r"overflow of \d+ ranges reported: ok", r.stdout), r.stdout[-1500:]


def test_description_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly, nothing preloaded): host code only."""
    exe = tmp_path / "step_prepare_main_san"
    r = subprocess.run([gxx(), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "step prepare ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
