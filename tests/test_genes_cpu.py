"""The gene choice in blocks (alphabeta_rs_amd/csrc/abn_genes.hpp) without a device: the three phases the kernels run, in
their serial host form (abh_choose_genes_blocked of host_capi.cpp), against the serial loop of the reference as
tests/_windows_model.py restates it — gene_start, gene_end and flags, element for element, at block lengths 1, 2, 3, 64
and 1024."""
import shutil
from pathlib import Path
import subprocess

import numpy as np
import pytest

import _genes_model as G

BLOCKS = (1, 2, 3, 64, 1024)


def check(L, case, label):
    off, _, _, _, _, gs, ge, fl = case.want()
    for b in BLOCKS:
        o, s, e, f = G.host_choose_blocked(L, case, b)
        assert np.array_equal(o, off), (label, b)
        assert np.array_equal(s, gs) and np.array_equal(e, ge) and np.array_equal(f, fl), (label, b)


def test_hand_made_cases_at_every_block_length():
    L = G.hostlib()
    cases = G.hand_cases()
    for name, case in cases.items():
        check(L, case, name)
    # the cases do what their descriptions say
    off, _, _, _, _, gs, _, fl = cases["sample_boundary"].want()
    assert gs[off[1] - 1] == 1000 and gs[off[1]] == 2500 and fl[off[2]] == 0
    off, _, _, _, _, gs, _, fl = cases["block_edges"].want()
    s = off[6]
    assert list(gs[s + 1022:s + 1026]) == [10_000, 50_000, 90_000, 10_000] and fl[s + 2047] == 0 and fl[s + 2048] == 2
    _, _, _, _, strand, gs, _, fl = cases["strands"].want()
    assert set(gs[:1100]) == {0, 1000, 1200} and np.all(gs[400:600:2] == 1000) and np.all(gs[401:600:2] == 1200)   # in turn
    o = cases["strands"].want()[0][1]
    assert list(gs[o:o + 4]) == [1000] * 4 and list(strand[o:o + 3]) == [2, 0, 1]   # the `*` gene kept by + and -
    assert 0 < (cases["wrap_cutoff"].want()[7] & 2).sum() < len(cases["wrap_cutoff"].want()[7])
    assert 0 < (cases["wrap_gene_length"].want()[7] & 2).sum() < len(cases["wrap_gene_length"].want()[7])


def test_seeded_cases_at_every_block_length():
    L = G.hostlib()
    with_gene = 0
    for seed in range(300):
        case = G.random_case(seed, 1500, 80)
        check(L, case, seed)
        with_gene += int((case.want()[7] & 2).sum())
    assert with_gene > 10_000


def test_block_length_is_checked():
    L = G.hostlib()
    case = G.Case(G.gene_line(1, 10, 20, "+"), [G.text([G.cg(1, 15, "+")])])
    for bad in (0, -1, 65535):
        texts = (G.C.c_char_p * 1)(case.texts[0].encode())
        lens = (G.C.c_longlong * 1)(len(case.texts[0]))
        off = (G.C.c_longlong * 2)()
        assert L.abh_choose_genes_blocked(b"", 0, texts, lens, 1, 0, 0, bad, 8, off, None, None, None) == -2


def test_block_phases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the three phases over seeded cases at several block lengths,
    every array in a heap block of exactly its length, against the serial loop, built with -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for the sanitizer build of tests/native/genes_blocks_main.cpp")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "genes_blocks_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o",
                        str(exe), str(root / "tests" / "native" / "genes_blocks_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sanitized gene blocks ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
