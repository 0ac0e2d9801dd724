"""The stream sweep (abn_sweep_kernel: a streamed chain's rows read once per Nelder-Mead iteration) on the CPU tier: the
four new symbols and their bindings, the routing through the shim's new entry — the sweep kernel where it applies, with
the chain stride and the LDS bytes worked out here; today's route, field for field, where it does not — and the two
instantiations in the cross-compiled code object, without scratch.  Metadata and kernel names only: no instruction is
searched for."""
import ctypes as C
import re

import numpy as np
import pytest

import _device_isa
import _route_model as RM
from _parity import synthetic_pedigree

CUS = 256
KERNEL_STREAM, KERNEL_STREAM_SWEEP, FAM_FIT, FAM_SWEEP = 4, 6, 0, 4
SWEEP_BLOCKS = 2 * RM.STREAM_BLOCKS                     # row blocks a lane of the sweep kernel's deep loop keeps in flight
SWEEP_DEEP_ROWS = SWEEP_BLOCKS * RM.STREAM_VEC * RM.WAVE  # rows of one trip of that loop: fewer take its pair loop (R = -1)
NAMES = ("kind", "family", "G", "R", "tp", "strict", "resume", "grid", "block", "lds", "chain_stride", "tree", "quantum",
         "tail_cap", "tail_R")
NEW_SYMBOLS = ("abn_plan_set_stream_sweep", "abn_plan_stream_sweep", "abn_multi_set_stream_sweep", "abn_fit_batch_sweep")


def test_library_exports_the_symbols_and_the_binding_has_the_methods(abn):
    L = abn.load_library(build_if_missing=True)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in abn.EXPORTED_SYMBOLS, name
    assert callable(abn.Plan.set_stream_sweep) and callable(abn.Plan.stream_sweep)
    assert callable(abn.Context.fit_batch_sweep)
    assert callable(abn.MultiPlan.set_stream_sweep)
    assert abn.KERNEL_NAMES[KERNEL_STREAM_SWEEP] == "stream_sweep"


class Shim:
    def __init__(self):
        from alphabeta_rs_amd import build as B

        B.build_host()
        L = C.CDLL(str(B.PEDIGREE_LIB))
        i, ll = C.c_int, C.c_longlong
        L.abh_route_launch.argtypes = [i, i, i, i, i, i, i, ll, i, i, i, i, C.POINTER(ll), C.c_char_p, i]
        L.abh_route_launch_sweep.argtypes = [i, i, i, i, i, i, i, ll, i, i, i, i, i, C.POINTER(ll), C.c_char_p, i]
        L.abh_route_pedigree.argtypes = [i, i, i, i, i, C.POINTER(ll)]
        self.L, self.p8, self.p15, self.err = L, (ll * 8)(), (ll * 15)(), C.create_string_buffer(128)

    def lanes(self, ped):
        self.L.abh_route_pedigree(*ped, self.p8)
        return int(self.p8[0])

    def old(self, ped, lanes, chains, queue=0, parking=0, pass_=0):
        st = self.L.abh_route_launch(*ped, 0, lanes, chains, CUS, queue, parking, pass_, self.p15, self.err, 128)
        return st, self.err.value, dict(zip(NAMES, map(int, self.p15)))

    def new(self, ped, lanes, chains, sweep, queue=0, parking=0, pass_=0):
        st = self.L.abh_route_launch_sweep(*ped, 0, lanes, chains, CUS, queue, parking, pass_, sweep, self.p15, self.err, 128)
        return st, self.err.value, dict(zip(NAMES, map(int, self.p15)))


@pytest.fixture(scope="module")
def shim():
    return Shim()


def _ped(gens, requested=0, strict=0):
    tmax, k, _ = RM.topology(gens)
    return (int(np.asarray(gens).shape[0]), k, tmax, requested, strict)


def _streamed_cases():
    from alphabeta_rs_amd import synthetic

    c5, _ = synthetic.c5_pedigree()
    n, tmax, k, _, kind = RM.boundary_cases()["auto64_rmax16_rows_over"]      # one row past the residency limit at 64 lanes
    assert kind == "stream"
    return {"c5": _ped(c5[:, :3]), "boundary": _ped(RM.boundary_pedigree(n, tmax, k)[:, :3]),
            "n1100": _ped(synthetic_pedigree(np.random.default_rng(5), 1100, 12)[:, :3])}


def test_sweep_offer_routes_streamed_launches_to_the_sweep_kernel(shim):
    cases = _streamed_cases()
    assert cases["c5"][:3] == (20100, 950, 125) and cases["boundary"][:3] == (1025, 1024, 127) and cases["n1100"][0] == 1100
    for name, ped in cases.items():
        n, k, tmax = ped[:3]
        lanes = shim.lanes(ped)
        assert lanes == RM.WAVE, name
        # by hand: the power table, THREE dt tables of K rounded up to even, four constants
        stride = RM.KPW * (tmax + 1) + 3 * ((k + 1) & ~1) + 4
        assert stride == RM.chain_stride(tmax, k) + 2 * ((k + 1) & ~1)
        for chains in (1, 7, 100000):
            for queue, parking in ((0, 0), (1, 0), (1, 1)):
                st, err, r = shim.new(ped, lanes, chains, 1, queue, parking)
                assert st == 0, (name, err)
                assert (r["kind"], r["family"], r["G"]) == (KERNEL_STREAM_SWEEP, FAM_SWEEP, RM.WAVE), (name, r)
                assert r["R"] == (0 if n >= SWEEP_DEEP_ROWS else -1), (name, r)
                assert (r["tp"], r["strict"], r["resume"], r["quantum"], r["tail_cap"]) == (0, 0, 0, 0, 0), (name, r)
                assert (r["chain_stride"], r["lds"]) == (stride, 8 * stride), (name, r)
                assert r["lds"] <= RM.MAX_DYN_LDS
                assert (r["grid"], r["block"], r["tree"]) == (chains, RM.WAVE, RM.WAVE), (name, r)
                assert shim.old(ped, lanes, chains, queue, parking)[2]["kind"] == KERNEL_STREAM      # what it replaces
    assert cases["c5"][:3] == (20100, 950, 125)
    assert shim.new(cases["c5"], 64, 10, 1)[2]["lds"] == 8 * (1260 + 3 * 950 + 4) == 32912   # four workgroups per CU
    assert shim.new(cases["c5"], 64, 10, 1)[2]["R"] == 0 and shim.new(cases["n1100"], 64, 10, 1)[2]["R"] == -1


def test_sweep_offer_changes_no_other_route(shim):
    """a resident pedigree, strict order, fewer than 64 lanes, a two-pass offer, a footprint beyond the CU's LDS: today's
    route, field for field"""
    from alphabeta_rs_amd import synthetic

    c3, _ = synthetic.c3_pedigree()
    big = synthetic_pedigree(np.random.default_rng(5), 1100, 12)[:, :3]
    kmax = RM.limit_k()                       # the largest plan there is: its scratch fits 160 KiB, three dt tables do not
    cases = [("resident", _ped(c3[:, :3], 0, RM.strict_of(c3.shape[0], {})), None, 0),
             ("resident_tree", _ped(c3[:, :3], 0, 0), None, 0),
             ("resident64", _ped(c3[:, :3], 0, 0), 64, 0),
             ("strict", _ped(big, 0, 1), None, 0),
             ("lanes16", _ped(big, 16, 0), None, 0),
             ("two_pass_1", _ped(big), None, 1),
             ("two_pass_2", _ped(big), None, 2),
             ("too_large", (kmax + 1, kmax, 127, 0, 0), None, 0)]
    for name, ped, lanes, pass_ in cases:
        lanes = lanes or shim.lanes(ped)
        for chains in (1, 5000):
            want = shim.old(ped, lanes, chains, 1, 0, pass_)
            got = shim.new(ped, lanes, chains, 1, 1, 0, pass_)
            assert got == want, (name, got, want)
            assert want[0] == 0 and want[2]["kind"] != KERNEL_STREAM_SWEEP and want[2]["family"] != FAM_SWEEP, (name, want)
    assert shim.old(cases[-1][1], 64, 1)[2]["kind"] == KERNEL_STREAM
    assert shim.old(cases[3][1], 64, 1)[2]["strict"] == 1 and shim.old(cases[4][1], 16, 1)[2]["G"] == 16


def test_without_the_offer_every_answer_is_the_old_entrys(shim):
    from alphabeta_rs_amd import synthetic

    c3, _ = synthetic.c3_pedigree()
    peds = list(_streamed_cases().values()) + [_ped(c3[:, :3])]
    peds += [(n, min(n, 600), 127, req, strict) for n in (6, 105, 351, 700, 1024, 1025, 3071, 3072, 5000)
             for req in (0, 16, 64) for strict in (0, 1)]
    asked = 0
    for ped in peds:
        lanes = shim.lanes(ped)
        for ph_lanes in {lanes, RM.WAVE}:
            for chains in (0, 1, 3000, 30000):
                for queue, parking, pass_ in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 2)):
                    assert shim.new(ped, ph_lanes, chains, 0, queue, parking, pass_) == \
                        shim.old(ped, ph_lanes, chains, queue, parking, pass_), (ped, ph_lanes, chains, queue, parking, pass_)
                    asked += 1
    assert asked > 1000


def test_code_object_has_the_two_sweep_kernels_without_scratch():
    isa = _device_isa.device_isa()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", isa, re.M)
    sweep = sorted(n for n in names if "abn_sweep_kernel" in n)
    assert sweep == ["_ZN3abn16abn_sweep_kernelILi0EEEvNS_7FitArgsE", "_ZN3abn16abn_sweep_kernelILin1EEEvNS_7FitArgsE"], sweep
    families = ("abn_fit_kernel", "abn_fit_refill_kernel", "abn_fit_spec_kernel", "abn_cost_kernel")
    assert sum(any(f in n for f in families) for n in names) == 103            # the pinned census, untouched
    assert not any(any(f in n for f in families) for n in sweep)
    meta = isa[isa.index("amdhsa.kernels:"):]
    for name in sweep:                      # the kernel's record of the code object's metadata
        rec = [r for r in re.split(r"\n  - ", meta) if re.search(r"\.name:\s+" + re.escape(name) + r"\s", r)]
        assert len(rec) == 1, name
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec[0])
        assert priv and int(priv.group(1)) == 0, (name, priv and priv.group(0))
        assert int(re.search(r"\.wavefront_size:\s+(\d+)", rec[0]).group(1)) == 64
