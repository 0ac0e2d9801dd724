"""Census of the compiled fit-path instantiations (CPU tier: the gfx950 assembly cross-compiles without a GPU).

abn_api.hip's C-ABI dispatches to 103 template instantiations of abn_fit_kernel, abn_fit_refill_kernel,
abn_fit_spec_kernel and abn_cost_kernel.  Each one must be in exactly one of tests/_kernel_matrix.py's tables: MATRIX
(a GPU case of tests/test_gpu_kernel_matrix.py whose inputs route to it) or UNREACHABLE (with the host condition that
rules it out).  A new instantiation — a new `case` of a dispatch switch, a new template argument — fails here until it
gets a case or a reason; a table entry the assembly no longer has fails too.
"""
import re

import pytest

import _device_isa
import _kernel_matrix as KM
import _route_model as RM

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
        assert "abn_route.hpp" in why and "route_launch" in why, (KM.label(k), why)   # a pointer to the host condition


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
    tmax, k, _ = RM.topology(ped)
    assert (ped.shape[0], tmax, k) == (c["n"], c["tmax"], c["k"])
    o = abn.default_options(**c["opts"])
    assert abn.reduction_tree(ped[:, :3], o) == RM.expected_tree(c["n"], c["tmax"], c["k"], c["opts"])
    assert key in KM.targets(c), [KM.label(t) for t in KM.targets(c)]


# ------------------------------------------------------------------------------------------------ the C++ routing, on the CPU
# csrc/abn_route.hpp decides every launch in three pure functions; host/host_capi.cpp exports them (abh_route_*).  Below
# they are asked what they would launch and held against the independent restatement of the policy in
# tests/_route_model.py (and tests/_kernel_matrix.py's routes over it) — which stays a restatement: nothing here feeds the
# shim's answers back in.
CUS = 256
SMALL_WAVES, BIG_WAVES = 8 * CUS, 12 * CUS      # persistent launches: wavefronts of the small / the full geometry
FAMILY = (KM.FIT, KM.REFILL, KM.SPEC, KM.COST)
LDS_REFUSAL = b"pedigree needs more LDS per workgroup than supported (T or K too large)"


class Route:
    def __init__(self):
        import ctypes as C

        from alphabeta_rs_amd import build as B

        B.build_host()
        L = C.CDLL(str(B.PEDIGREE_LIB))
        i, ll = C.c_int, C.c_longlong
        L.abh_route_pedigree.argtypes = [i, i, i, i, i, C.POINTER(ll)]
        L.abh_route_phase.argtypes = [i, i, i, i, i, i, ll, i, i, i, i, C.POINTER(i)]
        L.abh_route_launch.argtypes = [i, i, i, i, i, i, i, ll, i, i, i, i, C.POINTER(ll), C.c_char_p, i]
        self.L, self.p8, self.p3, self.p15, self.err = L, (ll * 8)(), (i * 3)(), (ll * 15)(), C.create_string_buffer(128)

    def pedigree(self, ped):
        """ped = (n, k, tmax, requested lanes, strict) -> the pedigree level's answers"""
        refused = self.L.abh_route_pedigree(*ped, self.p8)
        names = ("lanes", "tree", "reported_tree", "streams", "wide_ok", "spec_ok", "cost_lanes", "select_lds")
        return dict(zip(names, self.p8), refused=bool(refused))

    def phase(self, ped, phase, plan_chains, dmode, whole=True, two_pass=False):
        self.L.abh_route_phase(*ped, phase, plan_chains, CUS, dmode, whole, two_pass, self.p3)
        return tuple(self.p3)   # spec, lanes, two passes

    def launch(self, ped, spec, lanes, chains, queue=False, parking=False, pass_=0):
        """(status, error text, kind, keys): the launch's key, and its tail's resume launch's if there is one"""
        status = self.L.abh_route_launch(*ped, spec, lanes, chains, CUS, queue, parking, pass_, self.p15, self.err, 128)
        v = self.p15
        keys = []
        if status == 0 and v[0] != 0:
            keys.append((FAMILY[v[1]], v[2], v[3], bool(v[4]), bool(v[5]), bool(v[6])))
            if v[13] > 0:
                keys.append((KM.SPEC, RM.WAVE, v[14], False, False, True))
        return status, self.err.value, v[0], keys

    def phase_keys(self, ped, phase, chains, dmode, whole=True, two_pass=False, parking=False):
        """every key the launches of one phase of a plan take (both passes of a two-pass phase A, a tail's resume launch)"""
        spec, lanes, two = self.phase(ped, phase, chains, dmode, whole, two_pass)
        out = []
        for pass_ in ((1, 2) if two else (0,)):
            status, err, _, keys = self.launch(ped, spec, lanes, chains, queue=whole, parking=parking, pass_=pass_)
            assert status == 0, (ped, phase, chains, err)
            out += keys
        return out


@pytest.fixture(scope="module")
def route():
    return Route()


def _plan_inputs(c):
    """what a plan over a MATRIX case's pedigree passes down, by the restatements: (ped, S, B, two-pass, parking, dmode of B)"""
    n, tmax, k, o = c["n"], c["tmax"], c["k"], c["opts"]
    req, strict = o.get("lanes_per_chain", 0), RM.strict_of(n, o)
    cs = RM.chain_stride(tmax, k)
    lanes = RM.pick_lanes(n, req, cs)
    S, B = c["S"], KM.boot_count(c, SMALL_WAVES, CUS)
    two_pass = (S > RM.TWO_PASS_CHAINS and o.get("max_iters_start", 10000) > RM.PHASE_A_CAP and
                bool(o.get("no_fixed_point_skip", 0)) and not o.get("shrink_on_failed_contraction", 0) and not strict)
    parking = lanes < RM.WAVE and max(S, B) > SMALL_WAVES * (RM.WAVE // lanes)     # abn_plan_create: time slicing buffers
    dmode_b = 2 if RM.streams(n, k, cs, lanes, strict) and not o.get("stream_mode", 0) else 1
    return (n, k, tmax, req, strict), S, B, two_pass, parking, dmode_b


@pytest.mark.parametrize("key", list(KM.MATRIX), ids=KM.label)
def test_cpp_routes_case_to_its_instantiation(route, key):
    """what the C++ routes for the case's launches (256 CUs, the chain counts of tests/test_gpu_kernel_matrix.py) contains
    the case's own key and nothing the restated dispatch does not expect; the pedigree level reports the restated tree"""
    c = KM.MATRIX[key]
    o = c["opts"]
    if c["route"] == "cost":
        ped = (c["n"], c["k"], c["tmax"], o.get("lanes_per_chain", 0), RM.strict_of(c["n"], o))
        got = {(KM.COST, route.pedigree(ped)["cost_lanes"], 0, False, False, False)}
    else:
        ped, S, B, two_pass, parking, dmode_b = _plan_inputs(c)
        got = set(route.phase_keys(ped, 0, S, 0, two_pass=two_pass, parking=parking))
        got |= set(route.phase_keys(ped, 1, B, dmode_b, two_pass=two_pass, parking=parking))
    assert key in got, [KM.label(k) for k in got]
    assert got <= KM.targets(c), [KM.label(k) for k in got - KM.targets(c)]
    assert route.pedigree(ped)["reported_tree"] == RM.expected_tree(c["n"], c["tmax"], c["k"], o)
    strict_cost = (c["n"], c["k"], c["tmax"], o.get("lanes_per_chain", 0), 1)
    assert route.pedigree(strict_cost)["cost_lanes"] == RM.WAVE       # abn_cost_batch in strict order: a wavefront per candidate


def test_cpp_routing_at_the_lds_boundaries(route):
    """tests/test_gpu_lds_boundary.py's pairs: resident or streamed as filed, the speculative kernel one step either side of
    its footprint, and abn_plan_create's refusal one step over limit_k() with acceptance at it"""
    for name, (n, tmax, k, o, kind) in RM.boundary_cases().items():
        p = route.pedigree((n, k, tmax, o.get("lanes_per_chain", 0), o.get("strict_order", 0)))
        assert not p["refused"], name
        assert bool(p["streams"]) == (kind == "stream"), name
        assert p["reported_tree"] == RM.expected_tree(n, tmax, k, o), name
        if name.startswith("spec_"):
            assert bool(p["spec_ok"]) == (name == "spec_under"), name
    kmax = RM.limit_k()
    assert not route.pedigree((kmax + 1, kmax, 127, 0, 0))["refused"]
    assert route.pedigree((kmax + 3, kmax + 2, 127, 0, 0))["refused"]


def test_cpp_routing_sweep_stays_inside_the_census(route, kernels):
    """The launch level over a grid of pedigrees, options, chain counts either side of every threshold (256 CUs), both
    phases, with and without the caller's queue and parking buffers: never an UNREACHABLE key, never a key the assembly
    does not hold, and every MATRIX fit-path key at least once.  Pedigrees no plan accepts are refused with the one text."""
    peds = []
    for n in list(range(1, 1101)) + [1500, 2048, 3073, 5000, 20100]:
        for tmax, k in ((127, min(n, 600)), (3, min(n, 40))):
            peds += [(n, k, tmax, req, strict) for req in (0, 8, 16, 32, 64) for strict in (0, 1)]
    own = {}                                      # the MATRIX cases' own inputs: no key depends on the grid's luck
    for c in KM.MATRIX.values():
        if c["route"] != "cost":
            ped, S, B, *_ = _plan_inputs(c)
            own.setdefault(ped, set()).update((S, B))
    hits = set()
    for ped in peds + list(own):
        n = ped[0]
        p = route.pedigree(ped)
        if p["refused"]:      # abn_plan_create refuses; abn_fit_batch reaches the launch level, which refuses the same way
            status, err, _, _ = route.launch(ped, 0, p["lanes"], 1)
            assert (status, err) == (RM.ERR_INVALID_ARG, LDS_REFUSAL), ped
            continue
        ng = RM.WAVE // p["lanes"]
        small = RM.pick_rmax(n, RM.WAVE) <= 2
        edges = ({1, RM.TWO_PASS_CHAINS, 24 * CUS, SMALL_WAVES * ng, BIG_WAVES * ng, CUS * (16 if small else 8)},
                 {1, (3 * CUS // 4) * p["lanes"], SMALL_WAVES * ng, BIG_WAVES * ng, CUS * 6 if small else CUS * 3})
        for phase in (0, 1):
            for chains in sorted({x + d for x in edges[phase] | own.get(ped, set()) for d in (0, 1)}):
                for dmode in ((0,) if phase == 0 else (1, 2) if p["streams"] else (1,)):
                    for whole in (False, True):           # a window group is offered neither queue nor parking buffers
                        two = phase == 0 and whole and chains > RM.TWO_PASS_CHAINS and not ped[4]
                        for two_pass in ((False, True) if two else (False,)):
                            for parking in ((False, True) if whole and ng > 1 and chains > SMALL_WAVES * ng else (False,)):
                                hits.update(route.phase_keys(ped, phase, chains, dmode, whole, two_pass, parking))
    assert not hits & set(KM.UNREACHABLE), [KM.label(k) for k in hits & set(KM.UNREACHABLE)]
    assert hits <= set(kernels), [KM.label(k) for k in hits - set(kernels)]
    missing = {k for k in KM.MATRIX if k[0] != KM.COST} - hits
    assert not missing, [KM.label(k) for k in sorted(missing, key=str)]
