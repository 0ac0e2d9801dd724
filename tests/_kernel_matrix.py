"""The fit-path kernel matrix: every compiled instantiation of abn_fit_kernel, abn_fit_refill_kernel, abn_fit_spec_kernel
and abn_cost_kernel (the kernel table of abn_api.hip), each either in MATRIX — one deterministic case whose inputs route
to it — or in UNREACHABLE with the host condition that keeps it from launching.

Plain data and host arithmetic, no device: tests/test_kernel_matrix_census.py checks on the CPU that the two tables
partition what the gfx950 assembly holds and that every case's pedigree has the tree the case expects;
tests/test_gpu_kernel_matrix.py runs the cases on the MI355X against the oracle.

A key is (family, G, R, TP, STRICT, RESUME): G lanes per chain (64 for the speculative kernel), R rows per lane (0: deep
stream loop, -1: pair-loop stream; the speculative kernel's RMAX), TP two-pass, STRICT serial row order, RESUME the
speculative kernel's tail hand-over.  Fields a family has no template argument for are False (cost: R = 0).

The host arithmetic is the restatement in tests/_route_model.py (topology, footprints, pick_rmax, pick_lanes).
"""
import re

from _route_model import (DEEP_ROWS, MAX_DYN_LDS, SERIAL_SUM_MAX_ROWS, TWO_PASS_CHAINS, WAVE, boundary_pedigree,
                          chain_stride, fit_rmax, pick_lanes, pick_rmax, pool_size, spec_fits, streams, strict_of)

FIT, REFILL, SPEC, COST = "fit", "refill", "spec", "cost"


# ------------------------------------------------------------------------------------------------ names
def decode(name):
    """(family, G, R, TP, STRICT, RESUME) of a mangled kernel name, or None for any other kernel (Itanium mangling:
    `Li16E` is the int 16, `Lin1E` the int -1, `Lb1E` true)."""
    i, b = r"Li(n?)(\d+)E", r"Lb([01])E"

    def num(sign, digits):
        return -int(digits) if sign else int(digits)

    m = re.fullmatch(rf"_ZN3abn14abn_fit_kernelI{i}{i}{b}{b}EEvNS_7FitArgsE", name)
    if m:
        return (FIT, num(*m.group(1, 2)), num(*m.group(3, 4)), m.group(5) == "1", m.group(6) == "1", False)
    m = re.fullmatch(rf"_ZN3abn21abn_fit_refill_kernelI{i}{i}EEvNS_7FitArgsE", name)
    if m:
        return (REFILL, num(*m.group(1, 2)), num(*m.group(3, 4)), False, False, False)
    m = re.fullmatch(rf"_ZN3abn19abn_fit_spec_kernelI{i}{b}{b}EEvNS_7FitArgsE", name)
    if m:
        return (SPEC, WAVE, num(*m.group(1, 2)), False, m.group(3) == "1", m.group(4) == "1")
    m = re.fullmatch(rf"_ZN3abn15abn_cost_kernelI{i}EEvNS_8CostArgsE", name)
    if m:
        return (COST, num(*m.group(1, 2)), 0, False, False, False)
    return None


def label(key):
    fam, g, r, tp, strict, resume = key
    if fam == COST:
        return f"cost<{g}>"
    if fam == SPEC:
        return f"spec<{r},{'strict' if strict else 'tree'}{',resume' if resume else ''}>"
    if fam == REFILL:
        return f"refill<{g},{r}>"
    return f"fit<{g},{r}{',tp' if tp else ''}{',strict' if strict else ''}>"


# ------------------------------------------------------------------------------------------------ the routes
def targets(case):
    """the instantiations a case's route launches by this restatement (the case's own key must be among them)"""
    n, tmax, k, o = case["n"], case["tmax"], case["k"], case["opts"]
    cs = chain_stride(tmax, k)
    strict = strict_of(n, o)
    lanes = pick_lanes(n, o.get("lanes_per_chain", 0), cs)
    route = case["route"]
    if route == "cost":
        return {(COST, WAVE if strict else lanes, 0, False, False, False)}
    r = fit_rmax(n, k, tmax, lanes, strict)
    plain = (FIT, WAVE if r == 16 else lanes, r, False, bool(strict), False)
    if route == "plan":
        return {plain}
    if route == "twopass":
        return {plain, (FIT, plain[1], r, True, False, False)}
    if route == "persistent":
        return {plain, (REFILL, lanes, r, False, False, False)}
    rs = pick_rmax(n, WAVE)
    if route == "spec":
        return {(SPEC, WAVE, rs, False, bool(strict), False)} if spec_fits(n, tmax, k, strict) else set()
    if route == "tail":
        return {(SPEC, WAVE, rs, False, False, False), (REFILL, lanes, r, False, False, False),
                (SPEC, WAVE, rs, False, False, True), plain}
    raise ValueError(route)


# ------------------------------------------------------------------------------------------------ the cases
def _rows(g, r, full):
    """N at a step of the rows-per-lane ladder: G r (every lane group full) or one row past the step below (the last lane
    group ragged: the (gl + G q) < N masks); streams: the largest pair-loop / the first deep-loop pedigree, or one row
    past the last resident one / the deep threshold"""
    if r >= 1:
        return g * r if full else (g * (r // 2) + 1 if r > 1 else 3)
    if r == -1:
        return DEEP_ROWS * g - 1 if full else (8 * g + 1 if g < WAVE else 16 * WAVE + 1)
    return DEEP_ROWS * g + (0 if full else 1)


_T_ORDER = (0, 1, 2, 3, 127, 126, 33, 64, 7, 12, 96, 5, 20, 45)


def _shape(n, g, r, strict, index, want_stream, t_first=None):
    """(tmax, k) for N rows at G lanes: T from a rotation over small (0..3), odd and even large values, the first that
    keeps the route (resident or streamed as wanted, within the stream variant's LDS); K odd or even by `index`"""
    order = _T_ORDER[index % len(_T_ORDER):] + _T_ORDER[:index % len(_T_ORDER)]
    if t_first is not None:
        order = (t_first,) + order
    for tmax in order:
        k = min(n, pool_size(tmax), 600)
        if k > 1 and (k % 2) != (index % 2):
            k -= 1
        cs = chain_stride(tmax, k)
        if streams(n, k, cs, g, strict) != want_stream:
            if want_stream:
                continue
            # resident wanted: fewer distinct triples may fit
            while k > 2 and streams(n, k, cs, g, strict):
                k -= 2
                cs = chain_stride(tmax, k)
            if streams(n, k, cs, g, strict):
                continue
        stride = cs + (8 * g if strict and want_stream else 0)   # the strict stream variant's chunk of terms
        if want_stream and (WAVE // g) * stride * 8 > (MAX_DYN_LDS if g == WAVE else 64 * 1024):
            continue
        return tmax, k
    raise AssertionError(f"no shape for N={n} G={g} R={r}")


def _fit_case(g, r, tp, strict, index):
    full = ((g in (8, 32)) != tp) != strict
    n = _rows(g, r, full)
    tmax, k = _shape(n, g, r, strict, index, r <= 0, t_first=None if not tp else (1 if g == 8 else 3))
    o = {"lanes_per_chain": g, "strict_order": 1 if strict else -1, "max_iters_start": 20, "max_iters_boot": 15}
    if r <= 0:
        o["stream_mode"] = index % 2        # 0: bootstrap observations materialised, 1: gathered through the index row
    c = {"route": "plan", "n": n, "tmax": tmax, "k": k, "opts": o, "W": 1, "S": 5, "B": 7, "seed": 100 + index}
    if tp:   # > 4096 start chains, 4099 not a multiple of 64/G; the first pass parks what runs past 1000 iterations
        o.update(max_iters_start=1200, no_fixed_point_skip=1)
        c.update(route="twopass", S=TWO_PASS_CHAINS + 3, B=3)
    return c


def _build():
    m = {}
    index = 0
    for g in (8, 16, 32, 64):
        for tp, strict in ((False, False), (False, True), (True, False)):
            for r in (1, 2, 4, 8, 16, -1, 0):
                if (r == 16 and g != WAVE) or (r == -1 and strict):
                    continue
                m[(FIT, g, r, tp, strict, False)] = _fit_case(g, r, tp, strict, index)
                index += 1
    # persistent: more lane groups than 2048 wavefronts (persist_waves_small on 256 CUs) hold, explicit lanes (no tail)
    for g in (8, 16, 32):
        for r in (1, 2, 4, 8):
            n = _rows(g, r, (g + r) % 3 != 0)
            tmax, k = _shape(n, g, r, 0, index, False)
            o = {"lanes_per_chain": g, "strict_order": -1, "max_iters_start": 20, "max_iters_boot": 30}
            m[(REFILL, g, r, False, False, False)] = {
                "route": "persistent", "n": n, "tmax": tmax, "k": k, "opts": o, "W": 1, "S": 3,
                "B": "persistent+37", "seed": 100 + index}
            index += 1
    # speculative (few chains, auto lanes): phase A and phase B both on it
    spec = {  # R: (N, T, K) tree        strict
        (1, False): (64, 3, 63), (2, False): (65, 2, 26), (4, False): (256, 100, 101), (8, False): (257, 63, 200),
        (1, True): (16, 1, 7), (2, True): (128, 31, 100), (4, True): (129, 3, 63), (8, True): (300, 50, 201),
    }
    for (r, strict), (n, tmax, k) in spec.items():
        o = {"strict_order": (0 if n <= SERIAL_SUM_MAX_ROWS else 1) if strict else -1, "max_iters_start": 20,
             "max_iters_boot": 15}
        m[(SPEC, WAVE, r, False, strict, False)] = {"route": "spec", "n": n, "tmax": tmax, "k": k, "opts": o, "W": 1,
                                                    "S": 5, "B": 7, "seed": 100 + index}
        index += 1
    # tail hand-over: auto lanes (canonical tree), persistent phase B, bootstrap fits long enough to be parked
    for r, (n, tmax, k) in {1: (32, 12, 31), 2: (65, 40, 64), 4: (200, 90, 150)}.items():
        o = {"strict_order": -1, "max_iters_start": 20, "max_iters_boot": 1000}
        m[(SPEC, WAVE, r, False, False, True)] = {"route": "tail", "n": n, "tmax": tmax, "k": k, "opts": o, "W": 1,
                                                   "S": 3, "B": "persistent+37", "seed": 100 + index}
        index += 1
    # cost batch: explicit lanes; a streamed pedigree at 16 and 64 lanes (its cost tree is the lane count)
    for g, (n, tmax, k) in {8: (20, 5, 19), 16: (130, 9, 120), 32: (97, 126, 96), 64: (1025, 127, 601)}.items():
        m[(COST, g, 0, False, False, False)] = {"route": "cost", "n": n, "tmax": tmax, "k": k,
                                                "opts": {"lanes_per_chain": g}, "seed": 100 + index}
        index += 1
    return m


MATRIX = _build()

# instantiations the dispatch compiles but cannot launch, with the condition in abn_route.hpp that rules them out
_NO_REFILL_64 = ("route_launch (abn_route.hpp): a persistent launch needs several chains per wavefront (persistent_by_size: "
                 "kWave / lanes > 1), so never 64 lanes; abn_api.hip's kernel table lists refill<64, R> all the same")
UNREACHABLE = {
    (REFILL, 64, 1, False, False, False): _NO_REFILL_64,
    (REFILL, 64, 2, False, False, False): _NO_REFILL_64,
    (REFILL, 64, 4, False, False, False): _NO_REFILL_64,
    (REFILL, 64, 8, False, False, False): _NO_REFILL_64,
    (SPEC, 64, 8, False, False, True): (
        "route_launch (abn_route.hpp): the tail hand-over needs a persistent launch (lanes < 64) and the canonical tree "
        "(tail_cap_for: auto lanes); auto lanes below 64 means N <= 256 (pick_lanes), so pick_rmax(N, kWave) <= 4 and "
        "route_tail_resume never takes RMAX 8"),
}


def boot_count(case, small_waves, cus):
    """B of a case: 'persistent+37' is 37 chains past what the persistent launch needs at the case's lanes, so that the
    last wavefront is partly filled: more lane groups than persist_waves_small wavefronts hold, and with auto lanes more
    bootstraps than route_phase gives a wavefront each (3 cus / 4 x lanes: 6144 at 32 lanes on 256 CUs)"""
    b = case["B"]
    if isinstance(b, int):
        return b
    auto = not case["opts"].get("lanes_per_chain", 0)
    lanes = pick_lanes(case["n"], case["opts"].get("lanes_per_chain", 0), chain_stride(case["tmax"], case["k"]))
    return max(small_waves * (WAVE // lanes), (3 * cus // 4) * lanes if auto else 0) + 37


def pedigree(case):
    return boundary_pedigree(case["n"], case["tmax"], case["k"], seed=case["seed"])
