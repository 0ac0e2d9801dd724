"""abn_sim_*: methylomes simulated down a pedigree under the ABneutral model (src/divergence.rs:33-114 run forwards), as
functions on a Context.

A tree of V nodes — parent[0] = -1, parent[v] < v — with thresholds thr (V, 3, 2) uint64 and emit (V,) flags; the r-th
emitted node is row r of a 2-bit packed matrix, the format Context.pairwise_divergence_packed scans.  The law is written
in csrc/abn_sim.hpp and include/abneutral.h.  A module of its own, imported by its name:

    from alphabeta_rs_amd import simulate
    thr = simulate.thresholds(parent, generation, 2e-3, 5e-3, 0.7, 0.3)
    rows, p0uu = simulate.pedigree(ctx, 1, parent, generation, emit, 2e-3, 5e-3, 0.7, 0.3, 400_000)
    model, *_ = ctx.ab_neutral_run(rows, p0uu, p0uu, 1.0, 100)

The observation step turns true states into called ones — a miscall, or 3 = filtered — and a replicate study runs R
pedigrees as the column ranges of one simulation:

    othr = simulate.obs_thresholds(miscall, dropout)
    times, D, p0uu, census = simulate.study(ctx, 1, parent, generation, emit, 2e-3, 5e-3, 0.7, 0.3, 100_000, 50,
                                            miscall=miscall, dropout=dropout)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import AbnError, _arr, _dev, _ptr, load_host_library, load_library
from .context import packed_row_stride

MAX_NODES = 65535       # kSimMaxNodes: what the pairwise scan takes as samples
MAX_SITES = 1 << 34     # counter word c0 holds k >> 2


def _tree(parent, *per_node):
    """parent int32 (V,) and every other per-node array checked against V"""
    parent = _arr(parent, np.int32, -1)
    for a in per_node:
        if a.shape[0] != parent.shape[0]:
            raise ValueError("parent, generation, thr and emit describe one set of nodes")
    return parent


def _thr(thr):
    thr = _arr(thr, np.uint64)
    if thr.ndim != 3 or thr.shape[1:] != (3, 2):
        raise ValueError("thr is (nodes, 3, 2) uint64")
    return thr


def thresholds(parent, generation, alpha, beta, p_uu0, weight) -> np.ndarray:
    """thr (V, 3, 2) uint64 from rates (abn_sim_thresholds; host arithmetic, no device): for v > 0 the rows of
    genmatrix(alpha, beta) to the power generation[v] - generation[parent[v]], for the founder the row
    [p_uu0, w (1 - p_uu0), (1 - w)(1 - p_uu0)] . G^generation[0]; a cumulative probability c becomes 0 (c <= 0), 2^64 - 1
    (c >= 1) or int(ldexp(c, 64)).  AbnError: a generation outside 0..127, a child older than its parent, a rate outside
    [0, 1]."""
    generation = _arr(generation, np.int32, -1)
    parent = _tree(parent, generation)
    thr = np.zeros((parent.shape[0], 3, 2), dtype=np.uint64)
    text = C.create_string_buffer(256)
    rc = load_library().abn_sim_thresholds(float(alpha), float(beta), float(p_uu0), float(weight), parent.shape[0], _ptr(parent),
                                           _ptr(generation), _ptr(thr), text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return thr


def _arguments(parent, thr, emit):
    thr, emit = _thr(thr), _arr(emit, np.uint8, -1)
    return _tree(parent, thr, emit), thr, emit


def _packed(emit, n_sites, row_stride):
    stride = packed_row_stride(n_sites) if row_stride is None else int(row_stride)
    return np.zeros((int(np.count_nonzero(emit)), stride), dtype=np.uint8)


def codes(ctx, seed, parent, thr, emit, n_sites, row_stride=None) -> np.ndarray:
    """The simulated methylomes of the emitted nodes on the device (abn_sim_codes): packed uint8 (emitted, row_stride),
    row_stride = packed_row_stride(n_sites) unless given.  AbnError: what the law refuses (abn_last_error names it)."""
    parent, thr, emit = _arguments(parent, thr, emit)
    out = _packed(emit, n_sites, row_stride)
    ctx._check(ctx._L.abn_sim_codes(ctx._h, int(seed), parent.shape[0], _ptr(parent), _ptr(thr), _ptr(emit), int(n_sites),
                                    _ptr(out), out.shape[1]))
    return out


def codes_dev(ctx, seed, parent, thr, emit, n_sites, out_ptr: int, row_stride: int) -> float:
    """The same into a device matrix [emitted x row_stride] at out_ptr (16-byte aligned), what
    Context.pairwise_divergence_packed_dev reads; nothing reaches the host.  Returns the kernel's HIP-event ms."""
    parent, thr, emit = _arguments(parent, thr, emit)
    return ctx._timed(ctx._L.abn_sim_codes_dev, int(seed), parent.shape[0], _ptr(parent), _ptr(thr), _ptr(emit), int(n_sites),
                      _dev(out_ptr), int(row_stride))


def codes_host(seed, parent, thr, emit, n_sites, row_stride=None) -> np.ndarray:
    """codes in its serial host form (abn_sim_codes_host): no device needed; the same bytes and the same refusals"""
    parent, thr, emit = _arguments(parent, thr, emit)
    out = _packed(emit, n_sites, row_stride)
    H = load_host_library()
    H.abn_sim_codes_host.argtypes = [C.c_uint64, C.c_int] + [C.c_void_p] * 3 + [C.c_longlong, C.c_void_p, C.c_longlong,
                                                                                  C.c_char_p, C.c_int]
    text = C.create_string_buffer(256)
    rc = H.abn_sim_codes_host(int(seed), parent.shape[0], parent.ctypes.data, thr.ctypes.data, emit.ctypes.data, int(n_sites),
                              out.ctypes.data, out.shape[1], text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return out


def launch_grid(ctx, n_sites):
    """(workgroups, lanes per workgroup) of the launch codes makes for n_sites sites (abn_sim_grid): a lane owns one dword
    of a row — 16 sites — per trip of its grid stride"""
    grid = np.zeros(2, dtype=np.int32)
    ctx._check(ctx._L.abn_sim_grid(ctx._h, int(n_sites), _ptr(grid)))
    return int(grid[0]), int(grid[1])


def pedigree(ctx, seed, parent, generation, emit, alpha, beta, p_uu0, weight, n_sites, with_ms=False):
    """Pedigree::build (src/pedigree.rs:92-193) of simulated methylomes (abn_sim_pedigree): the simulation on the device, the
    packed pairwise scan on the matrix where it lies, and (rows (pairs, 4) = [t0, t1, t2, D] per pair i < j of the emitted
    nodes in node order, p0uu) — what Context.ab_neutral_run takes.  t0 is the generation of the pair's last common
    ancestor; p0uu the mean over the samples of 1 - (n1 + 2 n2) / (2 n_sites).  with_ms: also the HIP-event ms of the
    simulation and of the two passes over the matrix behind it (divergence scan and transition table, summed)."""
    thr = thresholds(parent, generation, alpha, beta, p_uu0, weight)
    generation = _arr(generation, np.int32, -1)
    parent, thr, emit = _arguments(parent, thr, emit)
    n = int(np.count_nonzero(emit))
    rows, p0uu, ms = np.zeros((max(n * (n - 1) // 2, 1), 4)), C.c_double(0.0), np.zeros(2)
    ctx._check(ctx._L.abn_sim_pedigree(ctx._h, int(seed), parent.shape[0], _ptr(parent), _ptr(generation), _ptr(thr), _ptr(emit),
                                       int(n_sites), _ptr(rows), C.byref(p0uu), _ptr(ms)))
    return (rows, p0uu.value, ms) if with_ms else (rows, p0uu.value)


# ---------------------------------------------------------------------------------------------- the observation step
def _othr(othr):
    othr = _arr(othr, np.uint64)
    if othr.shape != (3, 3):
        raise ValueError("othr is (3, 3) uint64")
    return othr


def obs_thresholds(miscall, dropout) -> np.ndarray:
    """othr (3, 3) uint64 of the observation law (abn_sim_obs_thresholds; host arithmetic): miscall (3, 3), row s the
    probabilities that a kept call of a true state s reads 0, 1, 2; dropout (3,), the probability that a call of a true
    state s is filtered.  AbnError: a value outside [0, 1], a miscall row that does not sum to 1 within 1e-12."""
    miscall, dropout = _arr(miscall, np.float64), _arr(dropout, np.float64)
    if miscall.shape != (3, 3) or dropout.shape != (3,):
        raise ValueError("miscall is (3, 3), dropout (3,)")
    othr = np.zeros((3, 3), dtype=np.uint64)
    text = C.create_string_buffer(256)
    rc = load_library().abn_sim_obs_thresholds(_ptr(miscall), _ptr(dropout), _ptr(othr), text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return othr


def _rows(packed, nodes):
    packed, nodes = _arr(packed, np.uint8), _arr(nodes, np.int32, -1)
    if packed.ndim != 2 or packed.shape[0] != nodes.shape[0]:
        raise ValueError("packed is (rows, row_stride) uint8 with one node per row")
    return packed, nodes


def observe(ctx, seed, packed, nodes, othr, n_sites, out_stride=None) -> np.ndarray:
    """The observation of the packed rows (abn_sim_observe) on the device: row r is the methylome of node nodes[r]; the
    field of a true state s becomes the number of othr[s] the site's draw reaches, 3 = filtered.  Returns packed uint8
    (rows, out_stride), out_stride = packed's unless given; bytes of a longer stride than packed_row_stride(n_sites) are
    zero."""
    packed, nodes = _rows(packed, nodes)
    othr = _othr(othr)
    out = np.zeros((packed.shape[0], packed.shape[1] if out_stride is None else int(out_stride)), dtype=np.uint8)
    ctx._check(ctx._L.abn_sim_observe(ctx._h, int(seed), packed.shape[0], _ptr(nodes), _ptr(othr), int(n_sites), _ptr(packed),
                                      packed.shape[1], _ptr(out), out.shape[1]))
    return out


def observe_dev(ctx, seed, nodes, othr, n_sites, in_ptr: int, in_stride: int, out_ptr: int, out_stride: int) -> float:
    """The same between device matrices (abn_sim_observe_dev; both 16-byte aligned): in_ptr == out_ptr with equal strides
    observes in place, any other overlap is refused.  Returns the kernel's HIP-event ms."""
    nodes, othr = _arr(nodes, np.int32, -1), _othr(othr)
    return ctx._timed(ctx._L.abn_sim_observe_dev, int(seed), nodes.shape[0], _ptr(nodes), _ptr(othr), int(n_sites), _dev(in_ptr),
                      int(in_stride), _dev(out_ptr), int(out_stride))


def observe_host(seed, packed, nodes, othr, n_sites, out_stride=None, walk_blocks=0, lazy=True, in_place=False) -> np.ndarray:
    """observe in its host forms (abn_sim_observe_host): no device needed; the same bytes and the same refusals.
    walk_blocks = 0: the law site by site; > 0: the kernel's lane function over that many workgroups' grid stride (lazy =
    False: the low words always drawn).  in_place: observed in a copy of packed itself."""
    packed, nodes = _rows(packed, nodes)
    othr = _othr(othr)
    if in_place:
        packed = packed.copy()
        out = packed
    else:
        out = np.zeros((packed.shape[0], packed.shape[1] if out_stride is None else int(out_stride)), dtype=np.uint8)
    H = load_host_library()
    H.abn_sim_observe_host.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                       C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_char_p, C.c_int]
    text = C.create_string_buffer(256)
    rc = H.abn_sim_observe_host(int(seed), packed.shape[0], nodes.ctypes.data, othr.ctypes.data, int(n_sites), packed.ctypes.data,
                                packed.shape[1], out.ctypes.data, out.shape[1], int(walk_blocks), int(bool(lazy)), text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return out


def noise(miscall_rate, dropout_rate):
    """(miscall (3, 3), dropout (3,)) of one miscall probability split evenly over the two other states and one dropout
    probability whatever the state: what `alphabeta --sim-miscall E --sim-dropout F` asks for"""
    e, f = float(miscall_rate), float(dropout_rate)
    m = np.full((3, 3), 0.5 * e)
    np.fill_diagonal(m, 1.0 - e)
    return m, np.full(3, f)


def study(ctx, seed, parent, generation, emit, alpha, beta, p_uu0, weight, n_sites, n_replicates, miscall=None, dropout=None,
          with_ms=False):
    """A replicate study (abn_sim_study): n_replicates pedigrees of n_sites sites as the column ranges of ONE simulation,
    observed in place where miscall or dropout is given (the other then the identity / zeros), scanned and counted in one
    windows scan and one census.  Returns (times (pairs, 3) = [t0, t1, t2], D (R, pairs), p0uu (R,), census (R, emitted, 3)
    uint64 = the kept fields 0, 1, 2 of every sample) and, with_ms, the HIP-event ms of the simulation, the observation, the
    scan and the census.  Replicate r with times is the pedigree Context.ab_neutral_run or a Plan window takes."""
    thr = thresholds(parent, generation, alpha, beta, p_uu0, weight)
    generation = _arr(generation, np.int32, -1)
    parent, thr, emit = _arguments(parent, thr, emit)
    othr = None
    if miscall is not None or dropout is not None:
        othr = obs_thresholds(np.eye(3) if miscall is None else miscall, np.zeros(3) if dropout is None else dropout)
    n, R = int(np.count_nonzero(emit)), int(n_replicates)
    pairs = max(n * (n - 1) // 2, 1)
    times, D, p0uu = np.zeros((pairs, 3)), np.zeros((max(R, 1), pairs)), np.zeros(max(R, 1))
    census, ms = np.zeros((max(R, 1), max(n, 1), 3), dtype=np.uint64), np.zeros(4)
    ctx._check(ctx._L.abn_sim_study(ctx._h, int(seed), parent.shape[0], _ptr(parent), _ptr(generation), _ptr(thr), _ptr(emit),
                                    _ptr(othr), int(n_sites), R, _ptr(times), _ptr(D), _ptr(p0uu), _ptr(census), _ptr(ms)))
    return (times, D, p0uu, census, ms) if with_ms else (times, D, p0uu, census)
