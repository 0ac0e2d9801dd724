"""abn_packed_region_states* and abn_regions_*: region-level methylation states of a 2-bit packed code matrix.

One field per (sample, region), called from the sample's single-site fields inside the region by a rule of exact integers
(csrc/abn_regions.hpp: 3 if kept < min_kept; 0 if m den < lo_num 2 kept; 2 if m den > hi_num 2 kept; else 1, with
m = n1 + 2 n2), in the packed format every scan and the census take.  A module of its own, imported by its name:

    from alphabeta_rs_amd import regions
    out = regions.region_states(ctx, packed, n_sites, begin, end, 1, 3, 4)
    reg = regions.from_tiles(tiles, 250_000, 750_000, 1_000_000)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import AbnError, _arr, _dev, _Handle, _pair_outputs, _pair_tables, _ptr, _window_ranges, load_host_library


def _matrix(packed):
    packed = _arr(packed, np.uint8)
    if packed.ndim != 2:
        raise ValueError("packed is (samples, row_stride) uint8")
    return packed


def _columns(src, n_windows, n_columns):
    """(src int32 or None, C)"""
    if src is None:
        return None, n_windows if n_columns is None else int(n_columns)
    src = _arr(src, np.int32)
    if src.ndim != 1:
        raise ValueError("src is a 1-d array")
    return src, src.shape[0] if n_columns is None else int(n_columns)


def _out_stride(n_columns: int) -> int:
    """abn_packed_row_stride(n_columns)"""
    return 0 if n_columns <= 0 else (n_columns + 255) // 256 * 64


def region_states(ctx, packed, n_sites, begin, end, lo_num, hi_num, den, min_kept=1, *, src=None, n_columns=None,
                  long_sites=0) -> np.ndarray:
    """The region matrix (samples, abn_packed_row_stride(C)) uint8 of the packed matrix (samples, row_stride) on the device
    (abn_packed_region_states): column c = the field of window src[c] (None: the identity)"""
    packed = _matrix(packed)
    b, e = _window_ranges(begin, end)
    src, n_cols = _columns(src, b.shape[0], n_columns)
    out = np.zeros((packed.shape[0], _out_stride(n_cols)), dtype=np.uint8)
    ctx._check(ctx._L.abn_packed_region_states(ctx._h, _ptr(packed), packed.shape[0], int(n_sites), packed.shape[1], _ptr(b),
                                               _ptr(e), b.shape[0], _ptr(src), n_cols, int(lo_num), int(hi_num), int(den),
                                               int(min_kept), int(long_sites), _ptr(out)))
    return out


def region_states_dev(ctx, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int, begin, end, lo_num, hi_num, den,
                      min_kept, out_ptr: int, *, src=None, n_columns=None, long_sites=0) -> np.ndarray:
    """The same of a device matrix (16-byte aligned) into a device output [samples x abn_packed_row_stride(C)]
    (abn_packed_region_states_dev); the window and src arrays are the host's.  Returns the HIP-event ms (2,) of the long
    windows' census and of the kernel."""
    b, e = _window_ranges(begin, end)
    src, n_cols = _columns(src, b.shape[0], n_columns)
    ms = np.zeros(2)
    ctx._check(ctx._L.abn_packed_region_states_dev(ctx._h, _dev(packed_ptr), int(n_samples), int(n_sites), int(row_stride),
                                                   _ptr(b), _ptr(e), b.shape[0], _ptr(src), n_cols, int(lo_num), int(hi_num),
                                                   int(den), int(min_kept), int(long_sites), _dev(out_ptr), _ptr(ms)))
    return ms


def region_states_host(packed, n_sites, begin, end, lo_num, hi_num, den, min_kept=1, *, src=None, n_columns=None,
                       long_sites=0, walk=False) -> np.ndarray:
    """region_states in its host forms (abn_packed_region_states_host): no device needed.  walk False: the law field by
    field; True: the kernel's lane and workgroup structure, windows of long_sites sites or more through the census's walk"""
    packed = _matrix(packed)
    b, e = _window_ranges(begin, end)
    src, n_cols = _columns(src, b.shape[0], n_columns)
    out = np.zeros((packed.shape[0], _out_stride(n_cols)), dtype=np.uint8)
    H = load_host_library()
    ll = C.c_longlong
    H.abn_packed_region_states_host.argtypes = [C.c_void_p, C.c_int, ll, ll, C.c_void_p, C.c_void_p, ll, C.c_void_p, ll, ll, ll,
                                                ll, ll, ll, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    text = C.create_string_buffer(256)
    rc = H.abn_packed_region_states_host(packed.ctypes.data, packed.shape[0], int(n_sites), packed.shape[1], b.ctypes.data,
                                         e.ctypes.data, b.shape[0], None if src is None else src.ctypes.data, n_cols,
                                         int(lo_num), int(hi_num), int(den), int(min_kept), int(long_sites),
                                         out.ctypes.data if out.size else None, int(bool(walk)), text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return out


def call_host(n0, n1, n2, lo_num, hi_num, den, min_kept=1) -> int:
    """region_call on planted counts (abn_region_call_host): the field 0..3"""
    H = load_host_library()
    ull, ll = C.c_ulonglong, C.c_longlong
    H.abn_region_call_host.argtypes = [ull, ull, ull, ll, ll, ll, ll]
    f = H.abn_region_call_host(int(n0), int(n1), int(n2), int(lo_num), int(hi_num), int(den), int(min_kept))
    if f < 0:
        raise AbnError(1, "the rule is not 0 <= lo_num <= hi_num <= den with den in 1..2^20 and min_kept >= 1")
    return f


class Regions(_Handle):
    """What from_tiles returns, and part of this module's surface for that reason alone: from_tiles makes it.  abn_regions:
    the region matrix of a tiles handle — every tile one column, the columns in ascending (group, tile) — device-resident
    and independent of the tiles handle it came from"""

    _DESTROY, _PREFIX = "abn_regions_destroy", "abn_regions"

    def info(self):
        """{n_samples, n_columns, row_stride (bytes), n_groups}"""
        n, g, cols, stride = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self._L.abn_regions_info(self._h, C.byref(n), C.byref(cols), C.byref(stride), C.byref(g)))
        return {"n_samples": n.value, "n_columns": cols.value, "row_stride": stride.value, "n_groups": g.value}

    def layout(self):
        """(group_begin int64, group_end int64), each (n_groups,): every group's columns"""
        G = self.info()["n_groups"]
        gb, ge = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
        self._check(self._L.abn_regions_layout(self._h, _ptr(gb), _ptr(ge)))
        return gb, ge

    def order(self) -> np.ndarray:
        """int32 (n_columns,): the tile of each column"""
        src = np.zeros(self.info()["n_columns"], dtype=np.int32)
        self._check(self._L.abn_regions_order(self._h, _ptr(src)))
        return src

    def packed(self) -> np.ndarray:
        """the region matrix (n_samples, row_stride) uint8, copied to the host"""
        i = self.info()
        out = np.empty((i["n_samples"], i["row_stride"]), dtype=np.uint8)
        self._check(self._L.abn_regions_packed(self._h, _ptr(out)))
        return out

    def packed_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._L.abn_regions_packed_device_ptr(self._h, C.byref(p)))
        return p.value or 0

    def census(self) -> np.ndarray:
        """uint64 (n_groups, n_samples, 3): the regions of every group each sample calls 0, 1 and 2"""
        i = self.info()
        counts = np.zeros((i["n_groups"], i["n_samples"], 3), dtype=np.uint64)
        self._check(self._L.abn_regions_census(self._h, _ptr(counts)))
        return counts

    def pairwise(self):
        """(diff, both, dvalue), each (n_groups, pairs): pairwise_divergence_windows_packed over the groups' columns"""
        i = self.info()
        diff, both, dval = _pair_outputs(i["n_samples"], (i["n_groups"],))
        self._check(self._L.abn_regions_pairwise(self._h, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval

    def transitions(self) -> np.ndarray:
        """uint64 (n_groups, pairs, 3, 3): pairwise_transitions_windows_packed over the groups' columns"""
        i = self.info()
        table = _pair_tables(i["n_samples"], (i["n_groups"],))
        self._check(self._L.abn_regions_transitions(self._h, _ptr(table)))
        return table

    def kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of the long tiles' census and of the kernel"""
        return self._ms(self._L.abn_regions_kernel_ms, 2)


def from_tiles(tiles, lo_num, hi_num, den, min_kept=1, group=None, n_groups=1) -> Regions:
    """The region matrix of a Tiles handle after set_intervals or set_fixed (abn_tiles_region_states).  group (n_tiles,)
    int32 puts every tile into a group in [0, n_groups), -1 leaves it out; None: all in group 0."""
    self = Regions._new(tiles.ctx)
    g = None if group is None else _arr(group, np.int32)
    if g is not None and g.shape != (max(tiles.info()["n_tiles"], 0),):
        raise ValueError("group is (n_tiles,)")
    h = C.c_void_p()
    self._check(self._L.abn_tiles_region_states(tiles._h, int(lo_num), int(hi_num), int(den), int(min_kept), _ptr(g),
                                                int(n_groups), C.byref(h)))
    self._h = h
    return self
