"""abn_packed_census_windows*: the state census of a 2-bit packed code matrix per column range, as functions on a Context.

counts (windows, samples, 3) uint64: the fields 0, 1 and 2 (U, I, M) every sample holds inside [begin[w], end[w]) — what
rc_meth_lvl over a sample's own kept sites needs once sites drop out of single samples (csrc/abn_packed_census.hpp).  A
module of its own, imported by its name:

    from alphabeta_rs_amd import census
    counts = census.census_windows(ctx, packed, n_sites, begin, end)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import AbnError, _arr, _dev, _ptr, _window_ranges, load_host_library


def _matrix(packed):
    packed = _arr(packed, np.uint8)
    if packed.ndim != 2:
        raise ValueError("packed is (samples, row_stride) uint8")
    return packed


def census_windows(ctx, packed, n_sites, begin, end) -> np.ndarray:
    """counts (windows, samples, 3) uint64 of the packed matrix (samples, row_stride) on the device
    (abn_packed_census_windows); arguments and refusals of Context.pairwise_divergence_windows_packed, one sample served"""
    packed = _matrix(packed)
    b, e = _window_ranges(begin, end)
    counts = np.zeros((b.shape[0], packed.shape[0], 3), dtype=np.uint64)
    ctx._check(ctx._L.abn_packed_census_windows(ctx._h, _ptr(packed), packed.shape[0], int(n_sites), packed.shape[1], _ptr(b),
                                                _ptr(e), b.shape[0], _ptr(counts)))
    return counts


def census_windows_dev(ctx, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int, begin, end, counts_ptr: int) -> float:
    """The same of a device matrix (16-byte aligned) into device counts uint64 [windows x samples x 3]
    (abn_packed_census_windows_dev); the window arrays are the host's.  Returns the two kernels' HIP-event ms."""
    b, e = _window_ranges(begin, end)
    return ctx._timed(ctx._L.abn_packed_census_windows_dev, _dev(packed_ptr), int(n_samples), int(n_sites), int(row_stride),
                      _ptr(b), _ptr(e), b.shape[0], _dev(counts_ptr))


def census_windows_host(packed, n_sites, begin, end, walk_chunk=0) -> np.ndarray:
    """census_windows in its host forms (abn_packed_census_windows_host): no device needed.  walk_chunk = 0: field by field;
    > 0 (a multiple of 256): the kernels' job structure walked with that many sites per job"""
    packed = _matrix(packed)
    b, e = _window_ranges(begin, end)
    counts = np.zeros((b.shape[0], packed.shape[0], 3), dtype=np.uint64)
    H = load_host_library()
    H.abn_packed_census_windows_host.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
    text = C.create_string_buffer(256)
    rc = H.abn_packed_census_windows_host(packed.ctypes.data, packed.shape[0], int(n_sites), packed.shape[1], b.ctypes.data,
                                          e.ctypes.data, b.shape[0], counts.ctypes.data, int(walk_chunk), text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return counts
