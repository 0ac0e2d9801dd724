"""abn_sites_dedup*: the collapse of a resident methylome's repeated sites, as functions on a Sites handle and a Context.

Every RUN — a maximal stretch of consecutive records with one (chromosome, start, end, strand) — of records in canonical
order (what Sites.sort() leaves) is collapsed to at most one record by a policy: "first" or "last" of the run in input
order, "best" (the highest posteriormax; ties keep the earlier record, a NaN loses against every number) or "drop" (no
record of a repeated key).  A module of its own, imported by its name:

    from alphabeta_rs_amd import dedup
    collapsed = dedup.dedup(sites.sort(), "best")
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import AbnError, _arr, _ok, _ptr, load_host_library
from .sites import Sites, _site_arrays

POLICIES = ("first", "last", "best", "drop")  # ABN_DEDUP_FIRST .. ABN_DEDUP_DROP


def _policy(policy) -> int:
    """"first" | "last" | "best" | "drop", or the ABN_DEDUP_* number itself"""
    if isinstance(policy, str):
        if policy not in POLICIES:
            raise ValueError(f"policy expects one of {POLICIES}, not {policy!r}")
        return POLICIES.index(policy)
    return int(policy)


def _info(info):
    return {"sites": int(info[0]), "kept": int(info[1]), "repeated": int(info[2]), "disagreeing": int(info[3])}


def dedup(sites: Sites, policy="first") -> Sites:
    """A new resident handle with every run of equal keys of `sites` collapsed to at most one record, on the device
    (abn_sites_dedup).  `sites` is in canonical order; a descent is refused.  The new handle's lines are 0 .. n_sites - 1;
    it goes into Windows.from_parsed, Codes.from_parsed, Tiles and split() as it is.  `sites` stays usable."""
    out = C.c_void_p()
    sites._check(sites._L.abn_sites_dedup(sites._h, _policy(policy), C.byref(out)))
    return Sites(sites.ctx, out)


def dedup_order(sites: Sites) -> np.ndarray:
    """of a handle dedup() made: the index, in the parent's fetch(), of every site, ascending (abn_sites_dedup_order)"""
    return sites._listed(sites._L.abn_sites_dedup_order)


def dedup_info(sites: Sites):
    """of a handle dedup() made: {sites (the parent's), kept, repeated (keys that occurred more than once), disagreeing
    (neighbours of equal key whose status differs), ms: the HIP-event ms of flatten, flags, scan, gather}"""
    info, ms = np.zeros(4, dtype=np.int64), np.zeros(4)
    sites._check(sites._L.abn_sites_dedup_info(sites._h, _ptr(info), _ptr(ms)))
    return {**_info(info), "ms": ms}


def _records(chromosome, start, end, strand, posteriormax, status):
    n = np.asarray(chromosome).reshape(-1).shape[0]
    _, u = _site_arrays([0, n], chromosome, start, end, strand)
    return n, [*u, _arr(posteriormax, np.float64, n), _arr(status, np.uint8, n)]


def dedup_sites(ctx, chromosome, start, end, strand, posteriormax, status, policy="first"):
    """The records kept when every run of equal keys of one sample in canonical order is collapsed, on the device
    (abn_sites_dedup_keys).  Returns (order int64 (kept,), ascending, info): info = {sites, kept, repeated, disagreeing}
    as dedup_info.  AbnError for a descent (sort first), a chromosome outside 0..257 or a strand above 2."""
    n, r = _records(chromosome, start, end, strand, posteriormax, status)
    order, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    ctx._check(ctx._L.abn_sites_dedup_keys(ctx._h, n, *map(_ptr, r), _policy(policy), _ptr(order), _ptr(info)))
    return order[:int(info[1])].copy(), _info(info)


def dedup_sites_host(chromosome, start, end, strand, posteriormax, status, policy="first"):
    """dedup_sites in its serial host form (abn_sites_dedup_keys_host): no device needed; the same result and the same
    refusals"""
    n, r = _records(chromosome, start, end, strand, posteriormax, status)
    order, info, descent = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64), np.full(1, -1, dtype=np.int64)
    H = load_host_library()
    H.abn_sites_dedup_keys_host.argtypes = [C.c_longlong] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3
    rc = H.abn_sites_dedup_keys_host(n, *(a.ctypes.data for a in r), _policy(policy), order.ctypes.data, info.ctypes.data,
                                     descent.ctypes.data)
    if rc and descent[0] >= 0:
        raise AbnError(rc, f"site {int(descent[0])} lies below its predecessor in canonical order: sort first")
    _ok(rc, "a policy outside 0..3, a chromosome outside 0..257 or a strand above 2")
    return order[:int(info[1])].copy(), _info(info)
