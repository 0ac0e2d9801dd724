"""The block bootstrap's argument checks and output arrays, and its two serial host forms."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import _arr, _f64, _ok, _ptr, load_library


def _block_groups(group_begin, group_end, group_id=None):
    gb, ge = (_arr(a, np.int64, -1) for a in (group_begin, group_end))
    gid = np.arange(gb.shape[0], dtype=np.uint32) if group_id is None else _arr(group_id, np.uint32, -1)
    if not gb.shape == ge.shape == gid.shape:
        raise ValueError("group_id, group_begin and group_end differ in length")
    return gid, gb, ge


def _block_counts_array(n_groups, n_replicates, n_blocks):
    return np.zeros((n_groups, int(n_replicates) + 1 if n_replicates >= 0 else 0, max(int(n_blocks), 0)), dtype=np.uint8)


def _block_arguments(group_begin, group_end, counts, both, diff, level_sum_kept, kept):
    _, gb, ge = _block_groups(group_begin, group_end)
    counts = _arr(counts, np.uint8)
    both, diff = _arr(both, np.uint64), _arr(diff, np.uint64)
    lsk, kept = _f64(level_sum_kept), _arr(kept, np.int64)
    if counts.ndim != 3 or counts.shape[0] != gb.shape[0]:
        raise ValueError("counts is (groups, rows, blocks)")
    T = counts.shape[2]
    if both.ndim != 2 or both.shape != diff.shape or both.shape[0] != T:
        raise ValueError("both and diff are (blocks, pairs)")
    if lsk.ndim != 2 or lsk.shape != kept.shape or lsk.shape[1] != T:
        raise ValueError("level_sum_kept and kept are (samples, blocks)")
    dims = (counts.shape[0], counts.shape[1], both.shape[1], lsk.shape[0])  # groups, rows, pairs, samples
    return {"gb": gb, "ge": ge, "counts": counts, "both": both, "diff": diff, "lsk": lsk, "kept": kept, "dims": dims}


def _block_outputs(G, rows, P, n):
    return {"both": np.zeros((G, rows, P), dtype=np.uint64), "diff": np.zeros((G, rows, P), dtype=np.uint64),
            "dvalue": np.zeros((G, rows, P)), "level": np.zeros((G, rows, n)), "kept": np.zeros((G, rows, n), dtype=np.int64)}


def _block_pointers(a, out):
    """the arguments abn_block_resample and abn_block_resample_host share, behind the context"""
    G, rows, P, n = a["dims"]
    return (G, _ptr(a["gb"]), _ptr(a["ge"]), rows, _ptr(a["counts"]), a["counts"].shape[2], P, n, _ptr(a["both"]),
            _ptr(a["diff"]), _ptr(a["lsk"]), _ptr(a["kept"]), *map(_ptr, out.values()))


def block_resample_host(group_begin, group_end, counts, both, diff, level_sum_kept, kept):
    """Context.block_resample in its serial host form (abn_block_resample_host): no device needed; the same refusals"""
    a = _block_arguments(group_begin, group_end, counts, both, diff, level_sum_kept, kept)
    out = _block_outputs(*a["dims"])
    text = C.create_string_buffer(256)
    _ok(load_library().abn_block_resample_host(*_block_pointers(a, out), text, len(text)), text.value.decode())
    return out


def block_counts_host(seed: int, group_id, group_begin, group_end, n_replicates: int, n_blocks: int) -> np.ndarray:
    """Context.block_counts in its serial host form (abn_block_counts_host): no device needed; the same refusals"""
    gid, gb, ge = _block_groups(group_begin, group_end, group_id)
    counts = _block_counts_array(gb.shape[0], n_replicates, n_blocks)
    text = C.create_string_buffer(256)
    _ok(load_library().abn_block_counts_host(int(seed), gb.shape[0], _ptr(gid), _ptr(gb), _ptr(ge), int(n_replicates),
                                             int(n_blocks), _ptr(counts), text, len(text)), text.value.decode())
    return counts
