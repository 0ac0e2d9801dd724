"""What Pedigree::build reads of a sample's sites (src/pedigree.rs:147-172 and :245-251), as the tests of abn_codes_* spell it
out: the code byte and the `counted` predicate of a site, the packed row through abn_pack_codes, and the rc_meth_lvl fold
as a Python float loop."""
import struct

import numpy as np

FILTER = 0.99
COUNTED = 0x40          # kCodeCounted of csrc/abn_codes.hpp


def code_bytes(status, posteriormax, flt=FILTER):
    """status | 0x80 where posteriormax < filter (src/pedigree.rs:249): a NaN posterior is compared, and not flagged"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(status, dtype=np.uint8) | np.where(np.asarray(posteriormax) < flt, 0x80, 0)).astype(np.uint8)


def counted(posteriormax, flt=FILTER):
    """posteriormax >= filter (src/pedigree.rs:159-172): a NaN posterior is not counted"""
    with np.errstate(invalid="ignore"):
        return np.asarray(posteriormax) >= flt


def fold(posteriormax, meth_lvl, flt=FILTER):
    """(sum as its 8 bytes, kept): `if posteriormax >= filter { sum += meth_lvl; count += 1 }` from 0.0 in file order"""
    s, k = 0.0, 0
    for pm, ml in zip(np.asarray(posteriormax).tolist(), np.asarray(meth_lvl).tolist()):
        if pm >= flt:
            s += ml
            k += 1
    return struct.pack("<d", s), k


def packed_rows(abn, codes_per_sample, stride=None):
    """abn_pack_codes of every sample's code bytes into rows of one stride (that of the longest sample, at least 64):
    every field behind a sample's last site is 3"""
    longest = max((len(c) for c in codes_per_sample), default=0)
    stride = max(abn.packed_row_stride(longest), 64) if stride is None else stride
    rows = [abn.pack_codes(np.asarray(c, dtype=np.uint8).reshape(1, -1), stride)[0] for c in codes_per_sample]
    return np.stack(rows) if rows else np.zeros((0, stride), dtype=np.uint8)
