"""What the sort tests share (tests/test_sites_sort_cpu.py, tests/test_sites_sort_gpu.py): the host shims of
host_capi.cpp, the independent reference for the canonical order — numpy.lexsort, which is stable — the key patterns and
the Python model that puts a methylome text's lines into canonical order."""
import ctypes as C

import numpy as np

import _parse_model as P

KEY_BITS = 75
PASSES = 10


def hostlib():
    L = P.hostlib()
    ll, vp = C.c_longlong, C.c_void_p
    L.abn_sites_sort_keys_host.argtypes = [ll, vp, vp, vp, vp, vp, vp]
    L.abh_sites_sort_walk.argtypes = [ll, vp, vp, vp, vp, C.c_int, vp, vp]
    L.abh_sites_sort_digit.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int]
    L.abh_sites_sort_digit.restype = C.c_uint
    return L


def tile(L) -> int:
    return L.abh_sites_sort_tile()


def sizes(L):
    t = tile(L)
    return (0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17)


def keys(chromosome, start, end, strand):
    return (np.ascontiguousarray(chromosome, dtype=np.int32), np.ascontiguousarray(start, dtype=np.uint32),
            np.ascontiguousarray(end, dtype=np.uint32), np.ascontiguousarray(strand, dtype=np.uint8))


def reference(k):
    """the canonical order of the keys and what the check reports of them, from numpy alone: (order, descents, equal)"""
    chromosome, start, end, strand = k
    order = np.lexsort((strand, end, start, chromosome)).astype(np.int64)
    cols = [a.astype(np.int64) for a in (chromosome, start, end, strand)]
    below = np.zeros(max(len(chromosome) - 1, 0), dtype=bool)
    same = np.ones_like(below)
    for a in cols:                                                           # lexicographic compare of neighbours
        below |= same & (a[1:] < a[:-1])
        same &= a[1:] == a[:-1]
    return order, int(below.sum()), int(same.sum())


def key_int(chromosome, start, end, strand) -> int:
    return (int(chromosome) << 66) | (int(start) << 34) | (int(end) << 2) | int(strand)


def passes_needed(k, descents) -> int:
    """the passes whose digit is not the same in every key, from the 75-bit keys as Python integers; 0 without a descent"""
    if descents == 0:
        return 0
    ints = [key_int(*row) for row in zip(*(a.tolist() for a in k))]
    return sum(1 for p in range(PASSES) if len({(v >> (8 * p)) & 0xff for v in ints}) > 1)


def key_of_bit(bit):
    """(chromosome, start, end, strand) of the key whose only set bit is `bit` of the 75"""
    if bit < 2:
        return 0, 0, 0, 1 << bit
    if bit < 34:
        return 0, 0, 1 << (bit - 2), 0
    if bit < 66:
        return 0, 1 << (bit - 34), 0, 0
    return 1 << (bit - 66), 0, 0, 0


def patterns(n, seed):
    """(name, keys) of every key pattern of size n"""
    rng = np.random.default_rng(seed)
    few = keys(*(rng.integers(0, 3, n) for _ in range(4)))
    full = keys(rng.integers(0, 258, n), rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64),
                rng.integers(0, 3, n))
    equal = keys(np.full(n, 7), np.full(n, 1000), np.full(n, 1001), np.full(n, 1))
    order = reference(full)[0]
    ascending = tuple(a[order] for a in full)
    descending = tuple(a[order[::-1]] for a in full)
    ext = [(c, s, 0xffffffff, 2) for c in (0, 255, 256, 257) for s in (0, 0xffffffff)]
    pick = rng.integers(0, len(ext), n)
    extremes = keys(*(np.array([ext[i][f] for i in pick], dtype=np.uint64) for f in range(4)))
    # a methylome sorted by (chromosome, strand, start): short sites on five chromosomes
    per = n // 5 + 1
    i = np.arange(n)
    strand = (i % per) // (per // 2 + 1)
    start = ((i % per) % (per // 2 + 1)) * 2 + strand
    by_strand = keys(1 + i // per, start, start + 1, strand)
    return (("three values", few), ("full ranges", full), ("all equal", equal), ("sorted", ascending), ("reversed", descending),
            ("extremes", extremes), ("by strand", by_strand))


def bit_pairs():
    """for each of the 75 bits two keys that differ in that bit alone, the higher one first (the other bits random but
    valid: a chromosome up to 257 = 0b100000001, a strand up to 2)"""
    rng = np.random.default_rng(75)
    out = []
    for bit in range(KEY_BITS):
        c, s, e, t = key_of_bit(bit)
        base_c = 0 if bit >= 66 else int(rng.integers(0, 256))
        if bit == 66:                                                        # bit 0 of the chromosome: 256 and 257 too
            base_c = 256
        base_t = 0 if bit < 2 else int(rng.integers(0, 3))
        base_s, base_e = int(rng.integers(0, 1 << 32)) & ~s, int(rng.integers(0, 1 << 32)) & ~e
        low = (base_c, base_s, base_e, base_t)
        high = (base_c | c, base_s | s, base_e | e, base_t | t)
        if high[0] > 257 or high[3] > 2:                                     # (bits 0 and 1 of the strand together are 3)
            continue
        out.append((bit, keys(*zip(high, low))))
    return out


def canonical_text(text: bytes, mask=1, skip_lines=1) -> bytes:
    """The text with its lines below the first skip_lines put into canonical order, stably, by the keys the masked host
    parser reads; a line that is no site goes behind every site (it holds no record, so where it stands does not matter to
    a parse)."""
    import _contexts_model as X

    lines = text.split(b"\n")
    tail = lines.pop() if lines and lines[-1] == b"" else None
    head, body = lines[:skip_lines], lines[skip_lines:]
    L = X.hostlib()
    sites = X.host_sites(L, text, mask, skip_lines=skip_lines)
    k = keys(sites["chromosome"], sites["start"], sites["end"], sites["strand"])
    order = reference(k)[0]
    site_lines = (sites["line"] - skip_lines)[order].tolist()
    used = set(site_lines)
    rest = [i for i in range(len(body)) if i not in used]
    out = head + [body[i] for i in site_lines] + [body[i] for i in rest]
    return b"\n".join(out) + (b"\n" if tail is not None else b"")


def shuffled_text(text: bytes, seed: int, skip_lines=1) -> bytes:
    """the text with its lines below the first skip_lines shuffled by a fixed seed"""
    lines = text.split(b"\n")
    tail = lines.pop() if lines and lines[-1] == b"" else None
    head, body = lines[:skip_lines], lines[skip_lines:]
    perm = np.random.default_rng(seed).permutation(len(body))
    return b"\n".join(head + [body[i] for i in perm]) + (b"\n" if tail is not None else b"")
