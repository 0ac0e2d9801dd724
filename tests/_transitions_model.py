"""The 3 x 3 state transition table of a sample pair, restated in numpy (the joint table behind DMatrix::from,
src/pedigree.rs:236-257): over the sites where neither byte code carries the filter, T[x][y] = #{k : s_a[k] = x, s_b[k] = y}
with a < b.  Shared by tests/test_transitions_cpu.py and tests/test_transitions_gpu.py; independent of the product."""
import numpy as np

WEIGHT = np.abs(np.arange(3)[:, None] - np.arange(3)[None, :]).astype(np.uint64)     # |x - y|


def pair_table(ca, cb):
    """byte codes (status | 0x80 when filtered) of two samples -> uint64 (3, 3)"""
    keep = ((ca | cb) & 0x80) == 0
    return np.bincount(3 * (ca[keep] & 3).astype(np.int64) + (cb[keep] & 3), minlength=9).astype(np.uint64).reshape(3, 3)


def table(codes):
    """byte codes (n, sites) -> uint64 (pairs, 3, 3) in the reference's pair order"""
    n = codes.shape[0]
    out = np.zeros((n * (n - 1) // 2, 3, 3), dtype=np.uint64)
    p = 0
    for a in range(n):
        for b in range(a + 1, n):
            out[p] = pair_table(codes[a], codes[b])
            p += 1
    return out


def windows_table(codes, begin, end):
    """... of every column range [begin[w], end[w]): uint64 (W, pairs, 3, 3)"""
    n = codes.shape[0]
    out = np.zeros((len(begin), n * (n - 1) // 2, 3, 3), dtype=np.uint64)
    for w, (b, e) in enumerate(zip(begin, end)):
        out[w] = table(codes[:, int(b):int(e)])
    return out


def table_by_planes(codes):
    """table() for many samples: the same counts as nine products of the 0 / 1 planes [status = x and not filtered], in
    float64 (exact below 2^53); tests/test_transitions_cpu.py holds it against table()"""
    n = codes.shape[0]
    planes = [((codes == x)).astype(np.float64) for x in range(3)]              # a filtered code is 0x80 | status: none
    iu = np.triu_indices(n, 1)                                                  # row-major: the reference's pair order
    out = np.zeros((len(iu[0]), 3, 3), dtype=np.uint64)
    for x in range(3):
        for y in range(3):
            out[:, x, y] = (planes[x] @ planes[y].T)[iu].astype(np.uint64)
    return out


def windows_table_by_planes(codes, begin, end):
    return np.stack([table_by_planes(codes[:, int(b):int(e)]) for b, e in zip(begin, end)]) if len(begin) else \
        np.zeros((0, codes.shape[0] * (codes.shape[0] - 1) // 2, 3, 3), dtype=np.uint64)


def folds(t):
    """(both, diff) of tables (..., 3, 3)"""
    return t.sum(axis=(-1, -2)), (t * WEIGHT).sum(axis=(-1, -2))


# the edge-window set of tests/test_pairwise_windows_packed.py (a copy: that file is not imported)
SITES = 6001
EDGE_LENGTHS = [0, 1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 2049]


def edge_windows():
    begin, end = [], []
    pos = 0
    for k, ln in enumerate(EDGE_LENGTHS * 3):
        b = pos // 16 * 16 + k % 16
        b = min(b, SITES - ln)
        begin.append(b)
        end.append(b + ln)
        pos = (b + ln // 2 + 5) % (SITES - 2100)
    extra = [(63, 66), (64, 65), (65, 70), (255, 258), (256, 512), (257, 300), (1023, 1025), (1024, 1280), (1025, 1279),
             (37, 40), (33, 47), (300, 500), (515, 767),                # inside one dword; inside one super-step
             (0, 64), (0, 1), (SITES - 129, SITES), (SITES - 1, SITES), (0, SITES), (SITES, SITES), (2, SITES - 3)]
    begin += [b for b, _ in extra]
    end += [e for _, e in extra]
    return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


def random_codes(seed, n, sites):
    """(status, pmax, byte codes) with a long filtered stretch in sample 0 and sample 2 filtered throughout"""
    rng = np.random.default_rng(seed)
    status = rng.integers(0, 3, size=(n, sites), dtype=np.uint8)
    pmax = rng.uniform(0.9, 1.0, size=(n, sites))
    pmax[0, : sites // 2] = 0.5
    if n > 2:
        pmax[2] = 0.1
    return status, pmax, (status | np.where(pmax < 0.99, 0x80, 0)).astype(np.uint8)
