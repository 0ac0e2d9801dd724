"""Rows of 2^26 to 2^34 sites with exact expected counts, for tests/test_long_rows_cpu.py and test_long_rows_gpu.py: one
period of P bytes repeated from byte 0 of a buffer ("the stream"), and views (n, L, stride) of it — row r begins at byte
r * stride, at phase (r * stride) mod P of the period.  Every count of a column range is then whole periods times the
period's total plus two prefix counts, in int64: nothing as long as a row is ever built.  numpy only; it never calls the
code under test, and unpacks with the format's rule (site 16 g + 4 j + e lies in byte 4 g + e at bits 2j..2j+1)."""
import numpy as np

P = 4 * 3079                     # bytes of a period: a multiple of a dword and of nothing larger
WEIGHTS = (0.4275, 0.095, 0.4275, 0.05)   # U, I, M and 3 = filtered
ABS = np.abs(np.arange(3)[:, None] - np.arange(3)[None, :]).astype(np.int64)     # |x - y|


def period(seed, kind):
    """one period, uint8 (P,).  kind "packed": 4 P two-bit fields drawn with WEIGHTS; "bytes": byte codes, a state 0 / 1 / 2
    with the weights of U, I, M, | 0x80 with probability 0.05"""
    rng = np.random.default_rng(seed)
    if kind == "packed":
        f = rng.choice(4, size=4 * P, p=WEIGHTS).astype(np.uint8).reshape(P // 4, 4, 4)          # [g][j][e]
        return (f[:, 0] | f[:, 1] << 2 | f[:, 2] << 4 | f[:, 3] << 6).astype(np.uint8).reshape(P)
    assert kind == "bytes"
    w = np.array(WEIGHTS[:3]) / sum(WEIGHTS[:3])
    return (rng.choice(3, size=P, p=w) | np.where(rng.random(P) < WEIGHTS[3], 0x80, 0)).astype(np.uint8)


def packed_stride(L):
    return (L + 255) // 256 * 64


def pair_index(n):
    return np.triu_indices(n, 1)                     # row-major: the reference's pair order


class View:
    """rows r = 0 .. n - 1 of L sites at byte r * stride of the stream of `per` (kind as period())"""

    def __init__(self, per, kind, n, L, stride=None):
        assert per.shape == (P,) and per.dtype == np.uint8
        self.per, self.kind, self.n, self.L = per, kind, int(n), int(L)
        if kind == "packed":
            self.least = packed_stride(self.L)
            self.stride = self.least if stride is None else int(stride)
            assert self.stride % 64 == 0 and self.stride >= self.least
            self.Ps = 4 * P
        else:
            self.stride = self.L if stride is None else int(stride)
            assert self.stride >= self.L
            self.Ps = P
        self.fields = np.stack([self._fields_of_row(r) for r in range(self.n)])         # (n, Ps) of 0..3, 3 = filtered
        self._planes = [(self.fields == x).astype(np.float64) for x in range(3)]
        self._at = {}

    def phase(self, r):
        return r * self.stride % P

    def _fields_of_row(self, r):
        by = np.roll(self.per, -self.phase(r))                                           # the row's first P bytes
        if self.kind == "bytes":
            return np.where(by & 0x80, 3, by & 3).astype(np.uint8)
        g = by.reshape(P // 4, 1, 4)                                                     # [g][.][e]
        return ((g >> (2 * np.arange(4, dtype=np.uint8)).reshape(1, 4, 1)) & 3).reshape(4 * P).astype(np.uint8)

    # ------------------------------------------------------------ the prefix counts, at the residues that are asked for
    def _prefix(self, x):
        """(joint (pairs, 3, 3), single (n, 3)) int64 of the first x sites of a period, 0 <= x <= Ps.  The joint counts
        are products of 0 / 1 planes in float64: integers below 2^53, exact"""
        if x not in self._at:
            iu = pair_index(self.n)
            joint = np.zeros((len(iu[0]), 3, 3), dtype=np.int64)
            for a in range(3):
                for b in range(3):
                    joint[:, a, b] = (self._planes[a][:, :x] @ self._planes[b][:, :x].T)[iu].astype(np.int64)
            single = np.stack([self._planes[a][:, :x].sum(axis=1) for a in range(3)], axis=1).astype(np.int64)
            self._at[x] = (joint, single)
        return self._at[x]

    def _upto(self, x):
        """F(x) = (x // Ps) total + prefix[x % Ps]"""
        x = int(x)
        assert 0 <= x <= self.L
        tj, ts = self._prefix(self.Ps)
        pj, ps = self._prefix(x % self.Ps)
        return (x // self.Ps) * tj + pj, (x // self.Ps) * ts + ps

    def tables(self, begin, end):
        """int64 (W, pairs, 3, 3): T[w][p][x][y] of the column range [begin[w], end[w]) = F(end) - F(begin)"""
        return np.stack([self._upto(e)[0] - self._upto(b)[0] for b, e in zip(begin, end)]) if len(begin) else \
            np.zeros((0, self.n * (self.n - 1) // 2, 3, 3), dtype=np.int64)

    def census(self, begin, end):
        """int64 (W, n, 3): the fields 0, 1, 2 every row holds inside [begin[w], end[w])"""
        return np.stack([self._upto(e)[1] - self._upto(b)[1] for b, e in zip(begin, end)]) if len(begin) else \
            np.zeros((0, self.n, 3), dtype=np.int64)

    # ------------------------------------------------------------ the bytes a test writes or builds
    def stream(self, at, count):
        """bytes [at, at + count) of the stream"""
        return self.per[(at + np.arange(count, dtype=np.int64)) % P]

    def tail_offset(self, r):
        return r * self.stride + self.least - 64

    def tail(self, r):
        """the last 64 bytes of packed row r (its bytes [least - 64, least)) with every field from site L on set to 3: what
        the whole-matrix packed scan requires of a row's padding"""
        assert self.kind == "packed" and self.L > 0
        by = self.stream(self.tail_offset(r), 64).copy()
        i = np.arange(64)
        for j in range(4):
            site = 4 * (self.least - 64) + 16 * (i // 4) + 4 * j + i % 4
            by[site >= self.L] |= np.uint8(3 << (2 * j))
        return by

    def end_of_buffer(self):
        return (self.n - 1) * self.stride + (self.least if self.kind == "packed" else self.L)

    def materialise(self, buffer_bytes=None):
        """the buffer itself, tails patched, for the short rows of the CPU tier: uint8 (buffer_bytes,)"""
        size = self.end_of_buffer() if buffer_bytes is None else buffer_bytes
        buf = np.tile(self.per, size // P + 1)[:size].copy()
        if self.kind == "packed":
            for r in range(self.n):
                buf[self.tail_offset(r): self.tail_offset(r) + 64] = self.tail(r)
        return buf

    def rows(self, buf):
        """the (n, stride) matrix of a buffer that holds the view (padded behind the last row if need be)"""
        need = self.n * self.stride
        if len(buf) < need:
            buf = np.concatenate([buf, np.zeros(need - len(buf), dtype=np.uint8)])
        return buf[:need].reshape(self.n, self.stride)


def folds(t):
    """(both, diff) int64 of tables (..., 3, 3): both = sum T, diff = sum |x - y| T"""
    return t.sum(axis=(-1, -2)), (t * ABS).sum(axis=(-1, -2))


def dvalue(diff, both):
    """D = diff / (2 both) in float64 — the kernel's own expression on operands that are exact below 2^53; 0 / 0 is NaN"""
    diff, both = np.asarray(diff, dtype=np.int64), np.asarray(both, dtype=np.int64)
    assert diff.max(initial=0) < 1 << 53 and both.max(initial=0) < 1 << 53
    with np.errstate(invalid="ignore", divide="ignore"):
        return diff.astype(np.float64) / (2.0 * both.astype(np.float64))


def chunk_of(begin, end, sites, align, max_jobs):
    """(sites per job, grown?, jobs) of one window under the rule of pairwise_windows_chunks (csrc/abn_pairwise.hip)"""
    unit = max(align, 128)
    span = end - (begin - begin % align)
    ch = sites
    grown = (span + ch - 1) // ch > max_jobs
    if grown:
        ch = ((span + max_jobs - 1) // max_jobs + unit - 1) // unit * unit
    return ch, grown, max(1, (span + ch - 1) // ch)
