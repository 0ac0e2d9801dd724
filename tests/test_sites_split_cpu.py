"""Methylation contexts on the host: the masked line parsers (parse_site_full, abn_parse_line) against the RELABEL oracle —
the CG-only parser of the parent behaviour on a text whose field 3 is rewritten reads what the parser of one context
reads on the text itself — and the partition by context (alphabeta_rs_amd/csrc/abn_sites_split.hpp) in its serial form
against the single-context parses."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _contexts_model as X
import _parse_model as P

ROOT = Path(__file__).resolve().parent.parent
RECORD_KEYS = ("line", "meta", "start", "end", "posteriormax", "meth_lvl")


@pytest.fixture(scope="module")
def L():
    return X.hostlib()


# ---------------------------------------------------------------- the relabel oracle
@pytest.mark.parametrize("name,text", X.texts(), ids=[n for n, _ in X.texts()])
def test_masked_host_parser_equals_cg_parser_on_relabelled_text(L, name, text):
    for skip_lines in (0, 1):
        for c in range(3):
            want, _ = P.host_sites(L, X.relabel(text, c), skip_lines)        # the parent behaviour: CG alone
            got = X.host_sites(L, text, 1 << c, skip_lines)
            P.assert_sites_equal(got, want)
            rows = got["context"] == 3
            assert set(got["context"][~rows].tolist()) <= {c}, (name, c)
    plain, _ = P.host_sites(L, text, 1)                                      # the default mask is the parent's parser
    P.assert_sites_equal(X.host_sites(L, text, 1, 1), plain)


def test_relabel_oracle_rewrites_what_it_should():
    text = b"h\n1\t5\t+\tCHG\t1\t2\t0.5\tM\t0.5\n1\t6\t+\tCG\t1\t2\t0.5\tM\t0.5\tCGA\n1\t2\t3\tCHG\n1 7 8 CG\n"
    assert X.relabel(text, 0) == text
    assert X.relabel(text, 1) == b"h\n1\t5\t+\tCG\t1\t2\t0.5\tM\t0.5\n1\t6\t+\tXX\t1\t2\t0.5\tM\t0.5\tCGA\n1\t2\t3\tCHG\n1 7 8 CG\n"
    assert X.relabel(text, 2) == text.replace(b"\tCG\t", b"\tXX\t")


def test_golden_methylome_counts(L):
    assert len(P.GOLDEN_METHYLOMES) == 4
    for path in P.GOLDEN_METHYLOMES:
        text = path.read_bytes()
        for mask, n in X.GOLDEN_COUNTS.items():
            sites = X.host_sites(L, text, mask, skip_lines=1)
            assert len(sites["line"]) == n, (path.name, mask)
        by_code = np.bincount(X.host_sites(L, text, 7)["context"], minlength=4)
        assert by_code.tolist() == [500, 400, 1900, 0], path.name


def test_every_mask_accepts_rows_without_a_context(L):
    text = X.rows_only_text(300)
    for mask in X.MASKS:
        sites = X.host_sites(L, text, mask)
        assert len(sites["line"]) == 300 and set(sites["context"].tolist()) == {3}
        cls, dev = X.classify(L, text, mask)
        assert cls.tolist() == [1] * 300 and set(dev["context"].tolist()) == {3}


# ---------------------------------------------------------------- the classifier the device shares
def test_classifier_agrees_with_masked_host_parser_on_every_line(L):
    text = X.torture_text()
    fields3 = X.line_contexts(text)[1:]                                      # the lines from skip_lines = 1 on
    spans = P.line_spans(text)
    n_deferred = {m: 0 for m in X.MASKS}
    for mask in X.MASKS:
        host = X.host_sites(L, text, mask)
        cls, dev = X.classify(L, text, mask)
        assert len(cls) == len(spans) - 1
        host_at = {int(l): i for i, l in enumerate(host["line"])}
        decided = []                                                         # (line, the host's index) of the deferred sites
        for k, c in enumerate(cls.tolist()):
            line, ctx = k + 1, fields3[k]
            in_mask = ctx in X.CONTEXTS and (mask >> X.CONTEXTS.index(ctx)) & 1
            if ctx is not None and not in_mask:
                assert c == 0, (mask, line, ctx, "a line outside the mask is no site, and never deferred")
            if c == 2:
                off, n = spans[line]
                one = X.host_sites(L, text[off:off + n], mask, skip_lines=0)  # the deferred line goes to the host's parser
                assert (len(one["line"]) == 1) == (line in host_at), (mask, line)
                if line in host_at:
                    P.assert_sites_equal({k2: v for k2, v in one.items() if k2 != "line"},
                                         {k2: v[host_at[line]:host_at[line] + 1] for k2, v in host.items()},
                                         [k2 for k2, _ in P.FIELDS if k2 != "line"] + ["context"])
                    decided.append(line)
                n_deferred[mask] += 1
            elif c == 0:
                assert line not in host_at, (mask, line)
        assert sorted(dev["line"].tolist() + decided) == host["line"].tolist(), mask
        at = np.array([host_at[int(l)] for l in dev["line"]], dtype=np.int64)
        P.assert_sites_equal(dev, {k: v[at] for k, v in host.items()}, [k for k, _ in P.FIELDS] + ["context"])
    assert n_deferred[1] > 0 and n_deferred[2] == n_deferred[1] == n_deferred[4]
    assert n_deferred[7] == 3 * n_deferred[1] and n_deferred[6] == 2 * n_deferred[1]


def test_default_mask_is_cg_alone(L):
    text = X.torture_text()
    cls0, dev0 = P.classify(L, text)
    cls1, dev1 = X.classify(L, text, 1)
    assert cls0.tobytes() == cls1.tobytes()
    P.assert_sites_equal(dev1, dev0, [k for k, _ in P.FIELDS] + ["status_flag"])
    assert set(dev1["context"].tolist()) == {0, 3}


# ---------------------------------------------------------------- the serial partition
def slabs(text, slab_bytes):
    """the (begin, end) of every slab as abn_sites_parse cuts them: behind the last '\\n' of slab_bytes bytes"""
    out, at = [], 0
    while at < len(text):
        if not slab_bytes or len(text) - at <= slab_bytes:
            to = len(text)
        else:
            hit = text.rfind(b"\n", at, at + slab_bytes)
            if hit < 0:
                fwd = text.find(b"\n", at + slab_bytes)
                to = len(text) if fwd < 0 else fwd + 1
            else:
                to = hit + 1
        out.append((at, to))
        at = to
    return out


def exact_text(n, mask, seed):
    """a plain methylome of exactly n lines, all of a context in the mask: n records under that mask"""
    head, *rows = P.plain_text(8 * n + 64, seed=seed, cg_every=3).decode().split("\n")
    keep = [r for r in rows if r and (mask >> X.CONTEXTS.index(r.split("\t")[3])) & 1][:n]
    assert len(keep) == n
    return ("\n".join([head] + keep) + "\n").encode()


def split_serial(L, text, mask, slab_bytes):
    """The device's side of a resident handle emulated with the classifier — the records per slab, slab-relative lines,
    the meta word — through sites_split_serial, the deferred lines the host accepts handed to the children by membership,
    each child then merged by line -> {c: sites dict}, the children's chunk sizes, the inserted codes seen"""
    cls, dev = X.classify(L, text, mask, skip_lines=1)
    spans = P.line_spans(text)
    begins = np.array([b for b, _ in spans] + [len(text)], dtype=np.int64)
    chunk_of_line = np.zeros(len(spans), dtype=np.int64)
    cuts = slabs(text, slab_bytes)
    line0 = [int(np.searchsorted(begins, b)) for b, _ in cuts]
    for k, (b, e) in enumerate(cuts):
        chunk_of_line[(begins[:-1] >= b) & (begins[:-1] < e)] = k
    chunk = chunk_of_line[dev["line"]]
    chunk_n = np.bincount(chunk, minlength=len(cuts)).astype(np.int64)
    n = len(dev["line"])
    meta = (dev["chromosome"].astype(np.uint32) | dev["strand"].astype(np.uint32) << 16 | dev["status"].astype(np.uint32) << 20 |
            dev["status_flag"].astype(np.uint32) << 24 | dev["context"].astype(np.uint32) << 28)
    rel = (dev["line"] - np.array(line0, dtype=np.int64)[chunk]).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    src = [np.ascontiguousarray(a) for a in (rel, meta, dev["start"], dev["end"], dev["posteriormax"], dev["meth_lvl"])]
    size = np.full(3 * len(cuts), 0xdead, dtype=np.uint32)
    out = [np.full(3 * n, 7, dtype=a.dtype) for a in src]
    types = L.abh_sites_split_serial.argtypes
    p = lambda a, t: a.ctypes.data_as(t)
    rc = L.abh_sites_split_serial(len(cuts), mask, p(chunk_n, types[2]), *(p(a, t) for a, t in zip(src, types[3:9])),
                                  p(size, types[9]), *(p(a, t) for a, t in zip(out, types[10:16])))
    assert rc == int(np.sum((chunk_n + 255) // 256)), rc
    size = size.reshape(len(cuts), 3)
    deferred = {"line": np.flatnonzero(cls == 2) + 1}
    deferred["offset"] = np.array([spans[l][0] for l in deferred["line"]], dtype=np.int64)
    deferred["length"] = np.array([spans[l][1] for l in deferred["line"]], dtype=np.int64)
    ins = X.decide(L, text, deferred, mask)
    children = {}
    for c in range(3):
        if not (mask >> c) & 1:
            assert size[:, c].sum() == 0
            continue
        k = int(size[:, c].sum())
        got = [a[c * n:c * n + k] for a in out]
        lines = got[0].astype(np.int64) + np.repeat(np.array(line0, dtype=np.int64), size[:, c])
        mine = (ins[8] == c) | (ins[8] == 3)
        rec = {"line": lines, "chromosome": (got[1] & 0xffff).astype(np.int32), "start": got[2], "end": got[3],
               "strand": ((got[1] >> 16) & 0xf).astype(np.uint8), "posteriormax": got[4],
               "status": ((got[1] >> 20) & 0xf).astype(np.uint8), "meth_lvl": got[5], "context": ((got[1] >> 28) & 3).astype(np.uint8)}
        names = ("line", "chromosome", "start", "end", "strand", "posteriormax", "status", "meth_lvl", "context")
        both = {key: np.concatenate([rec[key], ins[i][mine]]) for i, key in enumerate(names)}
        order = np.argsort(both["line"], kind="stable")
        children[c] = {key: v[order] for key, v in both.items()}
    return children, size, ins[8]


def check_split(L, text, mask, slab_bytes, label):
    children, size, inserted_codes = split_serial(L, text, mask, slab_bytes)
    assert sorted(children) == [c for c in range(3) if (mask >> c) & 1], label
    for c, got in children.items():
        want = X.host_sites(L, text, 1 << c)                                 # the single-context parse
        P.assert_sites_equal(got, want, [k for k, _ in P.FIELDS] + ["context"])
    return size, inserted_codes


@pytest.mark.parametrize("mask", [3, 5, 6, 7])
def test_serial_split_equals_single_context_parses(L, mask):
    for n in (0, 1, 255, 256, 257, 1025):                                    # records of the parent, in one chunk and in several
        text = exact_text(n, mask, seed=100 + n)
        for slab_bytes in (0, 300, 4096):
            size, _ = check_split(L, text, mask, slab_bytes, (n, slab_bytes))
            assert int(size.sum()) == n
            assert size.shape[0] == (1 if n == 0 or not slab_bytes else len(slabs(text, slab_bytes)))
    inserted = set()
    for name, text in X.texts():
        for slab_bytes in (300, 4096):
            size, codes = check_split(L, text, mask, slab_bytes, (name, slab_bytes))
            assert size.shape[0] > 1
            inserted |= set(codes.tolist())
    assert inserted == {c for c in range(3) if (mask >> c) & 1}              # inserted records of every context of the mask
    # a chunk with no record of one context: 40 lines of the mask's first context in front of the mixed ones
    first = min(c for c in range(3) if (mask >> c) & 1)
    lead = exact_text(40, 1 << first, seed=5).decode().split("\n", 1)[1]
    head, rest = exact_text(300, mask, seed=6).decode().split("\n", 1)
    size, _ = check_split(L, (head + "\n" + lead + rest).encode(), mask, 300, "empty context")
    others = [c for c in range(3) if (mask >> c) & 1 and c != first]
    assert size[0, first] > 0 and all(size[0, c] == 0 for c in others) and all(size[:, c].sum() > 0 for c in others)
    # 4-field rows alone: every child holds all of them
    rows = X.rows_only_text(300)
    size, _ = check_split(L, rows, mask, 300, "rows")
    assert all(int(size[:, c].sum()) == (300 if (mask >> c) & 1 else 0) for c in range(3))


def test_split_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial partition over chunk lists of every shape, every
    array in a heap block of exactly its length, built with -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for the sanitizer build of tests/native/sites_split_main.cpp")
    exe = tmp_path / "sites_split_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o",
                        str(exe), str(ROOT / "tests" / "native" / "sites_split_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sanitized sites split ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------- the ABI
def test_sites_params_layout_and_symbols():
    import alphabeta_rs_amd as abn

    assert C.sizeof(abn.SitesParams) == 16
    assert abn.SitesParams.contexts.offset == 12 and abn.SitesParams.contexts.size == 4
    assert [f[0] for f in abn.SitesParams._fields_] == ["slab_bytes", "skip_lines", "contexts"]
    for name in ("abn_sites_context", "abn_sites_insert_ctx", "abn_sites_split", "abn_sites_split_ms"):
        assert name in abn.EXPORTED_SYMBOLS
    header = (ROOT / "include" / "abneutral.h").read_text()
    assert "int32_t contexts;" in header and "int32_t reserved;" not in header
    assert abn._context_mask(("CG",)) == 1 and abn._context_mask("CG,CHH") == 5 and abn._context_mask(("CHG", "CHH", "CG")) == 7
    for bad in ((), ("CG", "CG"), ("CH",), "CG,,CHG", ("cg",)):
        with pytest.raises(ValueError):
            abn._context_mask(bad)
