"""The line parser host and device share (alphabeta_rs_amd/csrc/abn_parse.hpp), compiled for the host in host_capi.cpp:
its f64 path against Python's float() — correctly rounded like strtod — on the tokens the device must be certain of or
leave alone, and its line classifier against the host's parser (parse_site_full through abh_parse_sites) on the bundled
methylomes and on a text of every format and every way out of it.  No GPU."""
import numpy as np

import _parse_model as P


def test_f64_tokens_are_bit_equal_to_float_or_left_to_the_host():
    L = P.hostlib()
    for tok, want in P.TOKENS.items():
        cls, v = P.token_class(L, tok.encode())
        assert cls == want, (tok, cls, want)
        if cls == P.VALUE:
            assert P.bits(v) == P.bits(float(tok)), (tok, v, float(tok))
        elif cls == P.REJECT:                       # no prefix-free reading: the host's parser rejects these too
            try:
                float(tok)
            except ValueError:
                pass
            else:
                raise AssertionError(f"{tok!r} is rejected, but it is a number")
    assert P.bits(P.token_class(L, b"-0.0")[1]) == P.bits(-0.0) != P.bits(0.0)
    # the host's parser agrees with every certain answer (VALUE: a site with that value; REJECT: no site)
    for tok, want in P.TOKENS.items():
        text = (P.HEADER + P.cg_line(pm=tok, ml=tok) + "\n").encode()
        sites, _ = P.host_sites(L, text)
        if want == P.VALUE:
            assert len(sites["line"]) == 1 and P.bits(sites["posteriormax"][0]) == P.bits(float(tok)), tok
        elif want == P.REJECT:
            assert len(sites["line"]) == 0, tok


def test_f64_path_on_generated_decimals():
    """every decimal of up to 15 digits and no exponent is certain, and has float()'s bits"""
    L = P.hostlib()
    rng = np.random.default_rng(5)
    for _ in range(4000):
        nd = int(rng.integers(1, 16))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, size=nd))
        cut = int(rng.integers(0, nd + 1))
        tok = ("-" if rng.integers(4) == 0 else "") + digits[:cut] + "." + digits[cut:]
        if tok.strip("-") == ".":
            continue
        cls, v = P.token_class(L, tok.encode())
        assert cls == P.VALUE and P.bits(v) == P.bits(float(tok)), (tok, cls, v)
    for _ in range(2000):                            # with exponents, wherever the header is certain
        tok = f"{int(rng.integers(0, 2**53 + 1))}e{int(rng.integers(-30, 31))}"
        cls, v = P.token_class(L, tok.encode())
        assert cls in (P.VALUE, P.DEFER)
        if cls == P.VALUE:
            assert P.bits(v) == P.bits(float(tok)), (tok, v)


def check_classifier_against_host(L, text, skip_lines=1):
    """the classifier's sites are the host's sites on the lines it does not defer; returns (cls, sites, host sites)"""
    cls, sites = P.classify(L, text, skip_lines)
    host, n_warnings = P.host_sites(L, text, skip_lines)
    deferred = set((np.flatnonzero(cls == P.DEFER) + skip_lines).tolist())
    keep = np.array([l not in deferred for l in host["line"]], dtype=bool)
    P.assert_sites_equal(sites, {k: a[keep] for k, a in host.items()})
    assert int((cls == 1).sum()) == len(sites["line"])
    if not deferred:
        assert int(sites["status_flag"].sum()) == n_warnings
    return cls, sites, host


def test_line_classifier_equals_the_host_parser_on_the_bundled_methylomes():
    L = P.hostlib()
    assert len(P.GOLDEN_METHYLOMES) == 4
    for path in P.GOLDEN_METHYLOMES:
        text = path.read_bytes()
        for t in (text, text.replace(b"\n", b"\r\n"), text.rstrip(b"\n")):
            for skip in (1, 0):
                cls, sites, host = check_classifier_against_host(L, t, skip)
                assert int((cls == P.DEFER).sum()) == 0        # the condition of the issue: nothing deferred here
                assert len(sites["line"]) == len(host["line"]) == 500


def test_line_classifier_on_the_torture_text():
    L = P.hostlib()
    text = P.torture_text()
    for t in (text, text.replace(b"\n", b"\r\n")):
        cls, sites, host = check_classifier_against_host(L, t)
        spans = P.line_spans(t)
        assert len(cls) == len(spans) - 1 and len(host["line"]) > 100
        # a line is deferred exactly when it is a CG row that every other field accepts and one of whose float columns
        # holds a token the header defers
        want = set()
        for li, (b, n) in enumerate(spans):
            f = t[b:b + n].split(b"\t")
            if li == 0 or len(f) not in (9, 10, 11) or f[3] != b"CG":
                continue
            pm, ml = (f[8], f[10]) if len(f) == 11 else (f[6], f[8])
            kinds = [P.token_class(L, pm)[0], P.token_class(L, ml)[0]]
            if P.REJECT in kinds or P.DEFER not in kinds:
                continue
            ok = P.host_sites(L, (P.HEADER.encode() + b"\t".join(
                f[:8] + [b"0.5", f[9], b"0.5"] if len(f) == 11 else f[:6] + [b"0.5", f[7], b"0.5"] + f[9:]) + b"\n"))[0]
            if len(ok["line"]) == 1:
                want.add(li)
        assert set((np.flatnonzero(cls == P.DEFER) + 1).tolist()) == want and len(want) > 30
        # the status flag marks the sites whose status byte is none of M, I, U
        flagged = sites["line"][sites["status_flag"] == 1]
        assert len(flagged) >= 6
        for li in flagged:
            b, n = spans[li]
            f = t[b:b + n].split(b"\t")
            assert (f[9] if len(f) == 11 else f[7])[:1] not in (b"M", b"I", b"U")


def test_generated_plain_lines_are_never_deferred():
    """the condition of the issue: at most 15 significant digits and no exponent -> zero lines deferred"""
    L = P.hostlib()
    text = P.plain_text(3000, seed=11)
    cls, sites, host = check_classifier_against_host(L, text)
    assert int((cls == P.DEFER).sum()) == 0 and len(sites["line"]) == len(host["line"]) > 300


def test_shared_parser_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): corrupted lines of every format, each in a heap block of
    exactly its length, through abn_parse_line and parse_site_full, built with -fsanitize=address,undefined."""
    import shutil
    import subprocess

    import pytest

    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path / "parse_lines_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-pthread", "-I", str(P.ROOT / "include"), "-o", str(exe),
                        str(P.ROOT / "tests" / "native" / "parse_lines_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sanitized parse ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
