"""The C-ABI library loads and exports every symbol include/abneutral.h declares.  No compute calls
(there is no GPU in the CPU test tier and no CPU fallback in the product)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (ROOT / "include" / "abneutral.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(abn_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(abn):
    L = abn.load_library(build_if_missing=True)
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/abneutral.h but not exported"
    assert sorted(abn.EXPORTED_SYMBOLS) == names


SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
ELEMENTS = {**SCALARS, "uint8_t": ctypes.c_uint8}
RETURNS = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p, "int64_t": ctypes.c_int64}


def declarations():
    """[(name, return type, [parameter, ..])] of include/abneutral.h, in its order, as the C text of each piece"""
    text = (ROOT / "include" / "abneutral.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(abn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        out.append((name, " ".join(ret.split()), [] if params == ["void"] else params))
    return out


def check_parameter(c_text, ctype, structs):
    """one parameter's C text against its ctypes type; the reason it does not fit, or None"""
    levels = c_text.count("*") + ("[" in c_text)     # T name[k] is a pointer
    base = re.sub(r"\[.*\]|\*|\bconst\b", " ", c_text).split()[0]
    if levels == 0:
        return None if ctype is SCALARS.get(base, "unknown") else f"scalar {base} is not {ctype}"
    if ctype is ctypes.c_void_p or (ctype is ctypes.c_char_p and base == "char" and levels == 1):
        return None
    if not (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer)):
        return f"pointer is {ctype}"
    if levels == 2:    # T** and T* const*: an array of pointers
        want = ctypes.c_void_p
    elif base in ELEMENTS:
        want = ELEMENTS[base]
    else:              # a struct, by its name: abn_windows_params -> WindowsParams
        want = structs.get("".join(w.capitalize() for w in base.split("_")[1:]))
    return None if want is not None and ctype._type_ is want else f"POINTER({ctype._type_}) for {base}"


def test_prototypes_match_the_header():
    """Every entry of PROTOTYPES against its declaration in include/abneutral.h: one entry per declaration and in its
    order; the arity; the return type; every scalar parameter exactly the ctypes type of its C type; every pointer
    parameter c_void_p, c_char_p (a char*) or a POINTER of the declared element type, structs by name.  ctypes passes an
    int as a 32-bit value where a prototype is missing or short: an int64_t count or an address would lose its top half."""
    from alphabeta_rs_amd import _ffi

    structs = {n: v for n, v in vars(_ffi).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    decls = declarations()
    assert len(decls) >= 150 and sorted(d[0] for d in decls) == declared_symbols()
    assert list(_ffi.PROTOTYPES) == [d[0] for d in decls]
    assert _ffi.EXPORTED_SYMBOLS == list(_ffi.PROTOTYPES)
    wrong = []
    for name, ret, params in decls:
        restype, argtypes = _ffi.PROTOTYPES[name]
        if ret not in RETURNS or restype is not RETURNS[ret]:
            wrong.append(f"{name}: returns {ret}, not {restype}")
        if len(argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} bound")
            continue
        for k, (p, t) in enumerate(zip(params, argtypes)):
            why = check_parameter(p, t, structs)
            if why:
                wrong.append(f"{name} parameter {k} `{p}`: {why}")
    assert not wrong, "\n".join(wrong)
    # and the check refuses what the table must never hold: a narrower scalar, another element type, another struct
    P = ctypes.POINTER
    assert check_parameter("int64_t n", ctypes.c_int32, structs) and check_parameter("uint32_t w", ctypes.c_int32, structs)
    assert check_parameter("const int64_t* begin", P(ctypes.c_int32), structs)
    assert check_parameter("const double params[4]", ctypes.c_double, structs)
    assert check_parameter("const abn_options* opts", P(_ffi.GeneRule), structs)
    assert check_parameter("abn_ctx** ctx", P(ctypes.c_int64), structs) and check_parameter("uint8_t* out", ctypes.c_char_p, structs)
    assert check_parameter("const double params[4]", P(ctypes.c_double), structs) is None
    assert check_parameter("abn_sites* const* samples", P(ctypes.c_void_p), structs) is None
    assert check_parameter("const abn_options* opts", P(_ffi.Options), structs) is None


def test_options_layout_and_defaults(abn):
    o = abn.default_options()
    assert ctypes.sizeof(abn.Options) == 48
    assert o.seed == 20260101 and o.lanes_per_chain == 0 and o.strict_order == 0
    assert o.max_iters_start == 10000 and o.max_iters_boot == 1000   # src/ab_neutral.rs:62, src/boot_model.rs:81
    assert o.sd_tolerance == np.finfo(np.float64).eps
    assert abn.FIT_INFO_DTYPE.itemsize == 24


def test_status_strings(abn):
    L = abn.load_library()
    assert L.abn_status_string(0) == b"ok"
    assert b"pedigree" in L.abn_status_string(2)
    assert L.abn_version() == 1


def test_no_silent_cpu_fallback(abn):
    """Without a device the product refuses to compute (ABN_ERR_NO_DEVICE), it never falls back."""
    if abn.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(abn.AbnError) as e:
        abn.Context(0)
    assert e.value.status == 3


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under alphabeta_rs_amd/ may reference it."""
    for p in (ROOT / "alphabeta_rs_amd").rglob("*"):
        if p.suffix in {".py", ".hip", ".hpp", ".h", ".cpp"}:
            t = p.read_text()
            assert "abn_oracle" not in t and "import oracle" not in t and "from oracle" not in t, p


def test_integration_doc_lists_every_symbol():
    """INTEGRATION.md's `extern "C"` block binds every entry point the header declares (and nothing else)."""
    doc = (ROOT / "INTEGRATION.md").read_text()
    block = doc[doc.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = sorted(set(re.findall(r"pub fn (abn_[a-z0-9_]+)\(", block)))
    assert bound == declared_symbols()


def test_multi_device_entry_refuses_without_a_device(abn):
    """abn_multi_* has no CPU fallback either: without a HIP device creation fails with ABN_ERR_NO_DEVICE; bad arguments
    are status codes; librccl is found (the gather binds it at run time)."""
    assert abn.rccl_available()
    gens = np.array([[0.0, 1.0, 2.0], [0.0, 2.0, 2.0]])
    if abn.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(abn.AbnError) as e:
        abn.MultiPlan([0], gens, 1, 2, 2)
    assert e.value.status == 3
    L = abn.load_library()
    h = ctypes.c_void_p()
    assert L.abn_multi_create(None, 0, None, None, 0, 0, 0, 0, ctypes.byref(h)) == 1 and not h.value
