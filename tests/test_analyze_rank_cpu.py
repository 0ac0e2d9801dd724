"""The key and rank arithmetic of the device analysis (csrc/abn_analyze_rank.hpp; RawAnalysis::analyze,
src/analysis.rs:50-98) on the CPU, as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer — nothing
is loaded into python —, and what the analysis entries answer without a device: abn_analyze's NaN test and the argument
checks of the batched entries."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "alphabeta_rs_amd" / "csrc"
OK, INVALID, NO_FINITE_FIT = 0, 1, 5

_MAIN = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "abn_analyze_rank.hpp"

static unsigned long long state = 88172645463325252ull;
static unsigned long long rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static unsigned long long bits(double x) { unsigned long long u; std::memcpy(&u, &x, 8); return u; }

// ---- (1) key order == `<`; -0.0 and +0.0 distinct and adjacent; key -> double round-trips
static int key_order() {
  const double inf = std::numeric_limits<double>::infinity(), sub = std::numeric_limits<double>::denorm_min();
  std::vector<double> v = {0.0, -0.0, sub, -sub, 1e-310, -1e-310, 2.2250738585072009e-308, -2.2250738585072009e-308,
                           1e-300, -1e-300, 1.0, -1.0, inf, -inf, std::numeric_limits<double>::max(),
                           -std::numeric_limits<double>::max(), std::nextafter(1.0, 2.0), std::nextafter(-1.0, -2.0)};
  while (v.size() < 400) {
    double x;
    const unsigned long long u = rnd() ^ (rnd() << 32);
    std::memcpy(&x, &u, 8);
    if (x == x) v.push_back(x);  // every exponent, both signs; no NaN
  }
  for (double a : v) {
    CHECK(bits(abn::abn_order_key_value(abn::abn_order_key(a))) == bits(a));
    for (double b : v) {
      const unsigned long long ka = abn::abn_order_key(a), kb = abn::abn_order_key(b);
      if (a < b) CHECK(ka < kb);
      if (a > b) CHECK(ka > kb);
      if (a == b) CHECK((ka == kb) == (bits(a) == bits(b)));  // only the two zeros are equal with other bits
    }
  }
  CHECK(abn::abn_order_key(-0.0) + 1 == abn::abn_order_key(0.0));
  CHECK(abn::abn_order_key(-sub) + 1 == abn::abn_order_key(-0.0) && abn::abn_order_key(0.0) + 1 == abn::abn_order_key(sub));
  CHECK(abn::abn_order_key(-inf) < abn::abn_order_key(-std::numeric_limits<double>::max()));
  CHECK(abn::abn_order_key(inf) > abn::abn_order_key(std::numeric_limits<double>::max()));
  return 0;
}

// ---- (2) lo / hi / frac == the formula of abn_analyze (csrc/abn_analyze.hip), written out again here
static int quantile_formula() {
  std::vector<long long> Bs;
  for (long long B = 1; B <= 300; ++B) Bs.push_back(B);
  for (long long B : {1000ll, 5000ll, 10000ll, 65537ll}) Bs.push_back(B);
  for (long long Bll : Bs) {
    const size_t B = (size_t)Bll;
    const double qs[2] = {0.025, 0.975};
    for (int q = 0; q < 2; ++q) {
      const double fi = qs[q] * (double)(B - 1);
      const size_t lo = (size_t)std::floor(fi), hi = (size_t)std::ceil(fi);
      const double frac = fi - std::trunc(fi);
      const abn::QuantileRank r = abn::abn_quantile_rank(abn::abn_analyze_quantile(q), Bll);
      CHECK((size_t)r.lo == lo && (size_t)r.hi == hi && bits(r.frac) == bits(frac));
      CHECK(r.lo >= 0 && r.hi < Bll && (r.hi == r.lo || r.hi == r.lo + 1));
    }
  }
  const abn::QuantileRank r41 = abn::abn_quantile_rank(0.025, 41);  // 0.025 * 40 is integral
  CHECK(r41.lo == 1 && r41.hi == 1 && r41.frac == 0.0);
  for (int k = 0; k < 8; ++k) {
    static const int src_col[8] = {0, 1, -1, 2, 3, 4, 5, 6};
    CHECK(abn::abn_analyze_source_column(k) == src_col[k]);
  }
  return 0;
}

// ---- (3) tied zeros: whatever order a sort with `<` leaves -0.0 and +0.0 in, the interpolated quantile has the same
// bits — so the keys may put -0.0 first.  Every multiset of up to six values from a pool with both zeros, every
// placement of its zeros, every adjacent (lo, hi), several weights.
static int tied_zeros() {
  const double sub = std::numeric_limits<double>::denorm_min();
  const double pool[] = {-1.0, -sub, -0.0, 0.0, sub, 1e-300, 2.0};
  const double fracs[] = {0.0, 0.025, 0.5, 0.975, std::nextafter(1.0, 0.0), sub};
  long long cases = 0;
  for (int n = 2; n <= 6; ++n) {
    std::vector<int> pick((size_t)n, 0);  // non-decreasing indices into the pool: a multiset, already sorted by `<`
    for (;;) {
      std::vector<double> s;
      for (int i : pick) s.push_back(pool[i]);
      const auto z0 = std::find_if(s.begin(), s.end(), [](double x) { return x == 0.0; });
      const auto z1 = std::find_if(z0, s.end(), [](double x) { return x != 0.0; });
      bool neg = false, pos = false;
      for (auto it = z0; it != z1; ++it) (std::signbit(*it) ? neg : pos) = true;
      if (neg && pos) {
        std::vector<double> zeros(z0, z1);
        std::sort(zeros.begin(), zeros.end(), [](double a, double b) { return std::signbit(a) > std::signbit(b); });
        std::vector<std::vector<unsigned long long>> seen;  // per placement: the bits of every (lo, hi, frac)
        do {
          std::vector<double> t = s;
          std::copy(zeros.begin(), zeros.end(), t.begin() + (z0 - s.begin()));
          CHECK(std::is_sorted(t.begin(), t.end()));  // a result std::sort with `<` may return
          std::vector<unsigned long long> got;
          for (int lo = 0; lo < n; ++lo)
            for (int hi = lo; hi <= std::min(lo + 1, n - 1); ++hi)
              for (double f : fracs) got.push_back(bits(abn::abn_quantile_interpolate(t[(size_t)lo], t[(size_t)hi], f)));
          seen.push_back(got);
          ++cases;
        } while (std::next_permutation(zeros.begin(), zeros.end(),
                                       [](double a, double b) { return std::signbit(a) > std::signbit(b); }));
        CHECK(seen.size() >= 2);
        for (const auto& g : seen) CHECK(g == seen[0]);
        // the placement of the keys (-0.0 first) is one of them
        std::vector<double> t = s;
        std::sort(t.begin(), t.end(), [](double a, double b) { return abn::abn_order_key(a) < abn::abn_order_key(b); });
        CHECK(std::is_sorted(t.begin(), t.end()));
      }
      int i = n - 1;
      while (i >= 0 && pick[(size_t)i] == 6) --i;
      if (i < 0) break;
      const int v = pick[(size_t)i] + 1;
      for (int j = i; j < n; ++j) pick[(size_t)j] = v;
    }
  }
  // a zero result is +0.0; by hand: between -0.0 and +0.0 either way round, and both -0.0
  CHECK(bits(abn::abn_quantile_interpolate(-0.0, 0.0, 0.5)) == 0 && bits(abn::abn_quantile_interpolate(0.0, -0.0, 0.5)) == 0);
  CHECK(bits(abn::abn_quantile_interpolate(-0.0, -0.0, 0.0)) == 0);
  std::printf("tied zero placements %lld\n", cases);
  return cases > 1000 ? 0 : 1;
}

static int bad_rows() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double row[7] = {1e-4, 2e-4, 0.5, 0.1, 0.2, 0.3, 0.5};
  CHECK(!abn::abn_analyze_row_is_bad(row));
  for (int k = 0; k < 7; ++k) {
    double r[7];
    std::memcpy(r, row, sizeof r);
    r[k] = nan;
    CHECK(abn::abn_analyze_row_is_bad(r));
    r[k] = k % 2 ? inf : -inf;
    CHECK(!abn::abn_analyze_row_is_bad(r));  // isnan only
  }
  double zz[7] = {0.0, -0.0, 0.5, 0.1, 0.2, 0.3, 0.5};  // 0 / 0
  CHECK(abn::abn_analyze_row_is_bad(zz));
  double ii[7] = {inf, inf, 0.5, 0.1, 0.2, 0.3, 0.5};   // inf / inf
  CHECK(abn::abn_analyze_row_is_bad(ii));
  return 0;
}

int main() {
  if (key_order() || quantile_formula() || tied_zeros() || bad_rows()) return 1;
  std::printf("analyze rank ok\n");
  return 0;
}
"""


def test_keys_ranks_and_tied_zeros_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is a requirement of the CPU tier (the oracle and this program are built with it)"
    main = tmp_path / "rank_main.cpp"
    main.write_text(_MAIN)
    exe = tmp_path / "rank_asan"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", str(CSRC), "-o", str(exe),
                        str(main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "analyze rank ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def _table(B, seed=3):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0.05, 0.95, (B, 7))
    raw[:, 0] = 10.0 ** rng.uniform(-6, -2, B)
    raw[:, 1] = 10.0 ** rng.uniform(-6, -2, B)
    return raw


def _abn_analyze(L, raw, sentinel=-7.0):
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    out = np.full(32, sentinel)
    dp = C.POINTER(C.c_double)
    return L.abn_analyze(raw.ctypes.data_as(dp), raw.shape[0], out.ctypes.data_as(dp)), out


def test_abn_analyze_refuses_nan_tables_itself(abn, oracle):
    """no device needed: the NaN test is inside abn_analyze now (a C caller no longer sorts NaN with `<`)"""
    L = abn.load_library(build_if_missing=True)
    for B in (1, 2, 9, 41, 300):
        raw = _table(B)
        rc, out = _abn_analyze(L, raw)
        assert rc == OK
        want = oracle.analyze(raw).reshape(32)             # a clean table: the bits it always had
        assert np.all((out.view(np.uint64) == want.view(np.uint64)) | (np.isnan(out) & np.isnan(want)))   # B = 1: sd NaN
    raw = _table(40)
    for r, c in ((0, 0), (5, 2), (39, 6)):
        bad = raw.copy()
        bad[r, c] = np.nan
        rc, out = _abn_analyze(L, bad)
        assert rc == NO_FINITE_FIT and np.all(out == -7.0)      # refused, out32 not written
    bad = raw.copy()
    bad[7, 0] = bad[7, 1] = 0.0                                  # alpha = beta = 0: beta / alpha is 0 / 0
    rc, out = _abn_analyze(L, bad)
    assert rc == NO_FINITE_FIT and np.all(out == -7.0)
    inf = raw.copy()
    inf[3, 3] = np.inf                                           # isnan only: +-inf flows through
    rc, out = _abn_analyze(L, inf)
    assert rc == OK and np.isinf(out[4]) and np.isnan(out[8 + 4])


def test_batched_entries_refuse_bad_arguments_without_a_device(abn):
    L = abn.load_library(build_if_missing=True)
    raw, out, fb = _table(4), np.zeros(32), np.zeros(1, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    praw, pout, pfb = raw.ctypes.data_as(dp), out.ctypes.data_as(dp), fb.ctypes.data_as(ip)
    # a null context (all there is without a device), with good and with bad buffers and sizes
    for a_raw, n_boot, a_out in ((praw, 4, pout), (None, 4, pout), (praw, 4, None), (praw, 0, pout), (praw, -3, pout)):
        assert L.abn_analyze_batch(None, a_raw, 1, n_boot, a_out, pfb) == INVALID
    for n_boot in (4, 0, -1):
        assert L.abn_analyze_batch_dev(None, None, 1, n_boot, None, None, None) == INVALID
    assert L.abn_plan_analyze(None, pout, pfb) == INVALID
    assert L.abn_multi_analyze(None, pout, pfb) == INVALID
    assert not out.any() and not fb.any()


def test_binding_lists_the_analysis_entries(abn):
    L = abn.load_library(build_if_missing=True)
    for name in ("abn_analyze_batch", "abn_analyze_batch_dev", "abn_plan_analyze", "abn_multi_analyze"):
        assert name in abn.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    header = (ROOT / "include" / "abneutral.h").read_text()
    for name in ("abn_analyze_batch(", "abn_analyze_batch_dev(", "abn_plan_analyze(", "abn_multi_analyze("):
        assert "int " + name in header
    assert callable(abn.analyze_batch) and hasattr(abn.Context, "analyze_batch_dev")
    assert hasattr(abn.Plan, "analyze") and hasattr(abn.MultiPlan, "analyze")
