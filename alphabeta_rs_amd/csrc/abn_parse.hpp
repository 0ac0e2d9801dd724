// The methylome line parser shared by host and device (abn_sites_parse, abn_parse_kernels.hpp): one line, given as a byte
// range, classified exactly as windows::parse_site_full (host/windows_extract.hpp) classifies it — the mirror of
// MethylationSite::from_methylome_file_line (src/methylation_site.rs:146-362, without --invert).  Plain arithmetic on
// registers, no array, no HIP header: the kernel, the host library (host_capi.cpp) and the CPU tests
// (tests/test_parse_cpu.py) all include this file as it is.
// Beside it the arrays the device keeps its records in (ParseRecords, ParseDeferred) and the fields of their `meta` word,
// for everything that reads or writes them: abn_parse_kernels.hpp, abn_sites_merge.hpp, abn_codes.hpp, abn_sites_split.hpp
// and abn_sites.hip.
//
// The one thing the device does not decide in general is str::parse::<f64> (strtod on the host): abn_parse_f64 gives a
// value only where one IEEE operation is certain to give strtod's bits, says "rejected" only where strtod is certain to
// reject, and otherwise DEFERS: the line goes back to the host's parse_site_full.
#pragma once
#include <stdint.h>

#ifndef ABN_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ABN_HOST_DEVICE __host__ __device__
#else
#define ABN_HOST_DEVICE
#endif
#endif

namespace abn {

enum ParseToken : int { kTokValue = 0, kTokReject = 1, kTokDefer = 2 };
enum ParseLine : int { kLineNone = 0, kLineSite = 1, kLineDeferred = 2 };
// A site's methylation context: field 3 of the 9-, 10- and 11-field formats; the 4-field rows have none.  A context MASK
// holds bit 1 << code per accepted context; a row without a context is accepted under every mask.
enum ParseContext : uint32_t { kCtxCG = 0, kCtxCHG = 1, kCtxCHH = 2, kCtxNone = 3 };
constexpr uint32_t kContextsCG = 1u, kContextsAll = 7u;

// field 3 -> its code; kCtxNone: none of CG, CHG, CHH (such a line is no site)
ABN_HOST_DEVICE inline uint32_t abn_parse_context(const unsigned char* p, const unsigned char* e) {
  if (e - p == 2 && p[0] == 'C' && p[1] == 'G') return kCtxCG;
  if (e - p == 3 && p[0] == 'C' && p[1] == 'H' && p[2] == 'G') return kCtxCHG;
  if (e - p == 3 && p[0] == 'C' && p[1] == 'H' && p[2] == 'H') return kCtxCHH;
  return kCtxNone;
}

struct ParsedSite {  // windows::FullSite, and whether status_from would print its warning
  int32_t chromosome;  // Numbered(n) = n, Mitochondrial = 256, Chloroplast = 257
  uint32_t start, end;
  uint32_t strand;       // 0 Sense, 1 Antisense, 2 Unknown
  uint32_t status;       // U = 0, I = 1, M = 2
  uint32_t status_flag;  // 1: the status byte is none of M, I, U (parsed as U, src/methylation_site.rs:107-112)
  double posteriormax, meth_lvl;
  uint32_t context;  // ParseContext
};

// A device record's `meta` word: chromosome | strand << 16 | status << 20 | status_flag << 24 | context << 28 — sixteen
// bits, three fields of four and one of two.  The one writer is meta_pack; every reader takes its field through these.
constexpr int kMetaContextShift = 28;
ABN_HOST_DEVICE inline int32_t meta_chromosome(uint32_t meta) { return (int32_t)(meta & 0xffffu); }
ABN_HOST_DEVICE inline uint32_t meta_strand(uint32_t meta) { return (meta >> 16) & 0xfu; }
ABN_HOST_DEVICE inline uint32_t meta_status(uint32_t meta) { return (meta >> 20) & 0xfu; }
ABN_HOST_DEVICE inline uint32_t meta_status_flag(uint32_t meta) { return (meta >> 24) & 0xfu; }
ABN_HOST_DEVICE inline uint32_t meta_context(uint32_t meta) { return (meta >> kMetaContextShift) & 3u; }
ABN_HOST_DEVICE inline uint32_t meta_pack(const ParsedSite& s) {
  return (uint32_t)s.chromosome | s.strand << 16 | s.status << 20 | s.status_flag << 24 | s.context << kMetaContextShift;
}

// The device's records of one slab (abn_parse_kernels.hpp writes them, abn_sites_split.hpp copies them): struct of arrays,
// one entry per accepted site
struct ParseRecords {
  uint32_t* line;  // the line's index in the slab
  uint32_t* meta;  // (above)
  uint32_t* start;
  uint32_t* end;
  double* posteriormax;
  double* meth_lvl;
};
struct ParseDeferred {  // one entry per deferred line
  uint32_t* line;
  uint32_t* offset;  // the line's first byte in the slab
  uint32_t* length;  // without the line end
};

// str::parse::<u32> (detail::parse_u32): an optional '+', at least one digit, nothing else, at most 4294967295
ABN_HOST_DEVICE inline bool abn_parse_u32(const unsigned char* p, const unsigned char* e, uint32_t& v) {
  if (p == e) return false;
  if (*p == '+') ++p;
  if (p == e) return false;
  uint64_t acc = 0;
  for (; p < e; ++p) {
    const unsigned d = (unsigned)*p - (unsigned)'0';
    if (d > 9u) return false;
    acc = acc * 10u + d;
    if (acc > 0xffffffffull) return false;
  }
  v = (uint32_t)acc;
  return true;
}

// Chromosome::try_from (src/methylation_site.rs:55-68; windows::parse_chromosome_key): every leading "chr" stripped
ABN_HOST_DEVICE inline bool abn_parse_chromosome(const unsigned char* p, const unsigned char* e, int32_t& key) {
  while (e - p >= 3 && p[0] == 'c' && p[1] == 'h' && p[2] == 'r') p += 3;
  if (e - p == 1 && *p == 'M') return key = 256, true;
  if (e - p == 1 && *p == 'C') return key = 257, true;
  uint32_t n;
  if (!abn_parse_u32(p, e, n) || n > 255u) return false;
  return key = (int32_t)n, true;
}

// detail::parse_f64 (strtod, the whole token, no leading white space) where its answer is certain.
//   kTokValue   [sign] digits with at most one '.', at least one digit, [e|E [sign] digits], with at most 19 significant
//               digits (the first non-zero digit to the last digit written), their integer w <= 2^53 and the decimal
//               exponent q = exponent - fraction digits within +-22.  w and 10^|q| are exact doubles then, and the one
//               correctly rounded multiply or divide is the correctly rounded value of the token: strtod's bits.  The
//               sign goes on last (-0.0 keeps it).
//   kTokReject  the empty token, and a token of the bytes 0-9 + - . e E that does not have that shape: strtod consumes a
//               proper prefix of it at most ("1e", "1.2.3", ".", "e5").
//   kTokDefer   everything else: any other byte (inf, nan, 0x.., white space, NUL), 20 or more significant digits,
//               w > 2^53, |q| > 22.
ABN_HOST_DEVICE inline int abn_parse_f64(const unsigned char* p, const unsigned char* e, double& v) {
  if (p == e) return kTokReject;
  for (const unsigned char* s = p; s < e; ++s) {
    const unsigned char c = *s;
    if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return kTokDefer;
  }
  bool neg = false;
  if (*p == '+' || *p == '-') neg = *p == '-', ++p;
  uint64_t w = 0;
  int32_t sig = 0, frac = 0, ex = 0;
  bool any = false, dot = false;
  for (; p < e; ++p) {
    if (*p == '.') {
      if (dot) return kTokReject;
      dot = true;
      continue;
    }
    const unsigned d = (unsigned)*p - (unsigned)'0';
    if (d > 9u) break;
    any = true;
    if (sig > 0 || d > 0) {
      if (sig < 19) w = w * 10u + d;
      if (sig < 1000) ++sig;
    }
    if (dot && frac < 100000) ++frac;
  }
  if (!any) return kTokReject;
  if (p < e) {
    if (*p != 'e' && *p != 'E') return kTokReject;
    ++p;
    bool eneg = false;
    if (p < e && (*p == '+' || *p == '-')) eneg = *p == '-', ++p;
    if (p == e) return kTokReject;
    for (; p < e; ++p) {
      const unsigned d = (unsigned)*p - (unsigned)'0';
      if (d > 9u) return kTokReject;
      if (ex < 100000) ex = ex * 10 + (int32_t)d;
    }
    if (eneg) ex = -ex;
  }
  if (sig > 19 || w > (1ull << 53)) return kTokDefer;
  const int32_t q = ex - frac;
  if (q < -22 || q > 22) return kTokDefer;
  double pw = 1.0;  // 10^|q|: every partial product is an exact double
  for (int32_t i = q < 0 ? -q : q; i > 0; --i) pw = pw * 10.0;
  const double x = q < 0 ? (double)w / pw : (double)w * pw;
  v = neg ? -x : x;
  return kTokValue;
}

// BufRead::lines (windows::lines_of): a '\r' in front of the line's '\n' (or of the end of the text) is not the line's
ABN_HOST_DEVICE inline const unsigned char* abn_line_trim(const unsigned char* b, const unsigned char* e) {
  return (e > b && e[-1] == '\r') ? e - 1 : e;
}

// One line [b, e), already trimmed.  9 or 10 tab fields with field 3 a context of the mask `contexts` (CG alone by
// default): the first and second format; 11: the third (end from field 2, strand from field 5); a context outside the
// mask ends the line as no site before any later field is read, so such a line is never deferred; else exactly 4 fields under a split at tab or space: the chromatin-state /
// bigwig row.  A line of 9 to 11 tab fields has more than 4 fields under the wider split, so the two families never
// compete for a line.  Empty fields count (str::split).  A field the line is certainly rejected for outweighs a
// deferred one: such a line is no site whatever strtod says.
ABN_HOST_DEVICE inline int abn_parse_line(const unsigned char* b, const unsigned char* e, ParsedSite& out,
                                          uint32_t contexts = kContextsCG) {
  int ntab = 0, nsp = 0;
  for (const unsigned char* p = b; p < e; ++p) {
    ntab += *p == '\t' ? 1 : 0;
    nsp += *p == ' ' ? 1 : 0;
  }
  ParsedSite s;
  s.chromosome = 0;
  s.start = s.end = 0;
  s.strand = 2;
  s.status = s.status_flag = 0;
  s.posteriormax = s.meth_lvl = 0.0;
  s.context = kCtxNone;
  if (ntab >= 8 && ntab <= 10) {
    enum { CHROM = 0, START = 1, STRAND = 2, CTX = 3, CM = 4, CT = 5, PM = 6, ST = 7, ML = 8, IGN = 9, END = 10 };
    const bool third = ntab == 10;
    bool reject = false, defer = false, has_end = false;
    const unsigned char* f = b;
    for (int k = 0; k <= ntab; ++k) {
      const unsigned char* fb = f;
      while (f < e && *f != '\t') ++f;
      const unsigned char* fe = f;
      if (f < e) ++f;
      int role = k;
      if (third) role = k < 2 ? k : (k == 2 ? END : (k == 3 ? CTX : (k == 4 ? IGN : (k == 5 ? STRAND : k - 2))));
      uint32_t u;
      switch (role) {
        case CHROM: reject |= !abn_parse_chromosome(fb, fe, s.chromosome); break;
        case START: reject |= !abn_parse_u32(fb, fe, s.start); break;
        case END: reject |= !abn_parse_u32(fb, fe, s.end), has_end = true; break;
        case STRAND: s.strand = (fe - fb == 1 && *fb == '+') ? 0u : 1u; break;
        case CTX:
          s.context = abn_parse_context(fb, fe);
          if (s.context == kCtxNone || !((contexts >> s.context) & 1u)) return kLineNone;
          break;
        case CM:
        case CT: reject |= !abn_parse_u32(fb, fe, u); break;
        case PM:
        case ML: {
          double x = 0.0;
          const int t = abn_parse_f64(fb, fe, x);
          if (role == PM) s.posteriormax = x;
          else s.meth_lvl = x;
          reject |= t == kTokReject;
          defer |= t == kTokDefer;
          break;
        }
        case ST:
          if (fb == fe) {
            reject = true;
          } else {
            s.status = *fb == 'M' ? 2u : (*fb == 'I' ? 1u : 0u);
            s.status_flag = (*fb == 'M' || *fb == 'I' || *fb == 'U') ? 0u : 1u;
          }
          break;
        default: break;
      }
    }
    if (reject) return kLineNone;
    if (defer) return kLineDeferred;
    if (!has_end) s.end = s.start + 1u;  // wrapping, as the release build of the reference
    out = s;
    return kLineSite;
  }
  if (ntab + nsp == 3) {
    bool ok = true;
    const unsigned char* f = b;
    for (int k = 0; k < 3; ++k) {
      const unsigned char* fb = f;
      while (f < e && *f != '\t' && *f != ' ') ++f;
      const unsigned char* fe = f;
      if (f < e) ++f;
      uint32_t u = 0;
      if (k == 0) ok &= abn_parse_chromosome(fb, fe, s.chromosome);
      else ok &= abn_parse_u32(fb, fe, u);
      if (k == 1) s.start = u;
      if (k == 2) s.end = u;
    }
    if (!ok) return kLineNone;
    out = s;
    return kLineSite;
  }
  return kLineNone;
}

}  // namespace abn
