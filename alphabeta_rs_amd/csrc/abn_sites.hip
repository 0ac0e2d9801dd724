// abn_sites_*: methylome text -> site records on the device (src/methylation_site.rs:146-362 for every line of a file,
// the loops of src/windows.rs:303-338 and src/pedigree.rs:138-178 in front of it).  Kernels: abn_parse_kernels.hpp; the
// line parser they share with the host: abn_parse.hpp.  The resident form (abn_sites_parse_dev, abn_sites_insert) keeps the
// records on the device for abn_windows_create_parsed (abn_windows.hip; its merge kernels: abn_sites_merge.hpp) and for
// abn_codes_create_parsed (abn_codes.hip; its reduced merge kernels: abn_codes.hpp).  A handle parsed under a mask of
// several contexts is partitioned into one ordinary resident handle per context by abn_sites_split (its kernels:
// abn_sites_split.hpp).
#include "abn_host.hpp"
#include "abn_parse_kernels.hpp"
#define ABN_SITES_MERGE_KERNELS
#include "abn_sites_merge.hpp"
#define ABN_CODES_MERGE_KERNELS
#include "abn_codes.hpp"
#define ABN_SITES_SPLIT_KERNELS
#include "abn_sites_split.hpp"

using namespace abn;

constexpr int64_t kSitesDefaultSlab = (int64_t)64 << 20, kSitesMaxSlab = (int64_t)1 << 30;

namespace {

struct RecordBufs {
  DevBuf<uint32_t> line, meta, start, end, dline, doffset, dlength;
  DevBuf<double> pm, ml;
  hipError_t alloc(size_t n_rec, size_t n_def) {
    hipError_t e;
    if ((e = line.alloc(n_rec)) || (e = meta.alloc(n_rec)) || (e = start.alloc(n_rec)) || (e = end.alloc(n_rec)) ||
        (e = pm.alloc(n_rec)) || (e = ml.alloc(n_rec)) || (e = dline.alloc(n_def)) || (e = doffset.alloc(n_def)) ||
        (e = dlength.alloc(n_def)))
      return e;
    return hipSuccess;
  }
  ParseRecords records() { return ParseRecords{line.p, meta.p, start.p, end.p, pm.p, ml.p}; }
  ParseDeferred deferred() { return ParseDeferred{dline.p, doffset.p, dlength.p}; }
};

struct SiteChunk {  // a slab's compacted records, resident (abn_sites_parse_dev)
  RecordBufs rec;
  int64_t n = 0, line0 = 0, n_lines = 0, before = 0;
  MergeChunk ref() const {
    return MergeChunk{rec.line.p, rec.meta.p, rec.start.p, rec.end.p, rec.pm.p, rec.ml.p, n, line0, n_lines, before};
  }
};

}  // namespace

// The host form (abn_sites_parse) holds the records in the vectors; the resident form (abn_sites_parse_dev: ctx is set)
// holds them in `chunks` on the device and, after abn_sites_insert, the host-decided records in the same vectors and in
// the i* buffers.  The deferred triples, n_lines and kernel_ms are the same in both.  `context` goes with `line`: the code
// of every record the vectors hold.
struct abn_sites {
  int32_t mask = (int32_t)kContextsCG;  // the contexts the handle was parsed under
  std::vector<uint8_t> context;
  mutable double split_ms[2] = {0.0, 0.0};  // abn_sites_split's count and scatter kernels: on the parent and its children
  std::vector<int64_t> line, dline, doffset, dlength;
  std::vector<int32_t> chromosome;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, status, status_flag;
  std::vector<double> posteriormax, meth_lvl;
  int64_t n_lines = 0;
  double kernel_ms = 0.0;
  // resident form
  abn_ctx* ctx = nullptr;
  int device = -1;
  std::vector<std::unique_ptr<SiteChunk>> chunks;  // one per slab, in file order
  int64_t n_records = 0;                           // over all chunks
  std::vector<int64_t> flagged;                    // the file lines of the records with a status_flag
  bool inserted = false;
  DevBuf<MergeChunk> dchunks;
  DevBuf<long long> iline;
  DevBuf<int32_t> ichunk, ichromosome;
  DevBuf<uint32_t> istart, iend;
  DevBuf<uint8_t> istrand, istatus;
  DevBuf<double> ipm, iml;
};

namespace {

// where the slab that begins at `from` ends: behind the last '\n' of its slab_bytes bytes, or — a line longer than the
// slab — behind that line
size_t slab_end(const char* text, size_t n, size_t from, size_t slab_bytes) {
  if (n - from <= slab_bytes) return n;
  const char* hit = nullptr;
  for (const char* p = text + from + slab_bytes; p > text + from; --p)
    if (p[-1] == '\n') {
      hit = p;
      break;
    }
  if (hit) return (size_t)(hit - text);
  const void* fwd = std::memchr(text + from + slab_bytes, '\n', n - from - slab_bytes);
  return fwd ? (size_t)((const char*)fwd - text) + 1 : n;
}

// one slab [text, text + n): its lines from skip on, appended to h — to its vectors, or (resident) as one more chunk with
// only the deferred triples and the flagged records' lines coming back; line numbers and offsets are the file's
int parse_slab(abn_ctx* c, abn_sites* h, bool resident, const char* text, size_t n, int64_t skip, int64_t line0, int64_t byte0,
               EventPair& ev) {
  const uint32_t n_pieces = (uint32_t)((n + kParsePieceBytes - 1) / kParsePieceBytes);
  const uint32_t n_blocks = (n_pieces + kParseThreads - 1) / kParseThreads;
  DevBuf<uint4> dtext;
  DevBuf<uint32_t> dblock, dbegin, dcount;
  HIPCHK(c, dtext.alloc(n_pieces));
  HIPCHK(c, dblock.alloc((size_t)n_blocks + 1));
  HIPCHK(c, hipMemsetAsync((char*)dtext.p + (size_t)(n_pieces - 1) * kParsePieceBytes, 0, kParsePieceBytes, c->stream));
  HIPCHK(c, hipMemcpyAsync(dtext.p, text, n, hipMemcpyHostToDevice, c->stream));
  auto timed = [&]() {  // behind the kernels of a phase: their time, added to the handle's
    double ms = 0.0;
    const int rc = ev.end(c, &ms);
    h->kernel_ms += ms;
    return rc;
  };
  if (int rc = ev.begin(c, true)) return rc;
  hipLaunchKernelGGL(abn_parse_count_kernel, dim3(n_blocks), dim3(kParseThreads), 0, c->stream, dtext.p, n_pieces, dblock.p);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_parse_scan_kernel, dim3(1), dim3(kParseScanThreads), 0, c->stream, dblock.p, n_blocks, 0u);
  HIPCHK(c, hipGetLastError());
  if (int rc = timed()) return rc;
  uint32_t n_newlines = 0;
  HIPCHK(c, hipMemcpyAsync(&n_newlines, dblock.p + n_blocks, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t n_lines = n_newlines + (text[n - 1] != '\n' ? 1u : 0u);
  h->n_lines += n_lines;
  SiteChunk* chunk = nullptr;
  if (resident) {
    h->chunks.emplace_back(new SiteChunk);
    chunk = h->chunks.back().get();
    chunk->line0 = line0;
    chunk->n_lines = n_lines;
    chunk->before = h->n_records;
  }
  if ((int64_t)n_lines <= skip) return ABN_OK;
  const uint32_t first = (uint32_t)skip, n_runs = (n_lines - first + kParseRun - 1) / kParseRun;
  const uint32_t stride = n_runs + 1;
  RecordBufs run, out;
  HIPCHK(c, dbegin.alloc((size_t)n_newlines + 1));
  HIPCHK(c, dcount.alloc((size_t)2 * stride));
  HIPCHK(c, run.alloc((size_t)n_runs * kParseRun, (size_t)n_runs * kParseRun));
  if (int rc = ev.begin(c, true)) return rc;
  hipLaunchKernelGGL(abn_parse_index_kernel, dim3(n_blocks), dim3(kParseThreads), 0, c->stream, dtext.p, n_pieces,
                     dblock.p, dbegin.p);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_parse_lines_kernel, dim3(n_runs), dim3(kParseThreads), 0, c->stream, dtext.p, (uint32_t)n,
                     dbegin.p, n_newlines, n_lines, first, (uint32_t)h->mask, run.records(), run.deferred(), dcount.p, stride);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_parse_scan_kernel, dim3(2), dim3(kParseScanThreads), 0, c->stream, dcount.p, n_runs, stride);
  HIPCHK(c, hipGetLastError());
  if (int rc = timed()) return rc;
  uint32_t n_rec = 0, n_def = 0;
  HIPCHK(c, hipMemcpyAsync(&n_rec, dcount.p + n_runs, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&n_def, dcount.p + stride + n_runs, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_rec == 0 && n_def == 0) return ABN_OK;
  RecordBufs& rec = resident ? chunk->rec : out;  // the records stay with the handle; the deferred triples never do
  if (resident) HIPCHK(c, rec.alloc(n_rec, 0));
  HIPCHK(c, out.alloc(resident ? 0 : n_rec, n_def));
  const uint32_t flag_blocks =
      resident ? (uint32_t)std::min<size_t>(kMergeFlagBlocks, ((size_t)n_rec + kMergeThreads - 1) / kMergeThreads) : 0u;
  DevBuf<uint32_t> dflagged;
  HIPCHK(c, dflagged.alloc(flag_blocks));
  if (int rc = ev.begin(c, true)) return rc;
  hipLaunchKernelGGL(abn_parse_compact_kernel, dim3(n_runs), dim3(kParseThreads), 0, c->stream, run.records(),
                     run.deferred(), dcount.p, stride, rec.records(), out.deferred());
  HIPCHK(c, hipGetLastError());
  if (flag_blocks) {
    hipLaunchKernelGGL(abn_sites_flagged_kernel, dim3(flag_blocks), dim3(kMergeThreads), 0, c->stream, rec.meta.p,
                       (long long)n_rec, dflagged.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = timed()) return rc;
  std::vector<uint32_t> dline(n_def), doff(n_def), dlen(n_def);
  const size_t dat = h->dline.size();
  auto take_deferred = [&]() {
    h->dline.resize(dat + n_def);
    h->doffset.resize(dat + n_def);
    h->dlength.resize(dat + n_def);
    for (size_t i = 0; i < n_def; ++i) {
      h->dline[dat + i] = line0 + (int64_t)dline[i];
      h->doffset[dat + i] = byte0 + (int64_t)doff[i];
      h->dlength[dat + i] = (int64_t)dlen[i];
    }
  };
  if (resident) {
    std::vector<uint32_t> partial(flag_blocks);
    if (flag_blocks)
      HIPCHK(c, hipMemcpyAsync(partial.data(), dflagged.p, dflagged.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (n_def) {
      HIPCHK(c, hipMemcpyAsync(dline.data(), out.dline.p, 4 * (size_t)n_def, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(doff.data(), out.doffset.p, 4 * (size_t)n_def, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(dlen.data(), out.dlength.p, 4 * (size_t)n_def, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    chunk->n = n_rec;
    h->n_records += n_rec;
    take_deferred();
    uint64_t n_flagged = 0;
    for (uint32_t v : partial) n_flagged += v;
    if (n_flagged) {  // rare: the warning of src/methylation_site.rs:107-112 names these lines
      std::vector<uint32_t> line(n_rec), meta(n_rec);
      HIPCHK(c, hipMemcpyAsync(line.data(), rec.line.p, 4 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(meta.data(), rec.meta.p, 4 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (size_t i = 0; i < n_rec; ++i)
        if ((meta[i] >> 24) & 0xfu) h->flagged.push_back(line0 + (int64_t)line[i]);
    }
    return ABN_OK;
  }
  std::vector<uint32_t> line(n_rec), meta(n_rec), start(n_rec), end(n_rec);
  const size_t at = h->line.size();
  h->posteriormax.resize(at + n_rec);
  h->meth_lvl.resize(at + n_rec);
  if (n_rec) {
    HIPCHK(c, hipMemcpyAsync(line.data(), out.line.p, 4 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(meta.data(), out.meta.p, 4 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(start.data(), out.start.p, 4 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(end.data(), out.end.p, 4 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->posteriormax.data() + at, out.pm.p, 8 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->meth_lvl.data() + at, out.ml.p, 8 * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
  }
  if (n_def) {
    HIPCHK(c, hipMemcpyAsync(dline.data(), out.dline.p, 4 * (size_t)n_def, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(doff.data(), out.doffset.p, 4 * (size_t)n_def, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dlen.data(), out.dlength.p, 4 * (size_t)n_def, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h->line.resize(at + n_rec);
  h->chromosome.resize(at + n_rec);
  h->start.insert(h->start.end(), start.begin(), start.end());
  h->end.insert(h->end.end(), end.begin(), end.end());
  h->strand.resize(at + n_rec);
  h->status.resize(at + n_rec);
  h->status_flag.resize(at + n_rec);
  h->context.resize(at + n_rec);
  for (size_t i = 0; i < n_rec; ++i) {
    const uint32_t m = meta[i];
    h->line[at + i] = line0 + (int64_t)line[i];
    h->chromosome[at + i] = (int32_t)(m & 0xffffu);
    h->strand[at + i] = (uint8_t)((m >> 16) & 0xfu);
    h->status[at + i] = (uint8_t)((m >> 20) & 0xfu);
    h->status_flag[at + i] = (uint8_t)((m >> 24) & 0xfu);
    h->context[at + i] = (uint8_t)meta_context(m);
  }
  take_deferred();
  return ABN_OK;
}

// abn_sites_parse and abn_sites_parse_dev: the checks, the slabs
int sites_parse(abn_ctx* c, const char* text, int64_t n_bytes, const abn_sites_params* params, bool resident,
                abn_sites** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!out || n_bytes < 0 || (n_bytes > 0 && !text)) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  int64_t slab = params ? params->slab_bytes : 0, skip = params ? params->skip_lines : 1;
  if (slab < 0 || slab > kSitesMaxSlab || skip < 0) return set_err(c, ABN_ERR_INVALID_ARG, "slab_bytes / skip_lines");
  if (slab == 0) slab = kSitesDefaultSlab;
  const int32_t contexts = params ? params->contexts : 0;
  if (contexts < 0 || contexts > (int32_t)kContextsAll) return set_err(c, ABN_ERR_INVALID_ARG, "contexts outside 0..7");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  std::unique_ptr<abn_sites> h(new (std::nothrow) abn_sites);
  if (!h) return set_err(c, ABN_ERR_HIP, "out of host memory");
  if (resident) h->ctx = c, h->device = c->device;
  h->mask = contexts == 0 ? (int32_t)kContextsCG : contexts;
  EventPair ev;
  try {
    const size_t n = (size_t)n_bytes;
    for (size_t from = 0; from < n;) {
      const size_t to = slab_end(text, n, from, (size_t)slab);
      if (to - from > (size_t)kSitesMaxSlab + (size_t)kSitesMaxSlab)
        return set_err(c, ABN_ERR_INVALID_ARG, "a line of more than 2 GiB");
      const int64_t before = h->n_lines;
      if (int rc = parse_slab(c, h.get(), resident, text + from, to - from, skip, before, (int64_t)from, ev)) return rc;
      skip = std::max<int64_t>(0, skip - (h->n_lines - before));
      from = to;
    }
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  *out = h.release();
  return ABN_OK;
}

}  // namespace

extern "C" int abn_sites_parse(abn_ctx* c, const char* text, int64_t n_bytes, const abn_sites_params* params,
                               abn_sites** out) {
  return sites_parse(c, text, n_bytes, params, false, out);
}

extern "C" int abn_sites_parse_dev(abn_ctx* c, const char* text, int64_t n_bytes, const abn_sites_params* params,
                                   abn_sites** out) {
  return sites_parse(c, text, n_bytes, params, true, out);
}

extern "C" int abn_sites_destroy(abn_sites* h) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (h->ctx) (void)hipSetDevice(h->device);
  delete h;
  return ABN_OK;
}

extern "C" int abn_sites_info(const abn_sites* h, int64_t* n_sites, int64_t* n_deferred, int64_t* n_lines,
                              double* kernel_ms) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_sites) *n_sites = h->n_records + (int64_t)h->line.size();  // (one of the two is 0 until abn_sites_insert)
  if (n_deferred) *n_deferred = (int64_t)h->dline.size();
  if (n_lines) *n_lines = h->n_lines;
  if (kernel_ms) *kernel_ms = h->kernel_ms;
  return ABN_OK;
}

// abn_sites_fetch of a resident handle: every chunk's records come down and are merged by line with the inserted ones
static int sites_fetch_resident(const abn_sites* h, int64_t* line, int32_t* chromosome, uint32_t* start, uint32_t* end,
                                uint8_t* strand, double* posteriormax, uint8_t* status, uint8_t* status_flag,
                                double* meth_lvl, uint8_t* context) {
  abn_ctx* c = h->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  try {
    size_t j = 0, k = 0;  // the next inserted record, the next place
    const size_t n_ins = h->line.size();
    auto put_inserted = [&]() {
      if (line) line[k] = h->line[j];
      if (chromosome) chromosome[k] = h->chromosome[j];
      if (start) start[k] = h->start[j];
      if (end) end[k] = h->end[j];
      if (strand) strand[k] = h->strand[j];
      if (posteriormax) posteriormax[k] = h->posteriormax[j];
      if (status) status[k] = h->status[j];
      if (status_flag) status_flag[k] = 0;
      if (meth_lvl) meth_lvl[k] = h->meth_lvl[j];
      if (context) context[k] = h->context[j];
      ++j, ++k;
    };
    for (const auto& chunk : h->chunks) {
      const size_t n = (size_t)chunk->n;
      if (n == 0) continue;
      std::vector<uint32_t> l(n), m(n), s(n), e(n);
      std::vector<double> pm(n), ml(n);
      const RecordBufs& r = chunk->rec;
      HIPCHK(c, hipMemcpyAsync(l.data(), r.line.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(m.data(), r.meta.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
      if (start) HIPCHK(c, hipMemcpyAsync(s.data(), r.start.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
      if (end) HIPCHK(c, hipMemcpyAsync(e.data(), r.end.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
      if (posteriormax) HIPCHK(c, hipMemcpyAsync(pm.data(), r.pm.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
      if (meth_lvl) HIPCHK(c, hipMemcpyAsync(ml.data(), r.ml.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (size_t i = 0; i < n; ++i) {
        const int64_t li = chunk->line0 + (int64_t)l[i];
        while (j < n_ins && h->line[j] < li) put_inserted();
        if (line) line[k] = li;
        if (chromosome) chromosome[k] = (int32_t)(m[i] & 0xffffu);
        if (start) start[k] = s[i];
        if (end) end[k] = e[i];
        if (strand) strand[k] = (uint8_t)((m[i] >> 16) & 0xfu);
        if (posteriormax) posteriormax[k] = pm[i];
        if (status) status[k] = (uint8_t)((m[i] >> 20) & 0xfu);
        if (status_flag) status_flag[k] = (uint8_t)((m[i] >> 24) & 0xfu);
        if (meth_lvl) meth_lvl[k] = ml[i];
        if (context) context[k] = (uint8_t)meta_context(m[i]);
        ++k;
      }
    }
    while (j < n_ins) put_inserted();
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_sites_fetch(const abn_sites* h, int64_t* line, int32_t* chromosome, uint32_t* start, uint32_t* end,
                               uint8_t* strand, double* posteriormax, uint8_t* status, uint8_t* status_flag,
                               double* meth_lvl) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (h->ctx)
    return sites_fetch_resident(h, line, chromosome, start, end, strand, posteriormax, status, status_flag, meth_lvl, nullptr);
  if (line) std::copy(h->line.begin(), h->line.end(), line);
  if (chromosome) std::copy(h->chromosome.begin(), h->chromosome.end(), chromosome);
  if (start) std::copy(h->start.begin(), h->start.end(), start);
  if (end) std::copy(h->end.begin(), h->end.end(), end);
  if (strand) std::copy(h->strand.begin(), h->strand.end(), strand);
  if (posteriormax) std::copy(h->posteriormax.begin(), h->posteriormax.end(), posteriormax);
  if (status) std::copy(h->status.begin(), h->status.end(), status);
  if (status_flag) std::copy(h->status_flag.begin(), h->status_flag.end(), status_flag);
  if (meth_lvl) std::copy(h->meth_lvl.begin(), h->meth_lvl.end(), meth_lvl);
  return ABN_OK;
}

extern "C" int abn_sites_context(const abn_sites* h, int32_t* mask, uint8_t* context) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (mask) *mask = h->mask;
  if (!context) return ABN_OK;
  if (h->ctx)
    return sites_fetch_resident(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, context);
  std::copy(h->context.begin(), h->context.end(), context);
  return ABN_OK;
}

extern "C" int abn_sites_deferred(const abn_sites* h, int64_t* line, int64_t* offset, int64_t* length) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (line) std::copy(h->dline.begin(), h->dline.end(), line);
  if (offset) std::copy(h->doffset.begin(), h->doffset.end(), offset);
  if (length) std::copy(h->dlength.begin(), h->dlength.end(), length);
  return ABN_OK;
}

extern "C" int abn_sites_flagged(const abn_sites* h, int64_t* n, int64_t* line) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (!h->ctx) {  // the host form has the flags themselves
    int64_t k = 0;
    for (size_t i = 0; i < h->line.size(); ++i)
      if (h->status_flag[i]) {
        if (line) line[k] = h->line[i];
        ++k;
      }
    if (n) *n = k;
    return ABN_OK;
  }
  if (n) *n = (int64_t)h->flagged.size();
  if (line) std::copy(h->flagged.begin(), h->flagged.end(), line);
  return ABN_OK;
}

// abn_sites_insert_ctx (context null: every code is 0), and how a child of abn_sites_split gets its share of the parent's
// inserted records (inherited: it has no deferred lines to look the lines up in)
static int sites_insert(abn_sites* h, int64_t n, const int64_t* line, const int32_t* chromosome, const uint32_t* start,
                        const uint32_t* end, const uint8_t* strand, const double* posteriormax, const uint8_t* status,
                        const double* meth_lvl, const uint8_t* context, bool inherited) {
  if (!h || !h->ctx) return ABN_ERR_INVALID_ARG;  // (a host-form handle has no context to report to)
  abn_ctx* c = h->ctx;
  if (h->inserted) return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_insert was already called on this handle");
  if (n < 0 || (n > 0 && (!line || !chromosome || !start || !end || !strand || !posteriormax || !status || !meth_lvl)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  try {
    const size_t N = (size_t)n;
    size_t d = 0;  // both lists ascend: every line is looked for behind the one before
    for (size_t j = 0; j < N; ++j) {
      if (j > 0 && line[j] <= line[j - 1]) return set_err(c, ABN_ERR_INVALID_ARG, "the lines are not strictly ascending");
      while (d < h->dline.size() && h->dline[d] < line[j]) ++d;
      if (!inherited && (d == h->dline.size() || h->dline[d] != line[j]))
        return set_err(c, ABN_ERR_INVALID_ARG, "a line that was not deferred");
      if (chromosome[j] < 0 || chromosome[j] > 257) return set_err(c, ABN_ERR_INVALID_ARG, "a chromosome outside 0..257");
      if (strand[j] > 2 || status[j] > 2) return set_err(c, ABN_ERR_INVALID_ARG, "a strand or a status above 2");
      const uint32_t code = context ? context[j] : (uint32_t)kCtxCG;
      if (code > kCtxNone || (code < kCtxNone && !(((uint32_t)h->mask >> code) & 1u)))
        return set_err(c, ABN_ERR_INVALID_ARG, "a context code above 3 or outside the handle's contexts");
    }
    if (N > 0) {
      std::vector<MergeChunk> refs;
      for (const auto& chunk : h->chunks) refs.push_back(chunk->ref());
      std::vector<long long> l(line, line + N);
      std::vector<int32_t> pick(N);
      if (!merge_pick_chunks(refs.data(), (int)refs.size(), l.data(), (long long)N, pick.data()))
        return set_err(c, ABN_ERR_INVALID_ARG, "a line outside every slab");
      HIPCHK(c, hipSetDevice(c->device));
      PoolScope pool_scope(c);
      HIPCHK(c, h->dchunks.alloc(refs.size()));
      HIPCHK(c, h->iline.alloc(N));
      HIPCHK(c, h->ichunk.alloc(N));
      HIPCHK(c, h->ichromosome.alloc(N));
      HIPCHK(c, h->istart.alloc(N));
      HIPCHK(c, h->iend.alloc(N));
      HIPCHK(c, h->istrand.alloc(N));
      HIPCHK(c, h->istatus.alloc(N));
      HIPCHK(c, h->ipm.alloc(N));
      HIPCHK(c, h->iml.alloc(N));
      HIPCHK(c, hipMemcpyAsync(h->dchunks.p, refs.data(), h->dchunks.bytes(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->iline.p, l.data(), 8 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->ichunk.p, pick.data(), 4 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->ichromosome.p, chromosome, 4 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->istart.p, start, 4 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->iend.p, end, 4 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->istrand.p, strand, N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->istatus.p, status, N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->ipm.p, posteriormax, 8 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(h->iml.p, meth_lvl, 8 * N, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staging vectors go on return
      h->line.assign(line, line + N);  // the host's copy, for abn_sites_fetch
      h->chromosome.assign(chromosome, chromosome + N);
      h->start.assign(start, start + N);
      h->end.assign(end, end + N);
      h->strand.assign(strand, strand + N);
      h->posteriormax.assign(posteriormax, posteriormax + N);
      h->status.assign(status, status + N);
      h->meth_lvl.assign(meth_lvl, meth_lvl + N);
      if (context) h->context.assign(context, context + N);
      else h->context.assign(N, (uint8_t)kCtxCG);
    }
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  h->inserted = true;
  return ABN_OK;
}

extern "C" int abn_sites_insert_ctx(abn_sites* h, int64_t n, const int64_t* line, const int32_t* chromosome,
                                    const uint32_t* start, const uint32_t* end, const uint8_t* strand,
                                    const double* posteriormax, const uint8_t* status, const double* meth_lvl,
                                    const uint8_t* context) {
  if (h && h->ctx && n > 0 && !context) return set_err(h->ctx, ABN_ERR_INVALID_ARG, "null/size");
  return sites_insert(h, n, line, chromosome, start, end, strand, posteriormax, status, meth_lvl, context, false);
}

extern "C" int abn_sites_insert(abn_sites* h, int64_t n, const int64_t* line, const int32_t* chromosome,
                                const uint32_t* start, const uint32_t* end, const uint8_t* strand,
                                const double* posteriormax, const uint8_t* status, const double* meth_lvl) {
  if (h && h->ctx && n > 0 && h->mask != (int32_t)kContextsCG)
    return set_err(h->ctx, ABN_ERR_INVALID_ARG, "the handle holds other contexts than CG: abn_sites_insert_ctx names each record's");
  return sites_insert(h, n, line, chromosome, start, end, strand, posteriormax, status, meth_lvl, nullptr, false);
}

// ---- abn_sites_split
namespace {

// the chunk table on the device: the parent's chunks with their workgroups and (once made) the children's chunks
int upload_split_chunks(abn_ctx* c, const std::vector<SplitChunk>& table, DevBuf<SplitChunk>& d) {
  HIPCHK(c, hipMemcpyAsync(d.p, table.data(), d.bytes(), hipMemcpyHostToDevice, c->stream));
  return ABN_OK;
}

int sites_split(const abn_sites* h, std::unique_ptr<abn_sites>* kids) {
  abn_ctx* c = h->ctx;
  const int n_chunks = (int)h->chunks.size();
  std::vector<SplitChunk> table((size_t)n_chunks);
  std::vector<MergeChunk> refs((size_t)n_chunks);
  long long n_blocks = 0;
  for (int i = 0; i < n_chunks; ++i) {
    refs[(size_t)i] = h->chunks[(size_t)i]->ref();
    table[(size_t)i] = SplitChunk{refs[(size_t)i], n_blocks, {}};
    n_blocks += split_blocks(h->chunks[(size_t)i]->n);
  }
  if (n_blocks >= (long long)1 << 31 || h->n_records >= (int64_t)1 << 32)
    return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_split: 2^32 records or more");
  for (int k = 0; k < kSplitChildren; ++k) {
    if (!((h->mask >> k) & 1)) continue;
    kids[k].reset(new abn_sites);
    kids[k]->ctx = c, kids[k]->device = h->device;
    kids[k]->mask = 1 << k;
    kids[k]->n_lines = h->n_lines;
  }
  const uint32_t stride = (uint32_t)n_blocks + 1u;
  std::vector<uint32_t> size((size_t)n_chunks * kSplitChildren, 0u);
  DevBuf<SplitChunk> dtable;
  DevBuf<uint32_t> dcount, dsize;
  EventPair ev;
  h->split_ms[0] = h->split_ms[1] = 0.0;
  if (n_blocks > 0) {
    HIPCHK(c, dtable.alloc((size_t)n_chunks));
    HIPCHK(c, dcount.alloc((size_t)kSplitChildren * stride));
    HIPCHK(c, dsize.alloc(size.size()));
    if (int rc = upload_split_chunks(c, table, dtable)) return rc;
    if (int rc = ev.begin(c, true)) return rc;
    hipLaunchKernelGGL(abn_split_count_kernel, dim3((unsigned)n_blocks), dim3(kSplitThreads), 0, c->stream,
                       (const SplitChunk*)dtable.p, n_chunks, (uint32_t)h->mask, dcount.p, stride);
    HIPCHK(c, hipGetLastError());
    if (int rc = ev.end(c, &h->split_ms[0])) return rc;
    hipLaunchKernelGGL(abn_parse_scan_kernel, dim3(kSplitChildren), dim3(kParseScanThreads), 0, c->stream, dcount.p,
                       (uint32_t)n_blocks, stride);
    HIPCHK(c, hipGetLastError());
    const unsigned size_grid = (unsigned)((size.size() + kSplitThreads - 1) / kSplitThreads);
    hipLaunchKernelGGL(abn_split_sizes_kernel, dim3(size_grid), dim3(kSplitThreads), 0, c->stream,
                       (const SplitChunk*)dtable.p, n_chunks, (const uint32_t*)dcount.p, stride, (uint32_t)n_blocks, dsize.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(size.data(), dsize.p, dsize.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // the children's chunks: a slab keeps its lines, and holds the child's share of its records
  for (int i = 0; i < n_chunks; ++i)
    for (int k = 0; k < kSplitChildren; ++k) {
      if (!kids[k]) continue;  // (a context outside the mask has no child, and the kernels count no record for it)
      abn_sites* kid = kids[k].get();
      kid->chunks.emplace_back(new SiteChunk);
      SiteChunk* chunk = kid->chunks.back().get();
      chunk->n = size[(size_t)i * kSplitChildren + k];
      chunk->line0 = h->chunks[(size_t)i]->line0;
      chunk->n_lines = h->chunks[(size_t)i]->n_lines;
      chunk->before = kid->n_records;
      kid->n_records += chunk->n;
      HIPCHK(c, chunk->rec.alloc((size_t)chunk->n, 0));
      table[(size_t)i].out[k] = SplitOut{chunk->rec.line.p, chunk->rec.meta.p, chunk->rec.start.p,
                                         chunk->rec.end.p,  chunk->rec.pm.p,   chunk->rec.ml.p};
    }
  for (int i = 0; i < n_chunks; ++i)  // a record counted for a context without a child would have nowhere to go
    for (int k = 0; k < kSplitChildren; ++k)
      if (!kids[k] && size[(size_t)i * kSplitChildren + k] != 0)
        return set_err(c, ABN_ERR_HIP, "abn_sites_split: a record outside the handle's contexts");
  // the flagged lines: which children inherit each, found on the device
  const size_t n_flagged = h->flagged.size();
  std::vector<uint8_t> member(n_flagged, 0);
  DevBuf<long long> dfline;
  DevBuf<int32_t> dfchunk;
  DevBuf<uint8_t> dmember;
  std::vector<long long> fline(h->flagged.begin(), h->flagged.end());
  std::vector<int32_t> fchunk(n_flagged);
  if (n_blocks > 0) {
    if (int rc = upload_split_chunks(c, table, dtable)) return rc;
    if (n_flagged) {
      if (!merge_pick_chunks(refs.data(), n_chunks, fline.data(), (long long)n_flagged, fchunk.data()))
        return set_err(c, ABN_ERR_HIP, "abn_sites_split: a flagged line outside every slab");
      HIPCHK(c, dfline.alloc(n_flagged));
      HIPCHK(c, dfchunk.alloc(n_flagged));
      HIPCHK(c, dmember.alloc(n_flagged));
      HIPCHK(c, hipMemcpyAsync(dfline.p, fline.data(), dfline.bytes(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(dfchunk.p, fchunk.data(), dfchunk.bytes(), hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = ev.begin(c, true)) return rc;
    hipLaunchKernelGGL(abn_split_scatter_kernel, dim3((unsigned)n_blocks), dim3(kSplitThreads), 0, c->stream,
                       (const SplitChunk*)dtable.p, n_chunks, (uint32_t)h->mask, (const uint32_t*)dcount.p, stride);
    HIPCHK(c, hipGetLastError());
    if (int rc = ev.end(c, &h->split_ms[1])) return rc;
    if (n_flagged) {
      const unsigned grid = (unsigned)((n_flagged + kSplitThreads - 1) / kSplitThreads);
      hipLaunchKernelGGL(abn_split_flagged_kernel, dim3(grid), dim3(kSplitThreads), 0, c->stream,
                         (const SplitChunk*)dtable.p, (const long long*)dfline.p, (const int32_t*)dfchunk.p,
                         (long long)n_flagged, (uint32_t)h->mask, dmember.p);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(member.data(), dmember.p, n_flagged, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the tables and staging vectors go on return
  }
  for (int k = 0; k < kSplitChildren; ++k) {
    if (!kids[k]) continue;
    abn_sites* kid = kids[k].get();
    kid->split_ms[0] = h->split_ms[0], kid->split_ms[1] = h->split_ms[1];
    for (size_t j = 0; j < n_flagged; ++j)
      if ((member[j] >> k) & 1u) kid->flagged.push_back(h->flagged[j]);
    // the parent's inserted records of this membership, uploaded as abn_sites_insert uploads them
    std::vector<int64_t> line;
    std::vector<int32_t> chrom;
    std::vector<uint32_t> start, end;
    std::vector<uint8_t> strand, status, context;
    std::vector<double> pm, ml;
    for (size_t j = 0; j < h->line.size(); ++j) {
      const uint32_t code = h->context[j];
      if (code != kCtxNone && code != (uint32_t)k) continue;
      line.push_back(h->line[j]);
      chrom.push_back(h->chromosome[j]);
      start.push_back(h->start[j]);
      end.push_back(h->end[j]);
      strand.push_back(h->strand[j]);
      pm.push_back(h->posteriormax[j]);
      status.push_back(h->status[j]);
      ml.push_back(h->meth_lvl[j]);
      context.push_back((uint8_t)code);
    }
    if (int rc = sites_insert(kid, (int64_t)line.size(), line.data(), chrom.data(), start.data(), end.data(), strand.data(),
                              pm.data(), status.data(), ml.data(), context.data(), true))
      return rc;
  }
  return ABN_OK;
}

}  // namespace

extern "C" int abn_sites_split(const abn_sites* h, abn_sites** out3) {
  if (out3) out3[0] = out3[1] = out3[2] = nullptr;
  if (!h || !h->ctx) return ABN_ERR_INVALID_ARG;  // (a host-form handle has no context to report to)
  abn_ctx* c = h->ctx;
  if (!out3) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (!h->dline.empty() && !h->inserted)
    return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_split: the handle has deferred lines and abn_sites_insert was never called");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  std::unique_ptr<abn_sites> kids[kSplitChildren];
  try {
    if (int rc = sites_split(h, kids)) return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  for (int k = 0; k < kSplitChildren; ++k) out3[k] = kids[k].release();
  return ABN_OK;
}

extern "C" int abn_sites_split_ms(const abn_sites* h, double* ms2) {
  if (!h || !ms2) return ABN_ERR_INVALID_ARG;
  ms2[0] = h->split_ms[0], ms2[1] = h->split_ms[1];
  return ABN_OK;
}

// ---- for abn_windows_create_parsed (abn_windows.hip)
abn_ctx* abn::sites_ctx(const abn_sites* h) { return h ? h->ctx : nullptr; }

int64_t abn::sites_merged_count(const abn_sites* h) {
  if (!h || !h->ctx || (!h->dline.empty() && !h->inserted)) return -1;
  return h->n_records + (int64_t)h->line.size();
}

int abn::sites_merge_dev(const abn_sites* h, bool inserted, double filter, int32_t* dchrom, uint32_t* dstart,
                         uint32_t* dend, uint8_t* dstrand, uint8_t* dcode, double* dlevel) {
  abn_ctx* c = h->ctx;
  const MergeOut out{dchrom, dstart, dend, dstrand, dcode, dlevel};
  const long long n_ins = (long long)h->line.size();
  if (!inserted) {
    for (const auto& chunk : h->chunks) {
      if (chunk->n == 0) continue;
      const unsigned grid = (unsigned)((chunk->n + kMergeThreads - 1) / kMergeThreads);
      hipLaunchKernelGGL(abn_sites_fields_kernel, dim3(grid), dim3(kMergeThreads), 0, c->stream, chunk->ref(),
                         (const long long*)h->iline.p, n_ins, filter, out);
      HIPCHK(c, hipGetLastError());
    }
  } else if (n_ins > 0) {
    const MergeInserted ins{h->iline.p, h->ichunk.p, h->ichromosome.p, h->istart.p, h->iend.p,
                            h->istrand.p, h->istatus.p, h->ipm.p, h->iml.p, n_ins};
    const unsigned grid = (unsigned)((n_ins + kMergeThreads - 1) / kMergeThreads);
    hipLaunchKernelGGL(abn_sites_insert_kernel, dim3(grid), dim3(kMergeThreads), 0, c->stream,
                       (const MergeChunk*)h->dchunks.p, ins, filter, out);
    HIPCHK(c, hipGetLastError());
  }
  return ABN_OK;
}

// ---- for abn_codes_create_parsed (abn_codes.hip): the same launches with the reduced writers of abn_codes.hpp
int abn::sites_merge_codes_dev(const abn_sites* h, bool inserted, double filter, uint8_t* dcode, double* dlevel) {
  abn_ctx* c = h->ctx;
  const CodesOut out{dcode, dlevel};
  const long long n_ins = (long long)h->line.size();
  if (!inserted) {
    for (const auto& chunk : h->chunks) {
      if (chunk->n == 0) continue;
      const unsigned grid = (unsigned)((chunk->n + kMergeThreads - 1) / kMergeThreads);
      hipLaunchKernelGGL(abn_codes_fields_kernel, dim3(grid), dim3(kMergeThreads), 0, c->stream, chunk->ref(),
                         (const long long*)h->iline.p, n_ins, filter, out);
      HIPCHK(c, hipGetLastError());
    }
  } else if (n_ins > 0) {
    const MergeInserted ins{h->iline.p, h->ichunk.p, h->ichromosome.p, h->istart.p, h->iend.p,
                            h->istrand.p, h->istatus.p, h->ipm.p, h->iml.p, n_ins};
    const unsigned grid = (unsigned)((n_ins + kMergeThreads - 1) / kMergeThreads);
    hipLaunchKernelGGL(abn_codes_insert_kernel, dim3(grid), dim3(kMergeThreads), 0, c->stream,
                       (const MergeChunk*)h->dchunks.p, ins, filter, out);
    HIPCHK(c, hipGetLastError());
  }
  return ABN_OK;
}
