// abn_sites_*: methylome text -> site records on the device (src/methylation_site.rs:146-362 for every line of a file,
// the loops of src/windows.rs:303-338 and src/pedigree.rs:138-178 in front of it).  Kernels: abn_parse_kernels.hpp; the
// line parser they share with the host, the device's record arrays and their meta word: abn_parse.hpp.  The resident form
// (abn_sites_parse_dev, abn_sites_insert) keeps the records on the device for abn_windows_create_parsed (abn_windows.hip;
// its merge kernels: abn_sites_merge.hpp) and for abn_codes_create_parsed (abn_codes.hip; its reduced merge kernels:
// abn_codes.hpp).  A handle parsed under a mask of several contexts is partitioned into one ordinary resident handle per
// context by abn_sites_split (its kernels: abn_sites_split.hpp), sorted by genomic position into a new resident handle
// by abn_sites_sort (its kernels: abn_sites_sort.hpp, launched from abn_sites_sort.hip), and its repeated sites collapsed
// into another by abn_sites_dedup (abn_sites_dedup.hpp, abn_sites_dedup.hip).
//
// In this file: a site as the host reports it (SiteRecord, SiteOut, SiteIn, SiteColumns); the records on the device
// (RecordBufs, SiteChunk, InsertedBufs); the handle; the parse; what a handle reports; the insert; the split; the sort and the collapse;
// the merge launches of the builders.
#define ABN_SITES_MERGE_KERNELS  // (in front of abn_host.hpp: it includes abn_sites_merge.hpp through abn_sites_sort.hpp)
#define ABN_CODES_MERGE_KERNELS
#define ABN_SITES_SPLIT_KERNELS
#include "abn_host.hpp"
#include "abn_parse_kernels.hpp"
#include "abn_sites_merge.hpp"
#include "abn_codes.hpp"
#include "abn_sites_split.hpp"

using namespace abn;

constexpr int64_t kSitesDefaultSlab = (int64_t)64 << 20, kSitesMaxSlab = (int64_t)1 << 30;

namespace {

// ---- a site on the host: the ten columns of abn_sites_fetch and abn_sites_context
struct SiteRecord {
  int64_t line;
  int32_t chromosome;
  uint32_t start, end;
  uint8_t strand;
  double posteriormax;
  uint8_t status, status_flag;
  double meth_lvl;
  uint8_t context;
};

// a device record of the slab that begins at file line line0
SiteRecord site_decode(int64_t line0, uint32_t line, uint32_t meta, uint32_t start, uint32_t end, double pm, double ml) {
  return SiteRecord{line0 + (int64_t)line, meta_chromosome(meta), start, end, (uint8_t)meta_strand(meta), pm,
                    (uint8_t)meta_status(meta), (uint8_t)meta_status_flag(meta), ml, (uint8_t)meta_context(meta)};
}

struct SiteOut {  // where a caller wants the columns: null, not wanted
  int64_t* line;
  int32_t* chromosome;
  uint32_t *start, *end;
  uint8_t* strand;
  double* posteriormax;
  uint8_t *status, *status_flag;
  double* meth_lvl;
  uint8_t* context;
  void put(size_t k, const SiteRecord& r) const {
    if (line) line[k] = r.line;
    if (chromosome) chromosome[k] = r.chromosome;
    if (start) start[k] = r.start;
    if (end) end[k] = r.end;
    if (strand) strand[k] = r.strand;
    if (posteriormax) posteriormax[k] = r.posteriormax;
    if (status) status[k] = r.status;
    if (status_flag) status_flag[k] = r.status_flag;
    if (meth_lvl) meth_lvl[k] = r.meth_lvl;
    if (context) context[k] = r.context;
  }
};

struct SiteIn {  // host-decided records: what abn_sites_insert is given (context null: every code is CG) and keeps
  const int64_t* line;
  const int32_t* chromosome;
  const uint32_t *start, *end;
  const uint8_t* strand;
  const double* posteriormax;
  const uint8_t* status;
  const double* meth_lvl;
  const uint8_t* context;
  bool complete() const { return line && chromosome && start && end && strand && posteriormax && status && meth_lvl; }
  SiteRecord at(size_t j) const {  // (such a line has no status_flag: the host's parser printed its warning)
    return SiteRecord{line[j], chromosome[j], start[j], end[j], strand[j], posteriormax[j], status[j], 0, meth_lvl[j],
                      (uint8_t)(context ? context[j] : kCtxCG)};
  }
};

struct SiteColumns {  // the records a handle holds on the host
  std::vector<int64_t> line;
  std::vector<int32_t> chromosome;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, status, status_flag, context;
  std::vector<double> posteriormax, meth_lvl;
  size_t size() const { return line.size(); }
  void resize(size_t n) {
    line.resize(n), chromosome.resize(n), start.resize(n), end.resize(n), strand.resize(n), posteriormax.resize(n);
    status.resize(n), status_flag.resize(n), meth_lvl.resize(n), context.resize(n);
  }
  SiteOut view() {
    return SiteOut{line.data(), chromosome.data(), start.data(), end.data(), strand.data(), posteriormax.data(),
                   status.data(), status_flag.data(), meth_lvl.data(), context.data()};
  }
  SiteIn in() const {  // (a resident handle's: the inserted records)
    return SiteIn{line.data(), chromosome.data(), start.data(), end.data(), strand.data(), posteriormax.data(),
                  status.data(), meth_lvl.data(), context.data()};
  }
  // Records at .. at + n of the slab that begins at file line line0, from their line and meta words; start, end and the
  // two floats come down from the device into place.  Plain column stores: the time of abn_sites_parse rests on this loop
  void decode(size_t at, size_t n, int64_t line0, const uint32_t* l, const uint32_t* m) {
    for (size_t i = 0, k = at; i < n; ++i, ++k) {
      line[k] = line0 + (int64_t)l[i];
      chromosome[k] = meta_chromosome(m[i]);
      strand[k] = (uint8_t)meta_strand(m[i]);
      status[k] = (uint8_t)meta_status(m[i]);
      status_flag[k] = (uint8_t)meta_status_flag(m[i]);
      context[k] = (uint8_t)meta_context(m[i]);
    }
  }
  void push(const SiteRecord& r) {
    resize(size() + 1);
    view().put(size() - 1, r);
  }
  void copy_to(const SiteOut& o) const {  // column by column
    if (o.line) std::copy(line.begin(), line.end(), o.line);
    if (o.chromosome) std::copy(chromosome.begin(), chromosome.end(), o.chromosome);
    if (o.start) std::copy(start.begin(), start.end(), o.start);
    if (o.end) std::copy(end.begin(), end.end(), o.end);
    if (o.strand) std::copy(strand.begin(), strand.end(), o.strand);
    if (o.posteriormax) std::copy(posteriormax.begin(), posteriormax.end(), o.posteriormax);
    if (o.status) std::copy(status.begin(), status.end(), o.status);
    if (o.status_flag) std::copy(status_flag.begin(), status_flag.end(), o.status_flag);
    if (o.meth_lvl) std::copy(meth_lvl.begin(), meth_lvl.end(), o.meth_lvl);
    if (o.context) std::copy(context.begin(), context.end(), o.context);
  }
};

// ---- the records on the device
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
  ParseRecords records() const { return ParseRecords{line.p, meta.p, start.p, end.p, pm.p, ml.p}; }
  ParseDeferred deferred() const { return ParseDeferred{dline.p, doffset.p, dlength.p}; }
};

struct SiteChunk {  // a slab's compacted records, resident (abn_sites_parse_dev)
  RecordBufs rec;
  int64_t n = 0, line0 = 0, n_lines = 0, before = 0;
  MergeChunk ref() const {
    return MergeChunk{rec.line.p, rec.meta.p, rec.start.p, rec.end.p, rec.pm.p, rec.ml.p, n, line0, n_lines, before};
  }
};

struct InsertedBufs {  // the host-decided records (abn_sites_insert), with the chunk table their merge kernel reads
  DevBuf<MergeChunk> chunks;
  DevBuf<long long> line;
  DevBuf<int32_t> chunk, chromosome;
  DevBuf<uint32_t> start, end;
  DevBuf<uint8_t> strand, status;
  DevBuf<double> pm, ml;
  // line: in.line as the kernels read it; pick: the chunk of every line; refs: the handle's chunks.  Nothing waited for
  int upload(abn_ctx* c, const SiteIn& in, const std::vector<long long>& l, const std::vector<int32_t>& pick,
             const std::vector<MergeChunk>& refs) {
    const size_t n = l.size();
    int rc;
    if ((rc = abn::upload(c, chunks, refs.data(), refs.size())) || (rc = abn::upload(c, line, l.data(), n)) ||
        (rc = abn::upload(c, chunk, pick.data(), n)) || (rc = abn::upload(c, chromosome, in.chromosome, n)) ||
        (rc = abn::upload(c, start, in.start, n)) || (rc = abn::upload(c, end, in.end, n)) ||
        (rc = abn::upload(c, strand, in.strand, n)) || (rc = abn::upload(c, status, in.status, n)) ||
        (rc = abn::upload(c, pm, in.posteriormax, n)) || (rc = abn::upload(c, ml, in.meth_lvl, n)))
      return rc;
    return ABN_OK;
  }
  MergeInserted ref() const {
    return MergeInserted{line.p, chunk.p, chromosome.p, start.p, end.p, strand.p, status.p, pm.p, ml.p, (long long)line.n};
  }
};

}  // namespace

// The host form (abn_sites_parse) holds the records in `cols`; the resident form (abn_sites_parse_dev: ctx is set) holds
// them in `chunks` on the device and, after abn_sites_insert, the host-decided records in `cols` and in `ins`.  The
// deferred triples, n_lines and kernel_ms are the same in both.
struct abn_sites {
  int32_t mask = (int32_t)kContextsCG;  // the contexts the handle was parsed under
  mutable double split_ms[2] = {0.0, 0.0};  // abn_sites_split's count and scatter kernels: on the parent and its children
  SiteColumns cols;
  std::vector<int64_t> dline, doffset, dlength;
  int64_t n_lines = 0;
  double kernel_ms = 0.0;
  // resident form
  abn_ctx* ctx = nullptr;
  int device = -1;
  std::vector<std::unique_ptr<SiteChunk>> chunks;  // one per slab, in file order
  int64_t n_records = 0;                           // over all chunks
  std::vector<int64_t> flagged;                    // the file lines of the records with a status_flag
  bool inserted = false;
  InsertedBufs ins;
  // a handle abn_sites_sort made: order[k] = the parent's site at its place k; {sites, descents, equal neighbours, passes};
  // the HIP-event ms of flatten, check, passes, gather
  bool sorted = false;
  DevBuf<uint32_t> sort_order;
  int64_t sort_info[4] = {0, 0, 0, 0};
  double sort_ms[4] = {0.0, 0.0, 0.0, 0.0};
  // a handle abn_sites_dedup made: order[k] = the parent's site kept at its place k, ascending; {sites, kept, repeated
  // keys, disagreeing neighbours}; the HIP-event ms of flatten, flags, scan, gather
  bool deduped = false;
  DevBuf<uint32_t> dedup_order;
  int64_t dedup_info[4] = {0, 0, 0, 0};
  double dedup_ms[4] = {0.0, 0.0, 0.0, 0.0};
  // one more chunk: the slab of n_lines lines from file line line0, behind the records held so far ...
  SiteChunk* add_chunk(int64_t line0, int64_t n_lines_) {
    chunks.emplace_back(new SiteChunk);
    SiteChunk* chunk = chunks.back().get();
    chunk->line0 = line0, chunk->n_lines = n_lines_, chunk->before = n_records;
    return chunk;
  }
  // ... and, once known, its records (the last chunk's: `before` of the next one counts them)
  void chunk_records(SiteChunk* chunk, int64_t n) { chunk->n = n, n_records += n; }
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

// one slab [text, text + n): its lines from skip on, appended to h — to its columns, or (resident) as one more chunk with
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
  HIPCHK(c, hipMemcpyAsync(dtext.p, text, n, hipMemcpyHostToDevice, c->stream));  // (n bytes of n_pieces pieces)
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
  if (int rc = to_host(c, &n_newlines, dblock.p + n_blocks, 4)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t n_lines = n_newlines + (text[n - 1] != '\n' ? 1u : 0u);
  h->n_lines += n_lines;
  SiteChunk* chunk = resident ? h->add_chunk(line0, n_lines) : nullptr;
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
  int rc;
  if ((rc = to_host(c, &n_rec, dcount.p + n_runs, 4)) || (rc = to_host(c, &n_def, dcount.p + stride + n_runs, 4))) return rc;
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
  // What comes back — resident: the partial flag counts; host form: the records, start, end and the two floats into their
  // columns as they are, line and meta for SiteColumns::decode — then the deferred triples, and one wait for all of it
  std::vector<uint32_t> partial(flag_blocks), line, meta, dline(n_def), doff(n_def), dlen(n_def);
  const size_t at = h->cols.size();
  if (resident && flag_blocks) {
    if ((rc = to_host(c, partial.data(), dflagged))) return rc;
  } else if (!resident && n_rec) {
    SiteColumns& k = h->cols;
    k.resize(at + n_rec), line.resize(n_rec), meta.resize(n_rec);
    if ((rc = to_host(c, line.data(), out.line)) || (rc = to_host(c, meta.data(), out.meta)) ||
        (rc = to_host(c, k.start.data() + at, out.start)) || (rc = to_host(c, k.end.data() + at, out.end)) ||
        (rc = to_host(c, k.posteriormax.data() + at, out.pm)) || (rc = to_host(c, k.meth_lvl.data() + at, out.ml)))
      return rc;
  }
  if (n_def && ((rc = to_host(c, dline.data(), out.dline)) || (rc = to_host(c, doff.data(), out.doffset)) ||
                (rc = to_host(c, dlen.data(), out.dlength))))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n_def; ++i) {
    h->dline.push_back(line0 + (int64_t)dline[i]);
    h->doffset.push_back(byte0 + (int64_t)doff[i]);
    h->dlength.push_back((int64_t)dlen[i]);
  }
  if (!resident) {
    h->cols.decode(at, n_rec, line0, line.data(), meta.data());
    return ABN_OK;
  }
  h->chunk_records(chunk, n_rec);
  uint64_t n_flagged = 0;
  for (uint32_t v : partial) n_flagged += v;
  if (n_flagged) {  // rare: the warning of src/methylation_site.rs:107-112 names these lines
    line.resize(n_rec), meta.resize(n_rec);
    if ((rc = to_host(c, line.data(), rec.line)) || (rc = to_host(c, meta.data(), rec.meta))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n_rec; ++i)
      if (meta_status_flag(meta[i])) h->flagged.push_back(line0 + (int64_t)line[i]);
  }
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
  if (n_sites) *n_sites = h->n_records + (int64_t)h->cols.size();  // (one of the two is 0 until abn_sites_insert)
  if (n_deferred) *n_deferred = (int64_t)h->dline.size();
  if (n_lines) *n_lines = h->n_lines;
  if (kernel_ms) *kernel_ms = h->kernel_ms;
  return ABN_OK;
}

// The wanted columns of every site in file order.  Host form: column by column.  Resident: every chunk's records come down
// and are merged by line with the inserted ones.
static int sites_fetch(const abn_sites* h, const SiteOut& out) {
  if (!h->ctx) {
    h->cols.copy_to(out);
    return ABN_OK;
  }
  abn_ctx* c = h->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  try {
    size_t j = 0, k = 0;  // the next inserted record, the next place
    const size_t n_ins = h->cols.size();
    const SiteIn ins = h->cols.in();
    for (const auto& chunk : h->chunks) {
      const size_t n = (size_t)chunk->n;
      if (n == 0) continue;
      std::vector<uint32_t> l(n), m(n), s(n), e(n);
      std::vector<double> pm(n), ml(n);
      const RecordBufs& r = chunk->rec;
      int rc;
      if ((rc = to_host(c, l.data(), r.line)) || (rc = to_host(c, m.data(), r.meta)) ||
          (rc = to_host(c, out.start ? s.data() : nullptr, r.start)) || (rc = to_host(c, out.end ? e.data() : nullptr, r.end)) ||
          (rc = to_host(c, out.posteriormax ? pm.data() : nullptr, r.pm)) ||
          (rc = to_host(c, out.meth_lvl ? ml.data() : nullptr, r.ml)))
        return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (size_t i = 0; i < n; ++i) {
        const SiteRecord site = site_decode(chunk->line0, l[i], m[i], s[i], e[i], pm[i], ml[i]);
        while (j < n_ins && ins.line[j] < site.line) out.put(k++, ins.at(j++));
        out.put(k++, site);
      }
    }
    while (j < n_ins) out.put(k++, ins.at(j++));
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_sites_fetch(const abn_sites* h, int64_t* line, int32_t* chromosome, uint32_t* start, uint32_t* end,
                               uint8_t* strand, double* posteriormax, uint8_t* status, uint8_t* status_flag,
                               double* meth_lvl) {
  if (!h) return ABN_ERR_INVALID_ARG;
  return sites_fetch(h, SiteOut{line, chromosome, start, end, strand, posteriormax, status, status_flag, meth_lvl, nullptr});
}

extern "C" int abn_sites_context(const abn_sites* h, int32_t* mask, uint8_t* context) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (mask) *mask = h->mask;
  if (!context) return ABN_OK;
  SiteOut out{};
  out.context = context;
  return sites_fetch(h, out);
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
    for (size_t i = 0; i < h->cols.size(); ++i)
      if (h->cols.status_flag[i]) {
        if (line) line[k] = h->cols.line[i];
        ++k;
      }
    if (n) *n = k;
    return ABN_OK;
  }
  if (n) *n = (int64_t)h->flagged.size();
  if (line) std::copy(h->flagged.begin(), h->flagged.end(), line);
  return ABN_OK;
}

// abn_sites_insert and abn_sites_insert_ctx, and how a child of abn_sites_split gets its share of the parent's inserted
// records (inherited: it has no deferred lines to look the lines up in)
static int sites_insert(abn_sites* h, int64_t n, const SiteIn& in, bool inherited) {
  if (!h || !h->ctx) return ABN_ERR_INVALID_ARG;  // (a host-form handle has no context to report to)
  abn_ctx* c = h->ctx;
  if (h->inserted) return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_insert was already called on this handle");
  if (n < 0 || (n > 0 && !in.complete())) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  try {
    const size_t N = (size_t)n;
    size_t d = 0;  // both lists ascend: every line is looked for behind the one before
    for (size_t j = 0; j < N; ++j) {
      const SiteRecord r = in.at(j);
      if (j > 0 && r.line <= in.line[j - 1]) return set_err(c, ABN_ERR_INVALID_ARG, "the lines are not strictly ascending");
      while (d < h->dline.size() && h->dline[d] < r.line) ++d;
      if (!inherited && (d == h->dline.size() || h->dline[d] != r.line))
        return set_err(c, ABN_ERR_INVALID_ARG, "a line that was not deferred");
      if (r.chromosome < 0 || r.chromosome > 257) return set_err(c, ABN_ERR_INVALID_ARG, "a chromosome outside 0..257");
      if (r.strand > 2 || r.status > 2) return set_err(c, ABN_ERR_INVALID_ARG, "a strand or a status above 2");
      const uint32_t code = r.context;
      if (code > kCtxNone || (code < kCtxNone && !(((uint32_t)h->mask >> code) & 1u)))
        return set_err(c, ABN_ERR_INVALID_ARG, "a context code above 3 or outside the handle's contexts");
    }
    if (N > 0) {
      std::vector<MergeChunk> refs;
      for (const auto& chunk : h->chunks) refs.push_back(chunk->ref());
      std::vector<long long> l(in.line, in.line + N);
      std::vector<int32_t> pick(N);
      if (!merge_pick_chunks(refs.data(), (int)refs.size(), l.data(), (long long)N, pick.data()))
        return set_err(c, ABN_ERR_INVALID_ARG, "a line outside every slab");
      HIPCHK(c, hipSetDevice(c->device));
      PoolScope pool_scope(c);
      if (int rc = h->ins.upload(c, in, l, pick, refs)) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staging vectors go on return
      h->cols.resize(N);  // the host's copy, for abn_sites_fetch
      const SiteOut copy = h->cols.view();
      for (size_t j = 0; j < N; ++j) copy.put(j, in.at(j));
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
  return sites_insert(h, n, SiteIn{line, chromosome, start, end, strand, posteriormax, status, meth_lvl, context}, false);
}

extern "C" int abn_sites_insert(abn_sites* h, int64_t n, const int64_t* line, const int32_t* chromosome,
                                const uint32_t* start, const uint32_t* end, const uint8_t* strand,
                                const double* posteriormax, const uint8_t* status, const double* meth_lvl) {
  if (h && h->ctx && n > 0 && h->mask != (int32_t)kContextsCG)
    return set_err(h->ctx, ABN_ERR_INVALID_ARG, "the handle holds other contexts than CG: abn_sites_insert_ctx names each record's");
  return sites_insert(h, n, SiteIn{line, chromosome, start, end, strand, posteriormax, status, meth_lvl, nullptr}, false);
}

// ---- abn_sites_split
namespace {

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
    if (int rc = to_device(c, dtable.p, table.data(), dtable.bytes())) return rc;  // the parent's chunks, their workgroups
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
    if (int rc = to_host(c, size.data(), dsize)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // the children's chunks: a slab keeps its lines, and holds the child's share of its records
  for (int i = 0; i < n_chunks; ++i)
    for (int k = 0; k < kSplitChildren; ++k) {
      if (!kids[k]) continue;  // (a context outside the mask has no child, and the kernels count no record for it)
      SiteChunk* chunk = kids[k]->add_chunk(h->chunks[(size_t)i]->line0, h->chunks[(size_t)i]->n_lines);
      kids[k]->chunk_records(chunk, size[(size_t)i * kSplitChildren + k]);
      HIPCHK(c, chunk->rec.alloc((size_t)chunk->n, 0));
      table[(size_t)i].out[k] = chunk->rec.records();
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
    if (int rc = to_device(c, dtable.p, table.data(), dtable.bytes())) return rc;  // ... and the children's chunks
    if (n_flagged) {
      if (!merge_pick_chunks(refs.data(), n_chunks, fline.data(), (long long)n_flagged, fchunk.data()))
        return set_err(c, ABN_ERR_HIP, "abn_sites_split: a flagged line outside every slab");
      HIPCHK(c, dmember.alloc(n_flagged));
      if (int rc = upload(c, dfline, fline.data(), n_flagged)) return rc;
      if (int rc = upload(c, dfchunk, fchunk.data(), n_flagged)) return rc;
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
      if (int rc = to_host(c, member.data(), dmember)) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the tables and staging vectors go on return
  }
  for (int k = 0; k < kSplitChildren; ++k) {
    if (!kids[k]) continue;
    abn_sites* kid = kids[k].get();
    kid->split_ms[0] = h->split_ms[0], kid->split_ms[1] = h->split_ms[1];
    for (size_t j = 0; j < n_flagged; ++j)
      if ((member[j] >> k) & 1u) kid->flagged.push_back(h->flagged[j]);
    SiteColumns part;  // the parent's inserted records of this membership, uploaded as abn_sites_insert uploads them
    for (size_t j = 0; j < h->cols.size(); ++j)
      if (h->cols.context[j] == kCtxNone || h->cols.context[j] == (uint32_t)k) part.push(h->cols.in().at(j));
    if (int rc = sites_insert(kid, (int64_t)part.size(), part.in(), true)) return rc;
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

// ---- abn_sites_sort (kernels and the sort itself: abn_sites_sort.hpp, abn_sites_sort.hip)
int abn::sites_scan_rows(abn_ctx* c, uint32_t* data, uint32_t rows, uint32_t n, uint32_t stride) {
  hipLaunchKernelGGL(abn_parse_scan_kernel, dim3(rows), dim3(kParseScanThreads), 0, c->stream, data, n, stride);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

namespace {

// What abn_sites_sort and abn_sites_dedup share.  The flattened records of a handle: its sites in file order with their
// whole record
struct FlatBufs {
  DevBuf<uint32_t> meta, start, end;
  DevBuf<double> pm, ml;
  SortFlat ref() const { return SortFlat{meta.p, start.p, end.p, pm.p, ml.p}; }
};

// the flatten of h's N > 0 sites into f; *ms = its HIP-event ms
int sites_flatten(const abn_sites* h, size_t N, FlatBufs& f, double* ms) {
  abn_ctx* c = h->ctx;
  DevBuf<uint8_t> dcontext;
  HIPCHK(c, f.meta.alloc(N));
  HIPCHK(c, f.start.alloc(N));
  HIPCHK(c, f.end.alloc(N));
  HIPCHK(c, f.pm.alloc(N));
  HIPCHK(c, f.ml.alloc(N));
  const SortFlat flat = f.ref();
  const MergeInserted ins = h->ins.ref();
  if (ins.n > 0)
    if (int rc = upload(c, dcontext, h->cols.context.data(), h->cols.context.size())) return rc;
  EventPair ev;
  if (int rc = ev.begin(c, true)) return rc;
  for (const auto& src : h->chunks)
    if (int rc = sort_flatten_records_dev(c, src->ref(), ins.line, ins.n, flat)) return rc;
  if (int rc = sort_flatten_inserted_dev(c, h->ins.chunks.p, ins, dcontext.p, flat)) return rc;
  return ev.end(c, ms);  // (waits: dcontext may go)
}

// the child of h that both make: h's context and mask, one chunk of n lines that are its n records, counted as inserted
SiteChunk* sites_child(const abn_sites* h, abn_sites* kid, int64_t n) {
  kid->ctx = h->ctx, kid->device = h->device;
  kid->mask = h->mask;
  kid->n_lines = n;
  kid->inserted = true;
  SiteChunk* chunk = kid->add_chunk(0, n);
  kid->chunk_records(chunk, n);
  return chunk;
}

// rare: the ranks of the parent's flagged records among the child's N, from the child's meta words
int sites_child_flagged(const abn_sites* h, abn_sites* kid, const SiteChunk* chunk, size_t N) {
  if (h->flagged.empty() || N == 0) return ABN_OK;
  abn_ctx* c = h->ctx;
  std::vector<uint32_t> meta(N);
  if (int rc = to_host(c, meta.data(), chunk->rec.meta)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < N; ++k)
    if (meta_status_flag(meta[k])) kid->flagged.push_back((int64_t)k);
  return ABN_OK;
}

int sites_sort(const abn_sites* h, abn_sites* kid) {
  abn_ctx* c = h->ctx;
  const int64_t n = h->n_records + (int64_t)h->cols.size();
  SiteChunk* chunk = sites_child(h, kid, n);
  kid->sorted = true;
  kid->sort_info[0] = n;
  if (n == 0) return ABN_OK;
  const size_t N = (size_t)n;
  FlatBufs f;
  HIPCHK(c, kid->sort_order.alloc(N));
  HIPCHK(c, chunk->rec.alloc(N, 0));
  if (int rc = sites_flatten(h, N, f, &kid->sort_ms[0])) return rc;
  const SortFlat flat = f.ref();
  if (int rc = sort_flat_dev(c, n, flat, kid->sort_order.p, kid->sort_info, &kid->sort_ms[1])) return rc;
  EventPair ev;
  if (int rc = ev.begin(c, true)) return rc;
  if (int rc = sort_gather_dev(c, flat, kid->sort_order.p, n, chunk->rec.records())) return rc;
  if (int rc = ev.end(c, &kid->sort_ms[3])) return rc;
  return sites_child_flagged(h, kid, chunk, N);
}

// The child's records are allocated once the number kept is known: the flags and the compaction run first, into an order
// buffer with room for every record; the child keeps a copy of its kept entries
int sites_dedup(const abn_sites* h, int policy, abn_sites* kid) {
  abn_ctx* c = h->ctx;
  const int64_t n = h->n_records + (int64_t)h->cols.size();
  kid->deduped = true;
  kid->dedup_info[0] = n;
  if (n == 0) {
    sites_child(h, kid, 0);
    return ABN_OK;
  }
  FlatBufs f;
  DevBuf<uint32_t> dorder;
  HIPCHK(c, dorder.alloc((size_t)n));
  if (int rc = sites_flatten(h, (size_t)n, f, &kid->dedup_ms[0])) return rc;
  const SortFlat flat = f.ref();
  double ms2[2] = {0.0, 0.0};
  if (int rc = dedup_flat_dev(c, n, flat, policy, dorder.p, kid->dedup_info, ms2)) return rc;
  kid->dedup_ms[1] = ms2[0], kid->dedup_ms[2] = ms2[1];
  const int64_t kept = kid->dedup_info[1];
  SiteChunk* chunk = sites_child(h, kid, kept);
  if (kept == 0) return ABN_OK;
  const size_t K = (size_t)kept;
  HIPCHK(c, kid->dedup_order.alloc(K));
  HIPCHK(c, chunk->rec.alloc(K, 0));
  HIPCHK(c, hipMemcpyAsync(kid->dedup_order.p, dorder.p, K * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  EventPair ev;
  if (int rc = ev.begin(c, true)) return rc;
  if (int rc = dedup_gather_dev(c, flat, kid->dedup_order.p, kept, n, chunk->rec.records())) return rc;
  if (int rc = ev.end(c, &kid->dedup_ms[3])) return rc;  // (waits: f and dorder may go)
  return sites_child_flagged(h, kid, chunk, K);
}

// the shell of abn_sites_sort and abn_sites_dedup (`name`) behind their own checks: a new handle around build(kid)
template <class Build>
int sites_child_entry(const abn_sites* h, abn_sites** out, const char* name, Build build) {
  if (out) *out = nullptr;
  if (!h || !h->ctx) return ABN_ERR_INVALID_ARG;  // (a host-form handle has no context to report to)
  abn_ctx* c = h->ctx;
  if (!out) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (!h->dline.empty() && !h->inserted)
    return set_err(c, ABN_ERR_INVALID_ARG, std::string(name) + ": the handle has deferred lines and abn_sites_insert was never called");
  if (h->n_records + (int64_t)h->cols.size() >= (int64_t)1 << 32)
    return set_err(c, ABN_ERR_INVALID_ARG, std::string(name) + ": 2^32 records or more");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  std::unique_ptr<abn_sites> kid(new (std::nothrow) abn_sites);
  if (!kid) return set_err(c, ABN_ERR_HIP, "out of host memory");
  try {
    if (int rc = build(kid.get())) return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  *out = kid.release();
  return ABN_OK;
}

// *n = the child's sites, order [*n] = its order buffer on the host; either may be null
int sites_child_order(const abn_sites* kid, const DevBuf<uint32_t>& dorder, int64_t* n, int64_t* order) {
  abn_ctx* c = kid->ctx;
  if (n) *n = kid->n_records;
  if (!order || kid->n_records == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  try {
    std::vector<uint32_t> o((size_t)kid->n_records);
    if (int rc = to_host(c, o.data(), dorder)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < o.size(); ++k) order[k] = (int64_t)o[k];
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}

}  // namespace

extern "C" int abn_sites_sort(const abn_sites* h, abn_sites** out) {
  return sites_child_entry(h, out, "abn_sites_sort", [&](abn_sites* kid) { return sites_sort(h, kid); });
}

extern "C" int abn_sites_sort_order(const abn_sites* sorted, int64_t* n, int64_t* order) {
  if (!sorted || !sorted->sorted) return ABN_ERR_INVALID_ARG;
  return sites_child_order(sorted, sorted->sort_order, n, order);
}

extern "C" int abn_sites_sort_info(const abn_sites* sorted, int64_t* info4, double* ms4) {
  if (!sorted || !sorted->sorted) return ABN_ERR_INVALID_ARG;
  if (info4) std::copy(sorted->sort_info, sorted->sort_info + 4, info4);
  if (ms4) std::copy(sorted->sort_ms, sorted->sort_ms + 4, ms4);
  return ABN_OK;
}

// ---- abn_sites_dedup (kernels: abn_sites_dedup.hpp; the collapse itself: abn_sites_dedup.hip)
extern "C" int abn_sites_dedup(const abn_sites* h, int policy, abn_sites** out) {
  if (out) *out = nullptr;
  if (h && h->ctx && !dedup_policy_valid(policy)) return set_err(h->ctx, ABN_ERR_INVALID_ARG, "abn_sites_dedup: a policy outside 0..3");
  return sites_child_entry(h, out, "abn_sites_dedup", [&](abn_sites* kid) { return sites_dedup(h, policy, kid); });
}

extern "C" int abn_sites_dedup_order(const abn_sites* child, int64_t* n, int64_t* order) {
  if (!child || !child->deduped) return ABN_ERR_INVALID_ARG;
  return sites_child_order(child, child->dedup_order, n, order);
}

extern "C" int abn_sites_dedup_info(const abn_sites* child, int64_t* info4, double* ms4) {
  if (!child || !child->deduped) return ABN_ERR_INVALID_ARG;
  if (info4) std::copy(child->dedup_info, child->dedup_info + 4, info4);
  if (ms4) std::copy(child->dedup_ms, child->dedup_ms + 4, ms4);
  return ABN_OK;
}

// ---- for abn_windows_create_parsed (abn_windows.hip)
abn_ctx* abn::sites_ctx(const abn_sites* h) { return h ? h->ctx : nullptr; }

int64_t abn::sites_merged_count(const abn_sites* h) {
  if (!h || !h->ctx || (!h->dline.empty() && !h->inserted)) return -1;
  return h->n_records + (int64_t)h->cols.size();
}

// The merge of one sample into `out`, nothing waited for: the fields kernel of every chunk (inserted = false), or the insert
// kernel over the handle's inserted records (true)
template <class Fields, class Insert, class Out>
static int sites_merge(const abn_sites* h, bool inserted, double filter, Fields fields_kernel, Insert insert_kernel,
                       const Out& out) {
  abn_ctx* c = h->ctx;
  const MergeInserted ins = h->ins.ref();
  if (!inserted) {
    for (const auto& chunk : h->chunks) {
      if (chunk->n == 0) continue;
      const unsigned grid = (unsigned)((chunk->n + kMergeThreads - 1) / kMergeThreads);
      hipLaunchKernelGGL(fields_kernel, dim3(grid), dim3(kMergeThreads), 0, c->stream, chunk->ref(), ins.line, ins.n, filter,
                         out);
      HIPCHK(c, hipGetLastError());
    }
  } else if (ins.n > 0) {
    const unsigned grid = (unsigned)((ins.n + kMergeThreads - 1) / kMergeThreads);
    hipLaunchKernelGGL(insert_kernel, dim3(grid), dim3(kMergeThreads), 0, c->stream, (const MergeChunk*)h->ins.chunks.p, ins,
                       filter, out);
    HIPCHK(c, hipGetLastError());
  }
  return ABN_OK;
}

int abn::sites_merge_dev(const abn_sites* h, bool inserted, double filter, int32_t* dchrom, uint32_t* dstart,
                         uint32_t* dend, uint8_t* dstrand, uint8_t* dcode, double* dlevel) {
  return sites_merge(h, inserted, filter, abn_sites_fields_kernel, abn_sites_insert_kernel,
                     MergeOut{dchrom, dstart, dend, dstrand, dcode, dlevel});
}

// ---- for abn_codes_create_parsed (abn_codes.hip): the same launches with the reduced writers of abn_codes.hpp
int abn::sites_merge_codes_dev(const abn_sites* h, bool inserted, double filter, uint8_t* dcode, double* dlevel) {
  return sites_merge(h, inserted, filter, abn_codes_fields_kernel, abn_codes_insert_kernel, CodesOut{dcode, dlevel});
}
