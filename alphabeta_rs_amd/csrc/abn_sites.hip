// abn_sites_*: methylome text -> site records on the device (src/methylation_site.rs:146-362 for every line of a file,
// the loops of src/windows.rs:303-338 and src/pedigree.rs:138-178 in front of it).  Kernels: abn_parse_kernels.hpp; the
// line parser they share with the host: abn_parse.hpp.
#include "abn_host.hpp"
#include "abn_parse_kernels.hpp"

using namespace abn;

constexpr int64_t kSitesDefaultSlab = (int64_t)64 << 20, kSitesMaxSlab = (int64_t)1 << 30;

struct abn_sites {
  std::vector<int64_t> line, dline, doffset, dlength;
  std::vector<int32_t> chromosome;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, status, status_flag;
  std::vector<double> posteriormax, meth_lvl;
  int64_t n_lines = 0;
  double kernel_ms = 0.0;
};

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

// one slab [text, text + n): its lines from skip on, appended to h; line numbers and offsets are the file's
int parse_slab(abn_ctx* c, abn_sites* h, const char* text, size_t n, int64_t skip, int64_t line0, int64_t byte0,
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
                     dbegin.p, n_newlines, n_lines, first, run.records(), run.deferred(), dcount.p, stride);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_parse_scan_kernel, dim3(2), dim3(kParseScanThreads), 0, c->stream, dcount.p, n_runs, stride);
  HIPCHK(c, hipGetLastError());
  if (int rc = timed()) return rc;
  uint32_t n_rec = 0, n_def = 0;
  HIPCHK(c, hipMemcpyAsync(&n_rec, dcount.p + n_runs, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&n_def, dcount.p + stride + n_runs, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_rec == 0 && n_def == 0) return ABN_OK;
  HIPCHK(c, out.alloc(n_rec, n_def));
  if (int rc = ev.begin(c, true)) return rc;
  hipLaunchKernelGGL(abn_parse_compact_kernel, dim3(n_runs), dim3(kParseThreads), 0, c->stream, run.records(),
                     run.deferred(), dcount.p, stride, out.records(), out.deferred());
  HIPCHK(c, hipGetLastError());
  if (int rc = timed()) return rc;
  std::vector<uint32_t> line(n_rec), meta(n_rec), start(n_rec), end(n_rec), dline(n_def), doff(n_def), dlen(n_def);
  const size_t at = h->line.size(), dat = h->dline.size();
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
  for (size_t i = 0; i < n_rec; ++i) {
    const uint32_t m = meta[i];
    h->line[at + i] = line0 + (int64_t)line[i];
    h->chromosome[at + i] = (int32_t)(m & 0xffffu);
    h->strand[at + i] = (uint8_t)((m >> 16) & 0xfu);
    h->status[at + i] = (uint8_t)((m >> 20) & 0xfu);
    h->status_flag[at + i] = (uint8_t)((m >> 24) & 0xfu);
  }
  h->dline.resize(dat + n_def);
  h->doffset.resize(dat + n_def);
  h->dlength.resize(dat + n_def);
  for (size_t i = 0; i < n_def; ++i) {
    h->dline[dat + i] = line0 + (int64_t)dline[i];
    h->doffset[dat + i] = byte0 + (int64_t)doff[i];
    h->dlength[dat + i] = (int64_t)dlen[i];
  }
  return ABN_OK;
}

}  // namespace

extern "C" int abn_sites_parse(abn_ctx* c, const char* text, int64_t n_bytes, const abn_sites_params* params,
                               abn_sites** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!out || n_bytes < 0 || (n_bytes > 0 && !text)) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  int64_t slab = params ? params->slab_bytes : 0, skip = params ? params->skip_lines : 1;
  if (slab < 0 || slab > kSitesMaxSlab || skip < 0) return set_err(c, ABN_ERR_INVALID_ARG, "slab_bytes / skip_lines");
  if (slab == 0) slab = kSitesDefaultSlab;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  std::unique_ptr<abn_sites> h(new (std::nothrow) abn_sites);
  if (!h) return set_err(c, ABN_ERR_HIP, "out of host memory");
  EventPair ev;
  try {
    const size_t n = (size_t)n_bytes;
    for (size_t from = 0; from < n;) {
      const size_t to = slab_end(text, n, from, (size_t)slab);
      if (to - from > (size_t)kSitesMaxSlab + (size_t)kSitesMaxSlab)
        return set_err(c, ABN_ERR_INVALID_ARG, "a line of more than 2 GiB");
      const int64_t before = h->n_lines;
      if (int rc = parse_slab(c, h.get(), text + from, to - from, skip, before, (int64_t)from, ev)) return rc;
      skip = std::max<int64_t>(0, skip - (h->n_lines - before));
      from = to;
    }
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  *out = h.release();
  return ABN_OK;
}

extern "C" int abn_sites_destroy(abn_sites* h) {
  if (!h) return ABN_ERR_INVALID_ARG;
  delete h;
  return ABN_OK;
}

extern "C" int abn_sites_info(const abn_sites* h, int64_t* n_sites, int64_t* n_deferred, int64_t* n_lines,
                              double* kernel_ms) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_sites) *n_sites = (int64_t)h->line.size();
  if (n_deferred) *n_deferred = (int64_t)h->dline.size();
  if (n_lines) *n_lines = h->n_lines;
  if (kernel_ms) *kernel_ms = h->kernel_ms;
  return ABN_OK;
}

extern "C" int abn_sites_fetch(const abn_sites* h, int64_t* line, int32_t* chromosome, uint32_t* start, uint32_t* end,
                               uint8_t* strand, double* posteriormax, uint8_t* status, uint8_t* status_flag,
                               double* meth_lvl) {
  if (!h) return ABN_ERR_INVALID_ARG;
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

extern "C" int abn_sites_deferred(const abn_sites* h, int64_t* line, int64_t* offset, int64_t* length) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (line) std::copy(h->dline.begin(), h->dline.end(), line);
  if (offset) std::copy(h->doffset.begin(), h->doffset.end(), offset);
  if (length) std::copy(h->dlength.begin(), h->dlength.end(), length);
  return ABN_OK;
}
