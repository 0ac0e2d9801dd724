// The pedigree build from resident parse results (abn_codes_create_parsed): what Pedigree::build reads of every site
// (src/pedigree.rs:138-178 and :210-261) made on the device from the records abn_sites_parse_dev left there — the packed
// code matrix of abn_pairwise_divergence_packed_dev and every sample's rc_meth_lvl fold — without a host copy of any site.
//
//   merge   the reduced form of abn_sites_merge.hpp's writers: the same places (merge_dest_record, merge_dest_inserted),
//           but only a MERGED BYTE and the level per site, 9 bytes.  The merged byte is merge_code's byte (the status, 0x80
//           when the posterior is below the filter) plus kCodeCounted where the site counts for rc_meth_lvl.
//   pack    a lane per dword of the packed matrix: 16 merged bytes -> the 16 fields of include/abneutral.h
//           (abn_pack_codes), every field behind a sample's last site 3.
//   fold    sum += meth_lvl over the counted sites from +0.0 in file order, and their number: one wavefront per sample.
//
// TWO PREDICATES, both the host's, and they differ on a NaN posterior (only an inserted, host-decided record has one):
//   filtered  posteriormax <  filter   (DMatrix::from, src/pedigree.rs:249: merge_code)      NaN: not filtered
//   counted   posteriormax >= filter   (Pedigree::build, src/pedigree.rs:159-172)            NaN: not counted
// so `counted` is never derived from the code's 0x80.
//
// THE FOLD IS EXACT.  The chain s = s + x cannot be re-associated, so every lane of the wavefront runs the same chain over
// the 64 values of a step, broadcast by constant lane index.  An uncounted site (and a lane behind the last site) gets the
// addend +0.0, chosen in parallel before the chain, instead of being skipped: a round-to-nearest sum that starts at +0.0 is
// never -0.0 (x + y is -0.0 only when both are), so s + (+0.0) has the bits of s.  A NaN level of a counted site makes the
// sum NaN on both sides; which NaN is not part of the contract.
//
// The arithmetic and the whole thing in its serial form compile without a HIP header: the host library (host_capi.cpp)
// and tests/native/codes_main.cpp include this file as it is.
#pragma once
#include "abn_sites_merge.hpp"

namespace abn {

constexpr uint8_t kCodeCounted = 0x40;  // in a merged byte: the site counts for rc_meth_lvl
constexpr int kCodesThreads = 256;      // the pack kernel's workgroup
constexpr int kCodesWave = 64;          // the fold kernel's: one wavefront

struct CodesOut {  // what the pack and the fold read, at the sample's first site
  uint8_t* code;   // merged bytes
  double* level;
};

// the site's level is part of rc_meth_lvl (read_inputs, host/pedigree_build.hpp): the host's `>=`, so a NaN posterior is not
ABN_HOST_DEVICE inline bool merge_counted(double posteriormax, double filter) { return posteriormax >= filter; }

ABN_HOST_DEVICE inline uint8_t merge_byte(uint32_t status, double posteriormax, double filter) {
  return (uint8_t)(merge_code(status, posteriormax, filter) | (merge_counted(posteriormax, filter) ? kCodeCounted : 0u));
}

// one device record to its place: what a lane of abn_codes_fields_kernel does
ABN_HOST_DEVICE inline long long codes_write_record(const MergeChunk& c, long long i, const long long* inserted_line,
                                                    long long n_inserted, double filter, const CodesOut& out) {
  const long long d = merge_dest_record(c, i, inserted_line, n_inserted);
  out.code[d] = merge_byte(meta_status(c.meta[i]), c.posteriormax[i], filter);
  out.level[d] = c.meth_lvl[i];
  return d;
}

// one inserted record to its place: what a lane of abn_codes_insert_kernel does (of ins: line, chunk, status,
// posteriormax, meth_lvl are read)
ABN_HOST_DEVICE inline long long codes_write_inserted(const MergeChunk* chunks, const MergeInserted& ins, long long j,
                                                      double filter, const CodesOut& out) {
  const long long d = merge_dest_inserted(chunks[ins.chunk[j]], j, ins.line[j]);
  out.code[d] = merge_byte(ins.status[j], ins.posteriormax[j], filter);
  out.level[d] = ins.meth_lvl[j];
  return d;
}

// Four merged bytes in a little-endian word -> their four fields, a byte each: 3 where 0x80 is set, else the status
ABN_HOST_DEVICE inline uint32_t codes_fields4(uint32_t w) {
  const uint32_t filtered = (w >> 7) & 0x01010101u;
  return (w & 0x03030303u) | filtered * 3u;  // (status | 3 = 3; no byte carries into the next)
}

// The dword of the sites 16 g .. 16 g + 15 of a row: w[j] holds the merged bytes of the sites 16 g + 4 j + e in its bytes
// e = 0 .. 3; the first `valid` (0 .. 16) sites exist, every field behind them is 3.  Site 16 g + 4 j + e: byte e, bits
// 2j .. 2j+1 (include/abneutral.h).
ABN_HOST_DEVICE inline uint32_t codes_pack_dword(const uint32_t w[4], int valid) {
  uint32_t out = 0;
  for (int j = 0; j < 4; ++j) {
    const int here = valid - 4 * j;  // sites of this word that exist
    const uint32_t keep = here >= 4 ? 0xffffffffu : (here <= 0 ? 0u : (1u << (8 * here)) - 1u);
    out |= ((codes_fields4(w[j]) & keep) | (0x03030303u & ~keep)) << (2 * j);
  }
  return out;
}

// a packed row [row_stride_bytes] from the n merged bytes of a sample, serially: what the pack kernel's lanes write
inline void codes_pack_row_serial(const uint8_t* code, long long n, uint8_t* row, long long row_stride_bytes) {
  for (long long g = 0; g < row_stride_bytes / 4; ++g) {
    const long long left = n - 16 * g;
    const int valid = left >= 16 ? 16 : (left <= 0 ? 0 : (int)left);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < valid; ++k) w[k >> 2] |= (uint32_t)code[16 * g + k] << (8 * (k & 3));
    const uint32_t d = codes_pack_dword(w, valid);
    for (int e = 0; e < 4; ++e) row[4 * g + e] = (uint8_t)(d >> (8 * e));
  }
}

// the fold in the device's form: the addend of an uncounted site is +0.0 (exact: see above)
inline void codes_fold_serial(const uint8_t* code, const double* level, long long n, double* sum, long long* kept) {
  double s = 0.0;
  long long k = 0;
  for (long long i = 0; i < n; ++i) {
    const bool counted = (code[i] & kCodeCounted) != 0;
    s = s + (counted ? level[i] : 0.0);
    k += counted ? 1 : 0;
  }
  *sum = s;
  *kept = k;
}

// The whole build of one sample, serially: the merge into code / level [records of all chunks + ins.n], then the pack of
// the merged bytes into row [row_stride_bytes: a multiple of 4, at least a quarter byte per site], then the fold.
inline void codes_build_serial(const MergeChunk* chunks, int n_chunks, const MergeInserted& ins, double filter,
                               const CodesOut& out, uint8_t* row, long long row_stride_bytes, double* sum,
                               long long* kept) {
  long long n = ins.n;
  for (int c = 0; c < n_chunks; ++c) {
    n += chunks[c].n;
    for (long long i = 0; i < chunks[c].n; ++i) codes_write_record(chunks[c], i, ins.line, ins.n, filter, out);
  }
  for (long long j = 0; j < ins.n; ++j) codes_write_inserted(chunks, ins, j, filter, out);
  codes_pack_row_serial(out.code, n, row, row_stride_bytes);
  codes_fold_serial(out.code, out.level, n, sum, kept);
}

#if defined(__HIPCC__) && defined(ABN_CODES_MERGE_KERNELS)  // (abn_sites.hip defines it: the records are its handle's)
// ------------------------------------------------------------------------------------------------ merge kernels
// grid: ceil(chunk.n / kMergeThreads)
__global__ void __launch_bounds__(kMergeThreads)
abn_codes_fields_kernel(MergeChunk chunk, const long long* __restrict__ inserted_line, long long n_inserted, double filter,
                        CodesOut out) {
  const long long i = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (i < chunk.n) codes_write_record(chunk, i, inserted_line, n_inserted, filter, out);
}

// grid: ceil(ins.n / kMergeThreads); chunks: the sample's chunk table in device memory
__global__ void __launch_bounds__(kMergeThreads)
abn_codes_insert_kernel(const MergeChunk* __restrict__ chunks, MergeInserted ins, double filter, CodesOut out) {
  const long long j = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (j < ins.n) codes_write_inserted(chunks, ins, j, filter, out);
}
#endif

#if defined(__HIPCC__) && (defined(ABN_CODES_KERNELS) || defined(ABN_TILES_KERNELS))
// ------------------------------------------------------------------------------------------------ the fold of one wavefront
// The n sites at c (merged bytes) and l (levels), by the 64 lanes of one wavefront: acc = the chain s = s + x from +0.0 in
// file order, count = the counted sites; every lane ends with both.  Per step 64 sites: one coalesced load of their levels
// and merged bytes — the next step's issued before this step's chain begins, so their latency sits behind the 64 dependent
// additions — then every lane runs the same chain over the 64 addends, read by constant lane index.  c and l need no
// alignment.  (Shared by abn_codes_fold_kernel, a sample per wavefront, and abn_tiles.hpp's abn_tiles_fold_kernel, a
// (sample, tile) per wavefront.)
__device__ __forceinline__ void codes_fold_wave(const uint8_t* __restrict__ c, const double* __restrict__ l, long long n,
                                                int lane, double& acc_out, long long& count_out) {
  double acc = 0.0;
  long long count = 0;
  // A lane behind the last site loads the last site again (an index clamped to n - 1, never out of bounds) and is masked
  // where its values are used: loads under a branch would make the chain wait for the next step's too.
  const long long first = lane < n ? lane : n - 1;
  double next_level = n > 0 ? l[first] : 0.0;
  uint8_t next_code = n > 0 ? c[first] : (uint8_t)0;
  for (long long base = 0; base < n; base += kCodesWave) {
    const bool counted = base + lane < n && (next_code & kCodeCounted) != 0;
    const double x = counted ? next_level : 0.0;  // +0.0 for an uncounted site: changes no bit of the sum
    const long long ahead = base + kCodesWave + lane < n ? base + kCodesWave + lane : n - 1;
    next_level = l[ahead];
    next_code = c[ahead];
    asm volatile("" ::: "memory");  // the loads stay here, in front of the chain (else they are merged with the first
                                    // step's into one load at the loop's head, behind the chain of the step before)
    count +=__popcll(__ballot(counted));
    const int lo = __double2loint(x), hi = __double2hiint(x);
#pragma unroll
    for (int j = 0; j < kCodesWave; ++j)
      acc = acc + __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
  }
  acc_out = acc;
  count_out = count;
}
#endif

#if defined(__HIPCC__) && defined(ABN_CODES_KERNELS)  // (abn_codes.hip defines it)
// ------------------------------------------------------------------------------------------------ pack and fold
// Sample s: its merged bytes at code + code_off[s] (a multiple of 16; the bytes up to the next multiple of 16 behind its
// last site belong to it and may hold anything), its levels at level + site_off[s], site_off[s + 1] - site_off[s] sites.

// grid: ceil(n_samples * row_dwords / kCodesThreads); a lane per dword of packed [n_samples x 4 row_dwords bytes]
__global__ void __launch_bounds__(kCodesThreads)
abn_codes_pack_kernel(const uint8_t* __restrict__ code, const long long* __restrict__ code_off,
                      const long long* __restrict__ site_off, int n_samples, long long row_dwords,
                      uint32_t* __restrict__ packed) {
  const long long at = (long long)blockIdx.x * kCodesThreads + threadIdx.x;
  if (at >= (long long)n_samples * row_dwords) return;
  const long long s = at / row_dwords, g = at - s * row_dwords;
  const long long left = site_off[s + 1] - site_off[s] - 16 * g;
  const int valid = left >= 16 ? 16 : (left <= 0 ? 0 : (int)left);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (valid > 0) v = *(const uint4*)(code + code_off[s] + 16 * g);  // within the sample's bytes, 16-byte aligned
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  packed[at] = codes_pack_dword(w, valid);
}

// grid: n_samples workgroups of one wavefront: codes_fold_wave (above) over the sample's sites.  Lane 0 writes sum[s] and
// kept[s].
__global__ void __launch_bounds__(kCodesWave)
abn_codes_fold_kernel(const uint8_t* __restrict__ code, const double* __restrict__ level,
                      const long long* __restrict__ code_off, const long long* __restrict__ site_off,
                      double* __restrict__ sum, long long* __restrict__ kept) {
  const int s = blockIdx.x, lane = threadIdx.x;
  double acc;
  long long count;
  codes_fold_wave(code + code_off[s], level + site_off[s], site_off[s + 1] - site_off[s], lane, acc, count);
  if (lane == 0) {
    sum[s] = acc;
    kept[s] = count;
  }
}
#endif  // kernels

}  // namespace abn
