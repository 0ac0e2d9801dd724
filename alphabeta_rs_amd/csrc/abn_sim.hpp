// Methylomes simulated down a pedigree under the ABneutral model (src/divergence.rs:33-114): the law, its serial form, the
// thresholds from rates, and the kernel.  Host and device share this header; it compiles without a HIP header
// (tests/native/sim_main.cpp builds it with g++), the kernel only where abn_sim.hip asks for it (ABN_SIM_KERNELS).
//
// THE LAW.  A site of a diploid selfing line is UU, UM or MM — the codes 0, 1, 2, the U / I / M of the pairwise scan
// (src/pedigree.rs:253-257).  A tree of V nodes: parent[0] = -1, 0 <= parent[v] < v; thr[V][3][2] uint64 with
// thr[v][s][0] <= thr[v][s][1]; emit[V] uint8; n_sites = L; a 64-bit seed.
//   draw   u(k, v) = (uint64)H[k & 3] << 32 | Lw[k & 3], where H = philox4x32_10(c0 = (uint32)(k >> 2), c1 = 0, c2 = v,
//          c3 = kTagSim, seed_lo, seed_hi) and Lw is the same call with c1 = 1
//   state  founder: state(k, 0) = (u >= thr[0][0][0]) + (u >= thr[0][0][1]); any other node, with s = state(k, parent[v]):
//          state(k, v) = (u >= thr[v][s][0]) + (u >= thr[v][s][1])
//   output the r-th emitted node, in node order, is row r of a packed matrix in the format of abn_pack.cpp: the field of
//          site k holds its state, every field from site L to the end of abn_packed_row_stride(L) bytes holds 3; bytes of a
//          longer row_stride are not written
// A node's row depends on the seed, its own index, its ancestors and their thresholds — not on L, not on any other node,
// not on emit.  Refused before any launch (sim_refusal): null pointers, V < 1 or V > kSimMaxNodes, a parent outside the
// rule, thr[..][0] > thr[..][1], no emitted node, L < 0 or L > 2^34 (c0 is 32 bits of k >> 2), a row_stride that is not a
// multiple of 64 or is below abn_packed_row_stride(L).  kSimMaxNodes = 65535: what the pairwise scan takes as samples, so
// that every emitted set can be scanned.
//
// THRESHOLDS FROM RATES (sim_thresholds; host only).  For v > 0 the three rows of G^(generation[v] - generation[parent[v]]),
// G = genmatrix(alpha, beta) of src/divergence.rs:96-114, the power the reference's left-accumulated chain (:16-31; power
// 0: the identity — the child copies its parent); the founder's row is [p_uu0, w (1 - p_uu0), (1 - w)(1 - p_uu0)] .
// G^generation[0] (:44, :55).  Of a row p: c0 = p[0], c1 = p[0] + p[1] (one rounded add); threshold(c) = 0 for c <= 0,
// 2^64 - 1 for c >= 1, else (uint64)ldexp(c, 64).  A cumulative probability is a double: it is resolved to 2^-53 of 1, so
// a one-generation UU -> MM step at alpha = 4e-9 (probability 1.6e-17) cannot be represented — c1 rounds to 1.
//
// THE KERNEL.  One lane owns one dword of a row — 16 sites, the four Philox quads 4 g .. 4 g + 3 — and walks the nodes in
// index order; lanes are grid-strided over the dwords of a row.  A node that is emitted writes straight into the output, one
// that is not but has an emitted descendant into a scratch row, any other is skipped.  A child reads its parent's dword of
// the same 16 sites: from the lane's register when the parent is the previous node, else from the row the lane itself wrote
// (one writer per element, no atomics, no LDS).  A node's record and its twelve threshold words are uniform across the
// wavefront: scalar loads into scalar registers (SimThr), a site's two thresholds chosen from them by compare and select.
// One H call serves four sites; Lw decides a site only where H[k & 3] equals the high word of one of its two thresholds,
// so the Lw call is made only for a quad in which some site ties (kLazy) — the same law at half the Philox work.
//
// THE OBSERVATION LAW.  What a caller of methylation states sees of a true state: another state (a miscall) or nothing
// (a call below the posterior filter, which the reference drops per pair, src/pedigree.rs:249-251).  othr is uint64 [3][3],
// each row non-decreasing.  For the emitted row of node v, site k, true state s in {0, 1, 2}: the draw w(k, v) is built
// exactly as u(k, v) with c3 = kTagObs = 6; c2 = v is the NODE's index, not the row's, so emit still only selects rows.
//   observed field = (w >= othr[s][0]) + (w >= othr[s][1]) + (w >= othr[s][2]); the field 3 is "filtered"
// An input field that already is 3 (the padding behind the last site, or anything else) stays 3; the fields from site L
// to the end of abn_packed_row_stride(L) bytes are written as 3; bytes beyond abn_packed_row_stride(L) of a row are
// neither read nor written.  Refused before any launch (sim_observe_refusal): null pointers, fewer than 1 or more than
// 65535 rows, a node_of_row outside 0..65534, a decreasing othr row, L < 0 or L > 2^34, a stride outside the rule above, an
// input and an output that overlap other than in place (the same pointer and the same stride).
//
// OBSERVATION THRESHOLDS (sim_obs_thresholds; host only).  miscall[3][3]: row s the probabilities that a kept call of a
// true state s reads 0, 1, 2 (each row sums to 1 within 1e-12); dropout[3]: the probability that a call of a true state s
// is filtered.  With q = 1 - dropout[s]: c0 = q m[s][0], c1 = q (m[s][0] + m[s][1]), c2 = q; each through threshold(c);
// then t1 = max(t1, t0), t2 = max(t2, t1).
//
// THE OBSERVATION KERNEL.  One lane owns one dword of one row; the rows lie on blockIdx.y, x is grid-strided with
// sim_grid_blocks as the simulation is.  One H call per quad serves four sites; the Lw call is made only for a quad in
// which some site's H equals the high word of one of its three thresholds (kLazy; the argument above).  The eighteen
// threshold words are kernel arguments (ObsThr: a member each, no indexed array), the row's node one scalar load.  One
// writer per element, no atomics, no LDS, no scratch memory; in place the lane reads its dword before it writes it.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "abn_philox.h"

namespace abn {

constexpr int32_t kSimMaxNodes = 65535;
constexpr int64_t kSimMaxSites = (int64_t)1 << 34;
constexpr int kSimThreads = 256;
constexpr int kSimBlocksPerCu = 4;
constexpr int32_t kSimSkip = INT32_MIN;  // SimNode::slot of a node without an emitted descendant

struct SimNode {
  int32_t parent;  // -1: the founder
  int32_t slot;    // >= 0: the emitted row; < 0: scratch row ~slot; kSimSkip
};

inline int64_t sim_row_bytes(int64_t n_sites) { return n_sites <= 0 ? 0 : (n_sites + 255) / 256 * 64; }  // abn_packed_row_stride
// workgroups of the launch over `dwords` dwords of a row on `cus` compute units
inline int64_t sim_grid_blocks(int64_t dwords, int cus) {
  const int64_t want = (dwords + kSimThreads - 1) / kSimThreads, cap = (int64_t)(cus > 0 ? cus : 1) * kSimBlocksPerCu;
  return want < 1 ? 1 : (want < cap ? want : cap);
}

// ------------------------------------------------------------------------------------------------ the law
ABN_HD uint64_t sim_draw(uint64_t seed, uint64_t k, uint32_t v) {
  uint32_t h[4], l[4];
  philox4x32_10((uint32_t)(k >> 2), 0u, v, kTagSim, (uint32_t)seed, (uint32_t)(seed >> 32), h);
  philox4x32_10((uint32_t)(k >> 2), 1u, v, kTagSim, (uint32_t)seed, (uint32_t)(seed >> 32), l);
  return ((uint64_t)h[k & 3] << 32) | l[k & 3];
}
ABN_HD uint32_t sim_state(uint64_t u, uint64_t t0, uint64_t t1) { return (uint32_t)(u >= t0) + (uint32_t)(u >= t1); }
// thr[v][0..2][0..1] of one node as twelve words, each a member of its own: hi / lo of threshold 0 (a) and 1 (b) under the
// parent states 0, 1, 2.  No array: the selection by the parent's state stays a select between registers (an indexed
// private array becomes a per-lane table in LDS or scratch)
struct SimThr {
  uint32_t a0h, a0l, b0h, b0l, a1h, a1l, b1h, b1l, a2h, a2l, b2h, b2l;
};
ABN_HD SimThr sim_thr(const uint64_t* t) {
  return SimThr{(uint32_t)(t[0] >> 32), (uint32_t)t[0], (uint32_t)(t[1] >> 32), (uint32_t)t[1], (uint32_t)(t[2] >> 32), (uint32_t)t[2],
                (uint32_t)(t[3] >> 32), (uint32_t)t[3], (uint32_t)(t[4] >> 32), (uint32_t)t[4], (uint32_t)(t[5] >> 32), (uint32_t)t[5]};
}
ABN_HD uint32_t sim_pick(uint32_t s, uint32_t x0, uint32_t x1, uint32_t x2) { return s == 0u ? x0 : (s == 1u ? x1 : x2); }
// the fields of a dword from its n_valid-th site on, all 3: site i = 4 j + e lies at bits 8 e + 2 j
ABN_HD uint32_t sim_pad_mask(int n_valid) {
  if (n_valid >= 16) return 0u;
  const int j0 = n_valid >> 2, e0 = n_valid & 3;
  const uint32_t above = ((0xffu << (2 * (j0 + 1))) & 0xffu) * 0x01010101u;  // every e of the quads j > j0
  return above | ((0x03030303u << (8 * e0)) << (2 * j0));                   // e >= e0 of quad j0
}

// The dword g of node v from its parent's dword (ignored for the founder): fields of sites 16 g + 4 j + e at bits
// 8 e + 2 j; every field from the dword's n_valid-th site on is 3.  A parent field of 3 (behind the last site) reads the
// thresholds of state 2; its field is masked.
template <bool kLazy>
ABN_HD uint32_t sim_lane_dword(uint64_t seed, uint32_t v, uint64_t g, const SimThr t, bool founder, uint32_t parent_dword,
                               int n_valid) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t out = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t c0 = (uint32_t)(4 * g + (uint64_t)j);
    uint32_t h[4];
    philox4x32_10(c0, 0u, v, kTagSim, k0, k1, h);
    uint32_t s[4], ah[4], bh[4];
    bool tie = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] = founder ? 0u : (parent_dword >> (8 * e + 2 * j)) & 3u;
      ah[e] = sim_pick(s[e], t.a0h, t.a1h, t.a2h);
      bh[e] = sim_pick(s[e], t.b0h, t.b1h, t.b2h);
      tie = tie || h[e] == ah[e] || h[e] == bh[e];
    }
    uint32_t state[4];
    if (!kLazy || tie) {  // the low words decide
      uint32_t l[4];
      philox4x32_10(c0, 1u, v, kTagSim, k0, k1, l);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        state[e] = sim_state(((uint64_t)h[e] << 32) | l[e], ((uint64_t)ah[e] << 32) | sim_pick(s[e], t.a0l, t.a1l, t.a2l),
                             ((uint64_t)bh[e] << 32) | sim_pick(s[e], t.b0l, t.b1l, t.b2l));
    } else {  // no high word equals a threshold's: u >= t exactly when H > the threshold's high word
#pragma unroll
      for (int e = 0; e < 4; ++e) state[e] = (uint32_t)(h[e] > ah[e]) + (uint32_t)(h[e] > bh[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) out |= state[e] << (8 * e + 2 * j);
  }
  return out | sim_pad_mask(n_valid);  // a state is at most 2: or-ing 3 over it gives 3
}

// ------------------------------------------------------------------------------------------------ the arguments
// "" or why the arguments are refused; out == nullptr: the output and its stride are not part of the call
inline std::string sim_refusal(int64_t V, const int32_t* parent, const uint64_t* thr, const uint8_t* emit, int64_t n_sites,
                               const void* out, int64_t row_stride, bool with_out = true) {
  if (!parent || !thr || !emit || (with_out && !out)) return "abn_sim_codes: a null pointer";
  if (V < 1) return "abn_sim_codes: fewer than one node";
  if (V > kSimMaxNodes) return "abn_sim_codes: more than 65535 nodes";
  if (n_sites < 0 || n_sites > kSimMaxSites) return "abn_sim_codes: n_sites below 0 or above 2^34";
  if (parent[0] != -1) return "abn_sim_codes: parent[0] is not -1";
  for (int64_t v = 1; v < V; ++v)
    if (parent[v] < 0 || parent[v] >= v)
      return "abn_sim_codes: parent[" + std::to_string(v) + "] is not a node in front of it";
  for (int64_t i = 0; i < 3 * V; ++i)
    if (thr[2 * i] > thr[2 * i + 1])
      return "abn_sim_codes: thr[" + std::to_string(i / 3) + "][" + std::to_string(i % 3) + "][0] lies above its [1]";
  bool any = false;
  for (int64_t v = 0; v < V; ++v) any = any || emit[v] != 0;
  if (!any) return "abn_sim_codes: no emitted node";
  if (with_out && (row_stride < 0 || row_stride % 64 != 0 || row_stride < sim_row_bytes(n_sites)))
    return "abn_sim_codes: a row_stride that is not a multiple of 64 or is below abn_packed_row_stride(n_sites)";
  return "";
}

// The node records of valid arguments: the emitted rows in node order, a scratch row for every unemitted node with an
// emitted descendant, kSimSkip for the rest
struct SimPlan {
  std::vector<SimNode> nodes;
  int32_t n_emit = 0, n_scratch = 0;
};
inline SimPlan sim_plan(int32_t V, const int32_t* parent, const uint8_t* emit) {
  SimPlan p;
  p.nodes.resize((size_t)V);
  std::vector<uint8_t> live((size_t)V, 0);
  for (int32_t v = V - 1; v >= 0; --v) {
    if (emit[v]) live[(size_t)v] = 1;
    if (live[(size_t)v] && v > 0) live[(size_t)parent[v]] = 1;
  }
  for (int32_t v = 0; v < V; ++v) {
    p.nodes[(size_t)v].parent = parent[v];
    p.nodes[(size_t)v].slot = emit[v] ? p.n_emit++ : (live[(size_t)v] ? ~(p.n_scratch++) : kSimSkip);
  }
  return p;
}

// ------------------------------------------------------------------------------------------------ the serial forms
// The law site by site into out[n_emit x row_stride] (valid arguments): state[v] of one site at a time
inline void sim_codes_serial(uint64_t seed, int32_t V, const int32_t* parent, const uint64_t* thr, const uint8_t* emit,
                             int64_t n_sites, uint8_t* out, int64_t row_stride) {
  const int64_t row_bytes = sim_row_bytes(n_sites);
  int64_t rows = 0;
  for (int32_t v = 0; v < V; ++v) rows += emit[v] != 0;
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t b = 0; b < row_bytes; ++b) out[r * row_stride + b] = 0xff;
  std::vector<uint8_t> state((size_t)V);
  for (int64_t k = 0; k < n_sites; ++k) {
    int64_t r = 0;
    for (int32_t v = 0; v < V; ++v) {
      const uint64_t* t = thr + 6 * (size_t)v + 2 * (size_t)(v == 0 ? 0 : state[(size_t)parent[v]]);
      state[(size_t)v] = (uint8_t)sim_state(sim_draw(seed, (uint64_t)k, (uint32_t)v), t[0], t[1]);
      if (!emit[v]) continue;
      out[r * row_stride + (k >> 4) * 4 + (k & 3)] ^= (uint8_t)((3u ^ state[(size_t)v]) << (2 * ((k >> 2) & 3)));  // the field was 3
      ++r;
    }
  }
}

// One lane's trip of the kernel at dword g of the row: the nodes in index order.  `out` and `scratch` are the kernel's
// (dwords addressed through byte strides); row_dwords = sim_row_bytes(L) / 4.
template <bool kLazy>
ABN_HD void sim_lane_trip(uint64_t seed, int32_t V, const SimNode* nodes, const uint64_t* thr, int64_t n_sites, int64_t g,
                          uint8_t* out, int64_t row_stride, uint8_t* scratch, int64_t scratch_stride) {
  const int64_t left = n_sites - 16 * g;  // <= 0: a dword of padding
  const int n_valid = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
  uint32_t prev = 0;  // the dword of node v - 1 (a skipped node leaves it; nothing reads it then)
  for (int32_t v = 0; v < V; ++v) {
    const SimNode nd = nodes[v];
    if (nd.slot == kSimSkip) continue;
    uint32_t dw = 0xffffffffu;
    if (n_valid > 0) {
      uint32_t pd = prev;
      if (nd.parent >= 0 && nd.parent != v - 1) {
        const int32_t ps = nodes[nd.parent].slot;  // live: it has this live child
        const uint8_t* row = ps >= 0 ? out + (int64_t)ps * row_stride : scratch + (int64_t)~ps * scratch_stride;
        pd = *reinterpret_cast<const uint32_t*>(row + 4 * g);
      }
      dw = sim_lane_dword<kLazy>(seed, (uint32_t)v, (uint64_t)g, sim_thr(thr + 6 * (size_t)v), nd.parent < 0, pd, n_valid);
    }
    prev = dw;
    if (nd.slot >= 0) *reinterpret_cast<uint32_t*>(out + (int64_t)nd.slot * row_stride + 4 * g) = dw;
    else if (n_valid > 0) *reinterpret_cast<uint32_t*>(scratch + (int64_t)~nd.slot * scratch_stride + 4 * g) = dw;
  }
}

// The kernel's structure walked on the host: `blocks` workgroups of kSimThreads lanes, every lane grid-strided over the
// row's dwords.  scratch: n_scratch rows of sim_row_bytes(L) bytes
template <bool kLazy>
inline void sim_codes_walk(uint64_t seed, int32_t V, const SimNode* nodes, const uint64_t* thr, int64_t n_sites, int64_t blocks,
                           uint8_t* out, int64_t row_stride, uint8_t* scratch) {
  const int64_t row_dwords = sim_row_bytes(n_sites) / 4, lanes = blocks * kSimThreads;
  for (int64_t lane = 0; lane < lanes; ++lane)
    for (int64_t g = lane; g < row_dwords; g += lanes)
      sim_lane_trip<kLazy>(seed, V, nodes, thr, n_sites, g, out, row_stride, scratch, sim_row_bytes(n_sites));
}

// ------------------------------------------------------------------------------------------------ thresholds from rates
inline uint64_t sim_threshold(double c) {
  if (!(c > 0.0)) return 0;
  if (c >= 1.0) return ~(uint64_t)0;
  return (uint64_t)ldexp(c, 64);
}
inline void sim_genmatrix(double alpha, double beta, double G[9]) {  // src/divergence.rs:96-114
  G[0] = (1.0 - alpha) * (1.0 - alpha);
  G[1] = 2.0 * (1.0 - alpha) * alpha;
  G[2] = alpha * alpha;
  G[3] = 0.25 * ((beta + 1.0 - alpha) * (beta + 1.0 - alpha));
  G[4] = 0.5 * (beta + 1.0 - alpha) * (alpha + 1.0 - beta);
  G[5] = 0.25 * ((alpha + 1.0 - beta) * (alpha + 1.0 - beta));
  G[6] = beta * beta;
  G[7] = 2.0 * (1.0 - beta) * beta;
  G[8] = (1.0 - beta) * (1.0 - beta);
}
// "" or the refusal; thr[V][3][2].  The power table G^0 .. G^127 is the reference's chain result = result.dot(matrix)
// (src/divergence.rs:25-30), every dot product fused and accumulated from 0 in ascending k, as ndarray's is
inline std::string sim_thresholds(double alpha, double beta, double p_uu0, double weight, int64_t V, const int32_t* parent,
                                  const int32_t* generation, uint64_t* thr) {
  if (!parent || !generation || !thr) return "abn_sim_thresholds: a null pointer";
  if (V < 1) return "abn_sim_thresholds: fewer than one node";
  if (V > kSimMaxNodes) return "abn_sim_thresholds: more than 65535 nodes";
  const double rates[4] = {alpha, beta, p_uu0, weight};
  for (double r : rates)
    if (!(r >= 0.0 && r <= 1.0)) return "abn_sim_thresholds: alpha, beta, p_uu0 and weight lie in [0, 1]";
  if (parent[0] != -1) return "abn_sim_thresholds: parent[0] is not -1";
  int tmax = 0;
  for (int64_t v = 0; v < V; ++v) {
    if (v > 0 && (parent[v] < 0 || parent[v] >= v))
      return "abn_sim_thresholds: parent[" + std::to_string(v) + "] is not a node in front of it";
    if (generation[v] < 0 || generation[v] > 127)
      return "abn_sim_thresholds: generation[" + std::to_string(v) + "] lies outside 0..127";
    if (v > 0 && generation[v] < generation[parent[v]])
      return "abn_sim_thresholds: node " + std::to_string(v) + " is older than its parent";
    if (generation[v] > tmax) tmax = generation[v];
  }
  std::vector<double> tab((size_t)(tmax + 2) * 9, 0.0);
  tab[0] = tab[4] = tab[8] = 1.0;
  sim_genmatrix(alpha, beta, &tab[9]);
  for (int k = 2; k <= tmax; ++k)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double *R = &tab[(size_t)(k - 1) * 9], *M = &tab[9];
        double acc = 0.0;
        acc = __builtin_fma(R[3 * i + 0], M[0 + j], acc);
        acc = __builtin_fma(R[3 * i + 1], M[3 + j], acc);
        acc = __builtin_fma(R[3 * i + 2], M[6 + j], acc);
        tab[(size_t)k * 9 + 3 * i + j] = acc;
      }
  auto put = [](const double p[3], uint64_t* t) {
    t[0] = sim_threshold(p[0]);
    t[1] = sim_threshold(p[0] + p[1]);  // p[1] >= 0: never below t[0]
  };
  const double p_mm = 1.0 - p_uu0;
  const double sv0[3] = {p_uu0, weight * p_mm, (1.0 - weight) * p_mm};
  const double* P0 = &tab[(size_t)generation[0] * 9];
  double founder[3];
  for (int j = 0; j < 3; ++j) {
    double acc = 0.0;
    acc = __builtin_fma(sv0[0], P0[0 + j], acc);
    acc = __builtin_fma(sv0[1], P0[3 + j], acc);
    acc = __builtin_fma(sv0[2], P0[6 + j], acc);
    founder[j] = acc;
  }
  for (int s = 0; s < 3; ++s) put(founder, thr + 2 * s);  // (the law reads thr[0][0] alone)
  for (int64_t v = 1; v < V; ++v) {
    const double* P = &tab[(size_t)(generation[v] - generation[parent[v]]) * 9];
    for (int s = 0; s < 3; ++s) put(P + 3 * s, thr + 6 * v + 2 * s);
  }
  return "";
}

// The generation of the last common ancestor of nodes a and b
inline int32_t sim_common_generation(const int32_t* parent, const int32_t* generation, int32_t a, int32_t b) {
  while (a != b) {
    if (a > b) a = parent[a];
    else b = parent[b];
  }
  return generation[a];
}

// ------------------------------------------------------------------------------------------------ the observation step
ABN_HD uint64_t sim_obs_draw(uint64_t seed, uint64_t k, uint32_t v) {
  uint32_t h[4], l[4];
  philox4x32_10((uint32_t)(k >> 2), 0u, v, kTagObs, (uint32_t)seed, (uint32_t)(seed >> 32), h);
  philox4x32_10((uint32_t)(k >> 2), 1u, v, kTagObs, (uint32_t)seed, (uint32_t)(seed >> 32), l);
  return ((uint64_t)h[k & 3] << 32) | l[k & 3];
}
ABN_HD uint32_t sim_obs_field(uint64_t w, uint64_t t0, uint64_t t1, uint64_t t2) {
  return (uint32_t)(w >= t0) + (uint32_t)(w >= t1) + (uint32_t)(w >= t2);
}
// othr[0..2][0..2] as eighteen words, each a member of its own (SimThr's reason): hi / lo of the thresholds 0 (a), 1 (b)
// and 2 (c) under the true states 0, 1, 2.  A kernel argument: the words arrive in scalar registers
struct ObsThr {
  uint32_t a0h, a0l, b0h, b0l, c0h, c0l, a1h, a1l, b1h, b1l, c1h, c1l, a2h, a2l, b2h, b2l, c2h, c2l;
};
inline ObsThr sim_obs_thr(const uint64_t* t) {
  auto hi = [&](int i) { return (uint32_t)(t[i] >> 32); };
  auto lo = [&](int i) { return (uint32_t)t[i]; };
  return ObsThr{hi(0), lo(0), hi(1), lo(1), hi(2), lo(2), hi(3), lo(3), hi(4), lo(4), hi(5), lo(5),
                hi(6), lo(6), hi(7), lo(7), hi(8), lo(8)};
}

// The observed dword g of the row of node v from its true dword: fields of sites 16 g + 4 j + e at bits 8 e + 2 j; an
// input field of 3 stays 3 (it reads the thresholds of state 2; its field is set afterwards), and so does every field
// from the dword's n_valid-th site on.
template <bool kLazy>
ABN_HD uint32_t sim_obs_lane_dword(uint64_t seed, uint32_t v, uint64_t g, const ObsThr t, uint32_t in, int n_valid) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t out = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t c0 = (uint32_t)(4 * g + (uint64_t)j);
    uint32_t h[4];
    philox4x32_10(c0, 0u, v, kTagObs, k0, k1, h);
    uint32_t s[4], ah[4], bh[4], ch[4];
    bool tie = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] = (in >> (8 * e + 2 * j)) & 3u;
      ah[e] = sim_pick(s[e], t.a0h, t.a1h, t.a2h);
      bh[e] = sim_pick(s[e], t.b0h, t.b1h, t.b2h);
      ch[e] = sim_pick(s[e], t.c0h, t.c1h, t.c2h);
      tie = tie || h[e] == ah[e] || h[e] == bh[e] || h[e] == ch[e];
    }
    uint32_t field[4];
    if (!kLazy || tie) {  // the low words decide
      uint32_t l[4];
      philox4x32_10(c0, 1u, v, kTagObs, k0, k1, l);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        field[e] = sim_obs_field(((uint64_t)h[e] << 32) | l[e], ((uint64_t)ah[e] << 32) | sim_pick(s[e], t.a0l, t.a1l, t.a2l),
                                 ((uint64_t)bh[e] << 32) | sim_pick(s[e], t.b0l, t.b1l, t.b2l),
                                 ((uint64_t)ch[e] << 32) | sim_pick(s[e], t.c0l, t.c1l, t.c2l));
    } else {  // no high word equals a threshold's: w >= t exactly when H > the threshold's high word
#pragma unroll
      for (int e = 0; e < 4; ++e) field[e] = (uint32_t)(h[e] > ah[e]) + (uint32_t)(h[e] > bh[e]) + (uint32_t)(h[e] > ch[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) out |= field[e] << (8 * e + 2 * j);
  }
  const uint32_t was3 = in & (in >> 1) & 0x55555555u;  // bit 2 i of every input field i that is 3
  return out | was3 | (was3 << 1) | sim_pad_mask(n_valid);  // a field is at most 3: or-ing 3 over it gives 3
}

// "" or why the arguments of abn_sim_observe* are refused
inline std::string sim_observe_refusal(int64_t n_rows, const int32_t* node_of_row, const uint64_t* othr, int64_t n_sites,
                                       const void* in, int64_t in_stride, const void* out, int64_t out_stride) {
  if (!node_of_row || !othr || !in || !out) return "abn_sim_observe: a null pointer";
  if (n_rows < 1) return "abn_sim_observe: fewer than one row";
  if (n_rows > kSimMaxNodes) return "abn_sim_observe: more than 65535 rows";
  for (int64_t r = 0; r < n_rows; ++r)
    if (node_of_row[r] < 0 || node_of_row[r] >= kSimMaxNodes)
      return "abn_sim_observe: node_of_row[" + std::to_string(r) + "] lies outside 0..65534";
  for (int s = 0; s < 3; ++s)
    if (othr[3 * s] > othr[3 * s + 1] || othr[3 * s + 1] > othr[3 * s + 2])
      return "abn_sim_observe: othr[" + std::to_string(s) + "] decreases";
  if (n_sites < 0 || n_sites > kSimMaxSites) return "abn_sim_observe: n_sites below 0 or above 2^34";
  for (int64_t stride : {in_stride, out_stride})
    if (stride < 0 || stride % 64 != 0 || stride < sim_row_bytes(n_sites))
      return "abn_sim_observe: a row_stride that is not a multiple of 64 or is below abn_packed_row_stride(n_sites)";
  if (!(in == out && in_stride == out_stride) && n_sites > 0) {
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (uintptr_t)((n_rows - 1) * in_stride + sim_row_bytes(n_sites));
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uintptr_t)((n_rows - 1) * out_stride + sim_row_bytes(n_sites));
    if (a0 < b1 && b0 < a1) return "abn_sim_observe: the input and the output overlap other than in place";
  }
  return "";
}

// The law site by site (valid arguments): row r of `in` observed into row r of `out`
inline void sim_observe_serial(uint64_t seed, int64_t n_rows, const int32_t* node_of_row, const uint64_t* othr, int64_t n_sites,
                               const uint8_t* in, int64_t in_stride, uint8_t* out, int64_t out_stride) {
  const int64_t row_bytes = sim_row_bytes(n_sites);
  for (int64_t r = 0; r < n_rows; ++r) {
    const uint8_t* src = in + r * in_stride;
    uint8_t* dst = out + r * out_stride;
    for (int64_t k = 0; k < 4 * row_bytes; ++k) {
      const int64_t at = (k >> 4) * 4 + (k & 3);
      const int shift = 2 * (int)((k >> 2) & 3);
      const uint32_t s = (src[at] >> shift) & 3u;
      uint32_t f = 3u;
      if (k < n_sites && s != 3u) {
        const uint64_t* t = othr + 3 * s;
        f = sim_obs_field(sim_obs_draw(seed, (uint64_t)k, (uint32_t)node_of_row[r]), t[0], t[1], t[2]);
      }
      dst[at] = (uint8_t)((dst[at] & ~(3u << shift)) | (f << shift));  // (in place: the field read above is this one)
    }
  }
}

// One lane's trip of the observation kernel: the dword g of row r
template <bool kLazy>
ABN_HD void sim_obs_lane_trip(uint64_t seed, uint32_t v, const ObsThr t, int64_t n_sites, int64_t g, const uint8_t* in_row,
                              uint8_t* out_row) {
  const int64_t left = n_sites - 16 * g;
  const int n_valid = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
  const uint32_t x = *reinterpret_cast<const uint32_t*>(in_row + 4 * g);
  *reinterpret_cast<uint32_t*>(out_row + 4 * g) = sim_obs_lane_dword<kLazy>(seed, v, (uint64_t)g, t, x, n_valid);
}

// The observation kernel's structure walked on the host: rows on y, `blocks` workgroups of kSimThreads lanes on x, every
// lane grid-strided over the row's dwords
template <bool kLazy>
inline void sim_observe_walk(uint64_t seed, int64_t n_rows, const int32_t* node_of_row, const uint64_t* othr, int64_t n_sites,
                             int64_t blocks, const uint8_t* in, int64_t in_stride, uint8_t* out, int64_t out_stride) {
  const int64_t row_dwords = sim_row_bytes(n_sites) / 4, lanes = blocks * kSimThreads;
  const ObsThr t = sim_obs_thr(othr);
  for (int64_t r = 0; r < n_rows; ++r)
    for (int64_t lane = 0; lane < lanes; ++lane)
      for (int64_t g = lane; g < row_dwords; g += lanes)
        sim_obs_lane_trip<kLazy>(seed, (uint32_t)node_of_row[r], t, n_sites, g, in + r * in_stride, out + r * out_stride);
}

// "" or the refusal; othr[3][3] from miscall[3][3] and dropout[3]
inline std::string sim_obs_thresholds(const double* miscall, const double* dropout, uint64_t* othr) {
  if (!miscall || !dropout || !othr) return "abn_sim_obs_thresholds: a null pointer";
  for (int i = 0; i < 9; ++i)
    if (!(miscall[i] >= 0.0 && miscall[i] <= 1.0)) return "abn_sim_obs_thresholds: miscall and dropout lie in [0, 1]";
  for (int s = 0; s < 3; ++s)
    if (!(dropout[s] >= 0.0 && dropout[s] <= 1.0)) return "abn_sim_obs_thresholds: miscall and dropout lie in [0, 1]";
  for (int s = 0; s < 3; ++s) {
    const double* m = miscall + 3 * s;
    const double sum = (m[0] + m[1]) + m[2];
    if (!(fabs(sum - 1.0) <= 1e-12)) return "abn_sim_obs_thresholds: miscall[" + std::to_string(s) + "] does not sum to 1";
    const double q = 1.0 - dropout[s];
    uint64_t* t = othr + 3 * s;
    t[0] = sim_threshold(q * m[0]);
    t[1] = sim_threshold(q * (m[0] + m[1]));
    t[2] = sim_threshold(q);
    if (t[1] < t[0]) t[1] = t[0];
    if (t[2] < t[1]) t[2] = t[1];
  }
  return "";
}

#if defined(__HIPCC__) && defined(ABN_SIM_KERNELS)  // (abn_sim.hip defines it)
// grid: (sim_grid_blocks(row_dwords, cus), n_rows) workgroups of kSimThreads lanes.  Bounds: g < row_dwords = sim_row_bytes(L)
// / 4, so a row's reads and writes end at sim_row_bytes(L) <= both strides; blockIdx.y < n_rows.
template <bool kLazy>
__global__ void __launch_bounds__(kSimThreads)
abn_sim_observe_kernel(uint64_t seed, const int32_t* __restrict__ node_of_row, const ObsThr t, int64_t n_sites, int64_t row_dwords,
                       const uint8_t* in, int64_t in_stride, uint8_t* out, int64_t out_stride) {
  const uint32_t v = (uint32_t)node_of_row[blockIdx.y];
  const uint8_t* in_row = in + (int64_t)blockIdx.y * in_stride;
  uint8_t* out_row = out + (int64_t)blockIdx.y * out_stride;
  const int64_t lanes = (int64_t)gridDim.x * kSimThreads;
  for (int64_t g = (int64_t)blockIdx.x * kSimThreads + threadIdx.x; g < row_dwords; g += lanes)
    sim_obs_lane_trip<kLazy>(seed, v, t, n_sites, g, in_row, out_row);
}

// grid: sim_grid_blocks(row_dwords, cus) workgroups of kSimThreads lanes.  Bounds: g < row_dwords = sim_row_bytes(L) / 4, so a
// row's writes end at sim_row_bytes(L) <= row_stride; slots are below n_emit and n_scratch by sim_plan.
template <bool kLazy>
__global__ void __launch_bounds__(kSimThreads)
abn_sim_codes_kernel(uint64_t seed, int32_t V, const SimNode* __restrict__ nodes, const uint64_t* __restrict__ thr, int64_t n_sites,
                     int64_t row_dwords, uint8_t* out, int64_t row_stride, uint8_t* scratch, int64_t scratch_stride) {
  const int64_t lanes = (int64_t)gridDim.x * kSimThreads;
  for (int64_t g = (int64_t)blockIdx.x * kSimThreads + threadIdx.x; g < row_dwords; g += lanes)
    sim_lane_trip<kLazy>(seed, V, nodes, thr, n_sites, g, out, row_stride, scratch, scratch_stride);
}
#endif

}  // namespace abn
