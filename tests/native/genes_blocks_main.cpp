// Stand-alone driver for the gene choice in blocks (alphabeta_rs_amd/csrc/abn_genes.hpp), built by
// tests/test_genes_cpu.py with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded annotations and
// sites — sorted and unsorted, both strands and Unknown, nested and equal-keyed genes, coordinates at the top of u32 —
// through the three phases at several block lengths, every array in a heap block of exactly its length (a read or write
// past either end is a report), against the serial loop with its last-gene cache written out here.  No device.
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_genes.hpp"

static uint64_t rng_state = 20261018ull;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return n ? (uint32_t)(rng_state >> 33) % n : 0;
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap block of exactly v's length
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

int main() {
  size_t sites_total = 0, with_gene = 0;
  for (int it = 0; it < 400; ++it) {
    const uint32_t span = 1000u + rnd(100000), base = rnd(4) == 0 ? 0xffffffffu - span - 3000u : 0u;
    // the annotation: lists per (chromosome 0..2, kind), each stably sorted by start
    struct G {
      uint32_t start, end;
      uint8_t strand;
    };
    std::vector<G> lists[3][3];
    for (uint32_t k = rnd(60); k > 0; --k) {
      const uint32_t a = base + rnd(span), b = rnd(5) == 0 ? base + span / 2 : a + rnd(rnd(2) ? 50 : 5000);
      const G g{a, b, (uint8_t)rnd(3)};
      const uint32_t c = rnd(3);
      lists[c][2].push_back(g);
      if (g.strand < 2) lists[c][g.strand].push_back(g);
    }
    std::vector<uint32_t> off(abn::kGeneChromosomes * abn::kGeneKinds, 0), cnt(off.size(), 0), gstart, gend;
    std::vector<uint16_t> gchrom;
    std::vector<uint8_t> gstrand;
    for (int c = 0; c < 3; ++c)
      for (int kind = 0; kind < 3; ++kind) {
        auto& l = lists[c][kind];
        std::stable_sort(l.begin(), l.end(), [](const G& x, const G& y) { return x.start < y.start; });
        off[(size_t)(c * 3 + kind)] = (uint32_t)gstart.size();
        cnt[(size_t)(c * 3 + kind)] = (uint32_t)l.size();
        for (const G& g : l) gstart.push_back(g.start), gend.push_back(g.end), gstrand.push_back(g.strand), gchrom.push_back((uint16_t)c);
      }
    // the samples
    const int n_samples = 1 + (int)rnd(3);
    std::vector<int64_t> offset{0};
    std::vector<int32_t> chrom;
    std::vector<uint32_t> start, end;
    std::vector<uint8_t> strand;
    for (int s = 0; s < n_samples; ++s) {
      const uint32_t n = rnd(rnd(3) ? 60 : 2500);
      std::vector<uint32_t> pos(n);
      for (auto& p : pos) p = base + rnd(span + 3000);
      if (rnd(3)) std::sort(pos.begin(), pos.end());
      for (uint32_t i = 0; i < n; ++i) {
        chrom.push_back(rnd(10) ? 0 : (int32_t)rnd(4));  // chromosome 3 has no list
        start.push_back(pos[i]);
        const bool unknown = rnd(20) == 0;
        end.push_back(pos[i] + (unknown ? rnd(300) : 1u));
        strand.push_back(unknown ? 2 : (uint8_t)(rnd(2) ? i % 2 : rnd(2)));
      }
      offset.push_back((int64_t)start.size());
    }
    const size_t S = start.size();
    const abn::GeneRule rule{rnd(3) == 0 ? 0u : (rnd(2) ? 100u : 2048u), rnd(5) == 0};
    auto e_off = exact(off), e_cnt = exact(cnt), e_gs = exact(gstart), e_ge = exact(gend);
    auto e_gc = exact(gchrom);
    auto e_gd = exact(gstrand);
    auto e_c = exact(chrom);
    auto e_a = exact(start), e_z = exact(end);
    auto e_d = exact(strand);
    const abn::GeneTable T{e_off.get(), e_cnt.get(), e_gc.get(), e_gs.get(), e_ge.get(), e_gd.get()};
    const abn::GeneSites sites{e_c.get(), e_a.get(), e_z.get(), e_d.get()};
    // the serial loop (src/windows.rs:325-338)
    std::vector<uint32_t> want_s(S), want_e(S);
    std::vector<uint8_t> want_f(S);
    for (int s = 0; s < n_samples; ++s) {
      uint32_t last = abn::kGeneNone;
      for (int64_t i = offset[(size_t)s]; i < offset[(size_t)s + 1]; ++i) {
        if (last == abn::kGeneNone || !abn::gene_in(sites, i, T, last, rule)) last = abn::gene_find(sites, i, T, rule);
        abn::gene_output(strand[(size_t)i], T, last, want_s[(size_t)i], want_e[(size_t)i], want_f[(size_t)i]);
        with_gene += last != abn::kGeneNone;
      }
    }
    sites_total += S;
    for (int block : {1, 2, 3, 64, 1024}) {
      std::unique_ptr<uint32_t[]> F(new uint32_t[S]), gs(new uint32_t[S]), ge(new uint32_t[S]);
      std::unique_ptr<uint16_t[]> next(new uint16_t[S]), last(new uint16_t[S]);
      std::unique_ptr<uint8_t[]> fl(new uint8_t[S]);
      abn::genes_choose_blocked(sites, offset.data(), n_samples, T, rule, block, F.get(), next.get(), last.get(), gs.get(),
                                ge.get(), fl.get());
      if (S && (std::memcmp(gs.get(), want_s.data(), 4 * S) || std::memcmp(ge.get(), want_e.data(), 4 * S) ||
                std::memcmp(fl.get(), want_f.data(), S)))
        return std::printf("case %d differs at block length %d\n", it, block), 1;
    }
  }
  if (!sites_total || !with_gene || with_gene == sites_total) return std::printf("one outcome only\n"), 1;
  std::printf("sanitized gene blocks ok %zu %zu\n", sites_total, with_gene);
  return 0;
}
