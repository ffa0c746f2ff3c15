// recount_format.hpp — the file that stage 3 writes (kmcp_amd/csrc/recount_rule.hpp): one formatter for kmcp-refstats --recount and every
// other command that ends with the recounted references, so that their files are equal byte for byte.
//
//   # recounted reads: N        reads with at least one kept target
//   # unique reads: U           reads that ended with one target
//   # corrected reads: C        reads that lost at least one target to the correction
//   #ref chunks tLen reads ureads hicUreads chunksFrac depthStdev coverage verdict chunkReads chunkUreads chunkHicUreads chunkBases
// one line per reference with at least one add, in ascending byte order of the name.  Counts are printed from the integers as %.6f
// (units / 720720), bases as %.4f (units / 2^16); the four per-chunk lists are comma-joined.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../kmcp_amd/csrc/recount_rule.hpp"
#include "tsv_out.hpp"

namespace recount_format {

struct Ref {
  const std::string* name;
  uint64_t chunks, tlen;
  const uint64_t* counters;  // RECOUNT_WORDS per chunk
};

inline void write(tsv_out::Out& out, std::vector<Ref> refs, uint64_t recounted, uint64_t unique, uint64_t corrected, const kmcpg::RecountThresholds& th) {
  using namespace kmcpg;
  char line[256];
  out.write(line, (size_t)snprintf(line, sizeof line, "# recounted reads: %llu\n# unique reads: %llu\n# corrected reads: %llu\n", (unsigned long long)recounted,
                                   (unsigned long long)unique, (unsigned long long)corrected));
  out.write("#ref\tchunks\ttLen\treads\tureads\thicUreads\tchunksFrac\tdepthStdev\tcoverage\tverdict\tchunkReads\tchunkUreads\tchunkHicUreads\tchunkBases\n");
  std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) { return *a.name < *b.name; });
  std::string s;
  for (const Ref& r : refs) {
    const uint64_t* w = r.counters;
    const RecountRef t = recount_rollup(r.chunks, r.tlen, th, [&](uint64_t c) { return w + c * RECOUNT_WORDS; });
    if (!t.listed) continue;
    const double unit = (double)RECOUNT_UNIT;
    s = *r.name;
    s.append(line, (size_t)snprintf(line, sizeof line, "\t%llu\t%llu\t%.6f\t%.6f\t%.6f\t%.4f\t%.6f\t%.6f\t%s", (unsigned long long)r.chunks, (unsigned long long)r.tlen,
                                    (double)t.match / unit, (double)t.uniq / unit, (double)t.hic / unit, t.chunks_frac, t.depth_stdev, t.coverage,
                                    recount_verdict_name(t.verdict)));
    static const int words[4] = {RECOUNT_MATCH, RECOUNT_UNIQ, RECOUNT_HIC, RECOUNT_BASES};
    for (int j : words)
      for (uint64_t c = 0; c < r.chunks; c++) {
        s.push_back(c ? ',' : '\t');
        const uint64_t v = w[c * RECOUNT_WORDS + j];
        s.append(line, (size_t)(j == RECOUNT_BASES ? snprintf(line, sizeof line, "%.4f", (double)v / (double)RECOUNT_BASE_UNIT) : snprintf(line, sizeof line, "%.6f", (double)v / unit)));
      }
    s.push_back('\n');
    out.write(s);
  }
}

}  // namespace recount_format
