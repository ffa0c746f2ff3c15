// profile_format.hpp — the table that stage 4 ends with (kmcp_amd/csrc/em_rule.hpp): one formatter for kmcp-refstats --profile and
// kmcp-search --ref-stats-profile, so that their files are equal byte for byte.
//
//   # assigned reads: N         reads the last pass assigned
//   # passes: K                 passes made, the initialisation included
//   # converged: yes|no         the last pass moved the top percentage by less than --abund-pct-threshold
//   #ref percentage coverage chunksFrac chunksRelDepth chunksRelDepthStd reads ureads hicureads refsize
// one line per estimated reference, in the order of em_finish.  The column names and the formats are the reference's (profile.go:2860-2909):
// %.6f %.6f %.2f, the relative depths %.2f joined by ';', %.2f, three %.0f, %d.  The counts are the roll-up's integers / EM_UNIT.
#pragma once
#include <string>
#include <vector>

#include "../kmcp_amd/csrc/em_rule.hpp"
#include "tsv_out.hpp"

namespace profile_format {

inline void write(tsv_out::Out& out, const std::vector<kmcpg::EmClass>& classes, const kmcpg::EmResult& res, const std::vector<uint32_t>& order) {
  using namespace kmcpg;
  char line[256];
  out.write(line, (size_t)snprintf(line, sizeof line, "# assigned reads: %llu\n# passes: %d\n# converged: %s\n", (unsigned long long)res.assigned, res.passes, res.converged ? "yes" : "no"));
  out.write("#ref\tpercentage\tcoverage\tchunksFrac\tchunksRelDepth\tchunksRelDepthStd\treads\tureads\thicureads\trefsize\n");
  std::string s;
  const double unit = (double)EM_UNIT;
  for (const uint32_t c : order) {
    const EmRef& r = res.refs[c];
    s = classes[c].name;
    s.append(line, (size_t)snprintf(line, sizeof line, "\t%.6f\t%.6f\t%.2f\t", r.percentage, r.coverage, r.chunks_frac));
    for (size_t k = 0; k < r.rel_depth.size(); k++) {
      if (k) s.push_back(';');
      s.append(line, (size_t)snprintf(line, sizeof line, "%.2f", r.rel_depth[k]));
    }
    s.append(line, (size_t)snprintf(line, sizeof line, "\t%.2f\t%.0f\t%.0f\t%.0f\t%llu\n", r.depth_stdev, (double)r.match / unit, (double)r.uniq / unit, (double)r.hic / unit,
                                    (unsigned long long)classes[c].tlen));
    out.write(s);
  }
}

}  // namespace profile_format
