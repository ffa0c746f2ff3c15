// specific_rule.hpp — when a query's matches are "specific": the one rule behind kmcp-filter (cli/kmcp_filter.cpp), the library's host
// half (finalize.cpp) and the tests' stand-alone check (tests/specific_rule_check.cpp).  Host only; k4_specific.hip restates it.
//
// Reference counterpart: `kmcp utils filter` (kmcp/cmd/filter.go:306-391).  A query passes when its matches name ONE target, or, at
// --level species, when the LCA of its targets' TaxIds is at or below rank species.
//
// With species(t) = the nearest ancestor-or-self of t with rank species (0 if there is none, or t is unknown), the second condition is,
// in a tree, exactly "all targets have the same species(t), and it is not 0": if they share S != 0 the LCA lies at or below S; if the
// LCA lies at or below some species S', every target is under S'.  So every column carries two integers, fixed when the tables are made:
//   target_class   equal exactly when the printed target strings are equal (the chunks of one reference share it)
//   species_class  species(taxid of the target), or 0
// and a query is judged from the minimum and maximum of both over its matches.  A query without matches has no verdict.
#pragma once
#include <cstdint>

namespace kmcpg {

// the verdict byte of a read (include/kmcp_gpu.h: KMCPG_SPECIFIC_*)
constexpr uint8_t SPECIFIC_DROP = 0, SPECIFIC_KEEP = 1, SPECIFIC_HOST = 2;

struct SpecificAcc {
  uint32_t tmin = 0xffffffffu, tmax = 0, smin = 0xffffffffu, smax = 0;
  uint64_t n = 0;
  void add(uint32_t target_class, uint32_t species_class) {
    if (target_class < tmin) tmin = target_class;
    if (target_class > tmax) tmax = target_class;
    if (species_class < smin) smin = species_class;
    if (species_class > smax) smax = species_class;
    n++;
  }
};

// level_species: --level species; otherwise strain / assembly (one target only)
inline bool specific_keep(const SpecificAcc& a, bool level_species) {
  if (a.n == 0) return false;
  if (a.tmin == a.tmax) return true;
  return level_species && a.smin == a.smax && a.smin != 0;
}

}  // namespace kmcpg
