// taxonomy.hpp — NCBI taxdump files and reference-to-TaxId maps, as far as "which species is this target under" needs them.  Host only.
//
// Reference counterpart: loadTaxonomy (kmcp/cmd/taxonomy.go:32-120: nodes.dmp, optional merged.dmp and delnodes.dmp) and the TaxId map
// reading of `kmcp utils filter` (filter.go:162-191: two-column files, later files override earlier ones).  The reference asks a
// third-party module for LCA and AtOrBelowRank; here the one question asked is species_of (specific_rule.hpp says why that is enough).
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace kmcpg {

struct Taxonomy {
  struct Node {
    uint32_t parent;
    bool species;  // rank == "species"
  };
  std::unordered_map<uint32_t, Node> nodes;
  std::unordered_map<uint32_t, uint32_t> merged;
  std::unordered_set<uint32_t> deleted;

  // dir/nodes.dmp (needed), dir/merged.dmp and dir/delnodes.dmp (when present).  false: *err says what went wrong
  bool load(const std::string& dir, std::string* err);
  // a merged TaxId -> its target (chains are followed); every other TaxId is returned as it is
  uint32_t resolve(uint32_t taxid) const;
  bool known(uint32_t taxid) const;  // after resolve: in nodes.dmp and not deleted
  // nearest ancestor-or-self with rank species; 0 when there is none or the TaxId is deleted or absent
  uint32_t species_of(uint32_t taxid) const;
};

// reference ID -> TaxId.  Lines with fewer than two tab-separated columns are skipped; a key seen again (in the same or a later file)
// takes the later value.  false: *err = "invalid TaxId: <text>" or the file error
struct TaxidMap {
  std::unordered_map<std::string, uint32_t> ids;
  bool load(const std::string& path, std::string* err);
};

// The per-target side of the rule (specific_rule.hpp) for a list of printed target names: classes[i] is shared exactly by equal
// names; species[i] = species_of(TaxId of names[i]) (filled only when tax and map are given).  *unknown_taxids counts the distinct
// mapped TaxIds that are deleted or absent from nodes.dmp (their species is 0).  false: *missing = the first name without a TaxId.
bool specific_classes(const std::vector<std::string>& names, const TaxidMap* map, const Taxonomy* tax, std::vector<uint32_t>* classes,
                      std::vector<uint32_t>* species, uint64_t* unknown_taxids, std::string* missing);

}  // namespace kmcpg
