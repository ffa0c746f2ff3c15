// k2_forms_print.cpp — prints what kmcp_amd/csrc/k2_plan.hpp decides for the shapes of tests/k2_forms_plan.py's cases, one line in, one
// line out.  In: id stride num_hashes groups lpr8 lpr32 split_tiles n_reads max_n index_bytes listed max_long, then the per-query knobs
// split_min_set split_min split_chunk_set split_chunk prune group_rows_set group_rows prune_every slot_major pair.  `groups` groups of
// rows of `stride` bytes are cut into lane classes as finish_open does (k2_row_parts, classes in order of first appearance); listed /
// max_long are what the device would list above split_min, used only where k2_ask_long asks.
// Out: id ask classes (lpr:slots of one group, ...) forms (kind/lpr/lprb/npl/multi/gr in launch order).  Built and run by tests/test_k2_forms_plan_cpu.py.
#include <stdio.h>

#include <string>
#include <vector>

#include "../kmcp_amd/csrc/k2_plan.hpp"

using namespace kmcpg;

int main() {
  char id[128];
  unsigned stride, groups, n_reads, listed, max_long;
  int nh, lpr8, lpr32, split_tiles, sm_set, sm, sc_set, sc, prune, gr_set, gr, prune_every, slot_major, pair;
  unsigned long long max_n, index_bytes;
  while (scanf("%127s %u %d %u %d %d %d %u %llu %llu %u %u %d %d %d %d %d %d %d %d %d %d", id, &stride, &nh, &groups, &lpr8, &lpr32, &split_tiles, &n_reads, &max_n,
               &index_bytes, &listed, &max_long, &sm_set, &sm, &sc_set, &sc, &prune, &gr_set, &gr, &prune_every, &slot_major, &pair) == 22) {
    K2OpenKnobs ok;
    ok.lpr8 = lpr8 != 0;
    ok.lpr32 = lpr32 != 0;
    ok.split_tiles = split_tiles;
    K2Shape s;
    const K2RowParts parts = k2_row_parts(stride, nh, ok);
    for (unsigned g = 0; g < groups; g++)
      for (uint32_t i = 0; i < parts.size(); i++) {
        int c = 0;
        while (c < s.n_classes && s.classes[c].lpr != parts[i].lpr) c++;
        if (c == s.n_classes) s.classes[s.n_classes++].lpr = parts[i].lpr;
        s.classes[c].nslots++;
      }
    for (int c = 0; c < s.n_classes; c++)  // block units: a row that is whole 1-KiB tiles is one unit, any other tile one each
      if (s.classes[c].lpr == 64) s.classes[c].nbslots = parts.n_rem == 0 ? groups : s.classes[c].nslots;
    s.n_reads = n_reads;
    s.max_n = max_n;
    s.num_hashes = nh;
    s.matrix_bytes_local = index_bytes;
    s.n_cols = 1000;
    s.knobs.split_min_set = sm_set != 0;
    if (sm_set) s.knobs.split_min = sm;
    s.knobs.split_chunk_set = sc_set != 0;
    s.knobs.split_chunk = sc;
    s.knobs.prune = prune;
    s.knobs.group_rows_set = gr_set != 0;
    s.knobs.group_rows = gr;
    s.knobs.prune_every = prune_every;
    s.knobs.slot_major = slot_major;
    s.knobs.pair = pair != 0;
    const bool ask = k2_ask_long(s);
    const K2Plan p = k2_plan(s, ask, listed, max_long);
    std::vector<std::string> forms;
    static const char* const kinds[] = {"plain", "split", "pair"};
    for (int i = 0; i < p.n_launches; i++) {
      const K2Launch& l = p.launches[i];
      char buf[96];
      snprintf(buf, sizeof buf, "%s/%d/%d/%d/%d/%d", kinds[(int)l.kind], l.lpr, l.lprb, l.npl, (int)l.multi, l.gr);
      forms.push_back(buf);
    }
    printf("%s %d ", id, (int)ask);
    for (int c = 0; c < s.n_classes; c++) printf("%s%d:%u", c ? "," : "", s.classes[c].lpr, s.classes[c].nslots / groups);
    printf(" ");
    for (size_t i = 0; i < forms.size(); i++) printf("%s%s", i ? "," : "", forms[i].c_str());
    printf("%s\n", forms.empty() ? "-" : "");
  }
  return 0;
}
