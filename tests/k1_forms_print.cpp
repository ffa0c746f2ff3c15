// k1_forms_print.cpp — prints what kmcp_amd/csrc/k1_plan.hpp decides for the shapes of tests/k1_forms_plan.py's cases, one line in, one
// line out.  In: id mode k w_or_s paired n_reads max_read_len dedup_threshold flags wr_waves packed n_exc n_bases.  The batches are those
// of the K1-alone entry points: scratch is there, a packed batch's text buffer is where the kernels read text, no windows.
// Built and run by tests/test_k1_forms_plan_cpu.py.
#include <stdio.h>

#include "../kmcp_amd/csrc/k1_plan.hpp"

using namespace kmcpg;

int main() {
  char id[128];
  int mode, k, paired, flags, wr_waves, packed;
  unsigned ws, n_reads, max_read_len, n_exc;
  int dedup;
  unsigned long long n_bases;
  static const char* const names[] = {"None", "WinOnce", "SegRoll2", "SegRoll", "SegHash", "WindowsRoll", "WindowsWave", "WgGlobal", "Wg", "Short"};
  while (scanf("%127s %d %d %u %d %u %u %d %d %d %d %u %llu", id, &mode, &k, &ws, &paired, &n_reads, &max_read_len, &dedup, &flags, &wr_waves, &packed, &n_exc,
               &n_bases) == 13) {
    K1Shape s;
    s.mode = mode;
    s.k = k;
    s.w_or_s = ws;
    s.paired = paired != 0;
    s.n_reads = n_reads;
    s.max_read_len = max_read_len;
    s.have_scratch = true;
    s.dedup_threshold = dedup;
    s.knobs.flags = flags;
    s.knobs.wr_waves = wr_waves;
    s.packed.present = packed != 0;
    s.packed.n_exc = n_exc;
    s.packed.n_bases = n_bases;
    s.packed.text_is_seqs = true;
    const K1Plan p = k1_plan(s);
    printf("%s %s %d %d %u %u %zu %d %d %d %u %d\n", id, names[(int)p.form], p.wsz, p.waves, p.grid, p.grid2, p.lds_bytes, (int)p.codes_direct, (int)p.list_fallback,
           (int)p.adj_done, p.segs, (int)(p.marks.len != 0));
  }
  return 0;
}
