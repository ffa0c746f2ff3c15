// k1_plan_check.cpp — host instantiation of kmcp_amd/csrc/k1_plan.hpp (which K1 kernels a batch gets): for every row of the table in
// DESIGN.md §4 one shape inside it and the shapes on either side of each boundary the row names, every KMCPG_K1_FLAGS bit alone and the
// combinations the GPU tests use, and over a sweep of shapes the invariants the launcher and run_kmers rely on.  The expected forms are
// written out here by hand, the LDS boundaries worked out in the comments.  Built and run by tests/test_k1_plan_cpu.py.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../kmcp_amd/csrc/k1_plan.hpp"

using namespace kmcpg;

static unsigned long long bad = 0, checked = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    checked++;                                                         \
    if (!(cond)) {                                                     \
      if (bad < 20) printf("line %d: %s\n", __LINE__, #cond);          \
      bad++;                                                           \
    }                                                                  \
  } while (0)

typedef K1Form F;

// plain k-mers (mode 0), k = 21, 1000 single reads, with scratch, -u 256
static K1Shape plain(uint32_t max_read_len, uint32_t n_reads = 1000) {
  K1Shape s;
  s.k = 21;
  s.n_reads = n_reads;
  s.max_read_len = max_read_len;
  s.have_scratch = true;
  s.dedup_threshold = 256;
  return s;
}
static K1Shape syncmer(int k, uint32_t sm, uint32_t max_read_len, uint32_t n_reads = 1000) {
  K1Shape s = plain(max_read_len, n_reads);
  s.mode = 2;
  s.k = k;
  s.w_or_s = sm;
  return s;
}
static K1Shape minimizer(int k, uint32_t w, uint32_t max_read_len) {
  K1Shape s = plain(max_read_len);
  s.mode = 1;
  s.k = k;
  s.w_or_s = w;
  return s;
}
static K1Shape with_flags(K1Shape s, int flags) {
  s.knobs.flags = flags;
  return s;
}
static K1Shape windows(K1Shape s, uint64_t step, uint64_t window, uint64_t sb = 50000, uint64_t n_chunks = 40) {
  s.win.present = true;
  s.win.step = step;
  s.win.window = window;
  s.win.sb = sb;
  s.win.n_chunks = n_chunks;
  return s;
}
// 4 genomes of up to 100 000 bases (2 segments each) as 2-bit codes, 409 600 bases in all: the run limit of codes_mode 1 is 409600 / 4096 + 64 = 164
static K1Shape packed(uint32_t n_exc, int codes_mode = 1) {
  K1Shape s = plain(100000, 4);
  s.packed.present = true;
  s.packed.n_exc = n_exc;
  s.packed.n_bases = 409600;
  s.packed.text_is_seqs = true;
  s.knobs.codes_mode = codes_mode;
  return s;
}
static F form(const K1Shape& s) { return k1_plan(s).form; }

// the regions tile [0, side_words) in the order counts, counter, list, marks
static bool tiles(const K1Plan& p) {
  size_t at = 0;
  for (const K1Region* r : {&p.counts, &p.counter, &p.list, &p.marks}) {
    if (!r->len) continue;
    if (r->off != at) return false;
    at += r->len;
  }
  return at == p.side_words;
}

static void invariants(const K1Shape& s) {
  const K1Plan p = k1_plan(s);
  CHECK(tiles(p));
  CHECK(!p.codes_direct || p.form == F::SegRoll2);
  CHECK(!p.list_fallback || (p.list.len > 0 && p.counter.len == 1 && p.grid2 > 0));
  CHECK(!p.list_fallback || p.form == F::SegRoll2 || p.form == F::WindowsRoll);
  CHECK((p.form == F::SegRoll2 || p.form == F::SegRoll || p.form == F::SegHash) == (p.segs > 1));
  CHECK(p.segs <= 1 || (p.counts.len == (size_t)s.n_reads * p.segs && p.grid == s.n_reads * p.segs && (uint64_t)p.grid <= (1ull << 21)));
  CHECK(!p.marks.len || (p.codes_direct && s.packed.n_exc > 0 && p.marks.len == p.counts.len));
  CHECK(p.form != F::SegRoll2 || p.list.len == p.counts.len);
  CHECK(p.form != F::WindowsRoll || (p.lds_bytes <= 65536 && (p.waves == 1 || p.waves == 2 || p.waves == 4) && p.list.len == s.n_reads &&
                                     p.grid == (s.n_reads + p.waves - 1) / p.waves && p.wsz == 2 * (s.k - (int)s.w_or_s)));
  CHECK(!p.adj_done || (s.mode != 0 && s.have_scratch));
  CHECK((p.form == F::None) == (s.n_reads == 0));
  CHECK(p.form == F::None || p.form == F::WinOnce || p.grid > 0);
  CHECK((p.form == F::WinOnce) == (p.win_words != 0));
  CHECK(p.form == F::WinOnce || p.form == F::None || s.max_read_len > 2048 || p.form == F::Short);
}

int main() {
  // ---- row 0: nothing to do
  {
    const K1Plan p = k1_plan(plain(150, 0));
    CHECK(p.form == F::None && !p.adj_done && p.side_words == 0 && !p.codes_direct);
    CHECK(form(windows(plain(500, 0), 100, 500)) == F::None);
    CHECK(form(plain(100000, 0)) == F::None);
  }
  // ---- row 1: overlapping windows of plain k-mers, hashed once
  {
    const K1Plan p = k1_plan(windows(plain(500), 100, 500));
    CHECK(p.form == F::WinOnce && p.grid == 10 && p.grid2 == 250 && p.win_words == 50001 && p.win_chunk_words == 41 && p.side_words == 0 && !p.adj_done);
    CHECK(k1_plan(windows(plain(500), 100, 500, 50000, 0)).grid == 0);  // no chunks: the gather alone
    CHECK(k1_plan(windows(plain(500), 100, 500, 50000, 0)).win_chunk_words == 1);
    CHECK(k1_plan(windows(plain(500, 400000), 100, 500, 1u << 30, 400000)).grid == 65536);
    CHECK(k1_plan(windows(plain(500, 400000), 100, 500, 1u << 30, 400000)).grid2 == 65536);
    K1Shape s = windows(plain(500), 100, 500);
    s.k = 65;
    CHECK(form(s) == F::WinOnce);
    s.k = 66;
    CHECK(form(s) == F::Short);
    CHECK(form(windows(plain(500), 499, 500)) == F::WinOnce);
    CHECK(form(windows(plain(500), 500, 500)) == F::Short);  // windows that do not overlap share no k-mer
    s = windows(plain(500), 100, 500);
    s.knobs.win_once = false;
    CHECK(form(s) == F::Short);
    s = windows(plain(500), 100, 500);
    s.paired = true;
    CHECK(form(s) == F::Short);
    CHECK(form(windows(syncmer(21, 11, 500), 100, 500)) == F::Short);
    CHECK(form(windows(minimizer(21, 10, 500), 100, 500)) == F::Short);
    CHECK(form(windows(plain(100000, 4), 50000, 100000)) == F::WinOnce);  // in front of the segment forms
    s = windows(plain(100000, 4), 50000, 100000);
    s.knobs.win_once = false;
    CHECK(form(s) == F::SegRoll2);
  }
  // ---- rows 2-4: whole genomes, a workgroup per segment of 65536 positions
  {
    CHECK(form(plain(65536, 4)) == F::Wg);  // one segment: a long read
    const K1Plan p = k1_plan(plain(65537, 4));
    CHECK(p.form == F::SegRoll2 && p.segs == 2 && p.grid == 8 && p.grid2 == 8 && p.list_fallback && !p.codes_direct && !p.adj_done);
    CHECK(p.counts.off == 0 && p.counts.len == 8 && p.counter.off == 8 && p.counter.len == 1 && p.list.off == 9 && p.list.len == 8 && p.marks.len == 0 &&
          p.side_words == 17);
    CHECK(k1_plan(plain(131072, 4)).segs == 2);
    CHECK(k1_plan(plain(131073, 4)).segs == 3);
    const K1Plan q = k1_plan(plain(131072, 1u << 20));  // n_reads * segs = 2^21
    CHECK(q.form == F::SegRoll2 && q.grid == (1u << 21) && q.grid2 == 512);
    CHECK(form(plain(131072, (1u << 20) + 1)) == F::Wg);
    CHECK(form(plain(131073, 1u << 20)) == F::Wg);
    K1Shape s = plain(100000, 4);
    s.k = 128;
    CHECK(form(s) == F::SegRoll2);
    CHECK(form(with_flags(s, 16 | 3)) == F::SegRoll);
    s.k = 129;
    CHECK(form(s) == F::SegHash);
    CHECK(form(with_flags(s, 16 | 3)) == F::SegHash);
    for (int fl : {0, 1, 2, 3, 4, 7, 32, 35}) CHECK(form(with_flags(plain(100000, 4), fl)) == F::SegRoll2);
    for (int fl : {16, 19, 16 | 4, 16 | 32}) CHECK(form(with_flags(plain(100000, 4), fl)) == F::SegRoll);
    for (int fl : {8, 11, 24, 27}) CHECK(form(with_flags(plain(100000, 4), fl)) == F::SegHash);
    const K1Plan r = k1_plan(with_flags(plain(100000, 4), 19));
    CHECK(r.segs == 2 && r.grid == 8 && r.counts.len == 8 && r.side_words == 8 && !r.list_fallback && r.list.len == 0);
    const K1Plan h = k1_plan(with_flags(plain(100000, 4), 11));
    CHECK(h.segs == 2 && h.grid == 8 && h.side_words == 8 && !h.list_fallback);
    s = plain(100000, 4);
    s.have_scratch = false;
    CHECK(form(s) == F::Wg && k1_plan(s).side_words == 0);
    s = plain(100000, 4);
    s.paired = true;
    CHECK(form(s) == F::Wg && k1_plan(s).side_words == 0);
    CHECK(form(minimizer(21, 10, 100000)) == F::WindowsWave);
    CHECK(k1_whole_genomes(0, false, 65537) && !k1_whole_genomes(0, false, 65536) && !k1_whole_genomes(0, true, 65537) && !k1_whole_genomes(1, false, 65537) &&
          !k1_whole_genomes(2, false, 65537));
  }
  // ---- codes read directly (row 2 only)
  {
    K1Plan p = k1_plan(packed(0));
    CHECK(p.form == F::SegRoll2 && p.codes_direct && !p.list_fallback && p.marks.len == 0 && p.list.len == 8 && p.side_words == 17);
    p = k1_plan(packed(1));
    CHECK(p.form == F::SegRoll2 && p.codes_direct && p.list_fallback && p.marks.off == 17 && p.marks.len == 8 && p.side_words == 25 && p.grid2 == 8);
    CHECK(k1_plan(packed(164)).codes_direct);
    CHECK(!k1_plan(packed(165)).codes_direct && form(packed(165)) == F::SegRoll2 && k1_plan(packed(165)).list_fallback && k1_plan(packed(165)).marks.len == 0);
    CHECK(k1_plan(packed(164, 2)).codes_direct && k1_plan(packed(165, 2)).codes_direct && k1_plan(packed(1000000, 2)).codes_direct);
    CHECK(!k1_plan(packed(0, 0)).codes_direct && !k1_plan(packed(164, 0)).codes_direct);
    K1Shape s = packed(1);
    s.packed.text_is_seqs = false;
    CHECK(!k1_plan(s).codes_direct);
    s = packed(1);
    s.packed.present = false;
    CHECK(!k1_plan(s).codes_direct);
    s = windows(packed(1), 50000, 100000);
    s.knobs.win_once = false;
    CHECK(form(s) == F::SegRoll2 && !k1_plan(s).codes_direct);  // the codes of a window batch are expanded
    CHECK(!k1_plan(windows(packed(1), 50000, 100000)).codes_direct);
    for (int fl : {8, 16, 19, 24}) CHECK(!k1_plan(with_flags(packed(1, 2), fl)).codes_direct);
    for (int fl : {3, 4, 7, 35}) CHECK(k1_plan(with_flags(packed(1, 2), fl)).codes_direct);
    s = packed(1, 2);
    s.k = 128;
    CHECK(k1_plan(s).codes_direct);
    s.k = 129;
    CHECK(!k1_plan(s).codes_direct);
    s = packed(1, 2);
    s.max_read_len = 65536;
    CHECK(!k1_plan(s).codes_direct && form(s) == F::Wg);
    s = packed(1, 2);
    s.paired = true;
    CHECK(!k1_plan(s).codes_direct);
    s = packed(1, 2);
    s.have_scratch = false;
    CHECK(!k1_plan(s).codes_direct);
  }
  // ---- rows 5, 6: window sketches of long reads on the wave forms
  {
    CHECK(form(syncmer(21, 11, 2048)) == F::Short && k1_plan(syncmer(21, 11, 2048)).grid == 250 && k1_plan(syncmer(21, 11, 2048)).side_words == 0);
    K1Plan p = k1_plan(syncmer(21, 11, 2049));
    CHECK(p.form == F::WindowsRoll && p.adj_done && p.list_fallback && p.wsz == 20 && p.waves == 2 && p.grid == 500 && p.grid2 == 1000);
    // words = (2049 + 1280 + 15) / 16 + 4 = 213; LDS = 1024 + 2 * (16 * 64 * 8 + 213 * 4) = 19112
    CHECK(p.words == 213 && p.lds_bytes == 19112 && p.counter.off == 0 && p.counter.len == 1 && p.list.off == 1 && p.list.len == 1000 && p.side_words == 1001);
    CHECK(k1_plan(syncmer(21, 11, 10000, 5000)).grid == 2500 && k1_plan(syncmer(21, 11, 10000, 5000)).grid2 == 1024);
    CHECK(k1_plan(syncmer(21, 11, 10000, 999)).grid == 500);
    // 2 (k - s) = 12, 16, 20, 24, 32 roll; 14, 60 stay on k1_windows_wave; 62 is past what a wave's window scan holds
    CHECK(form(syncmer(21, 15, 10000)) == F::WindowsRoll && k1_plan(syncmer(21, 15, 10000)).wsz == 12);
    CHECK(form(syncmer(31, 23, 10000)) == F::WindowsRoll && k1_plan(syncmer(31, 23, 10000)).wsz == 16);
    CHECK(form(syncmer(21, 11, 10000)) == F::WindowsRoll && k1_plan(syncmer(21, 11, 10000)).wsz == 20);
    CHECK(form(syncmer(31, 19, 10000)) == F::WindowsRoll && k1_plan(syncmer(31, 19, 10000)).wsz == 24);
    CHECK(form(syncmer(31, 15, 10000)) == F::WindowsRoll && k1_plan(syncmer(31, 15, 10000)).wsz == 32);
    CHECK(form(syncmer(21, 14, 10000)) == F::WindowsWave && k1_plan(syncmer(21, 14, 10000)).adj_done && k1_plan(syncmer(21, 14, 10000)).side_words == 0);
    CHECK(form(syncmer(41, 11, 10000)) == F::WindowsWave);  // 60
    CHECK(form(syncmer(42, 11, 10000)) == F::Wg && k1_plan(syncmer(42, 11, 10000)).adj_done);  // 62
    CHECK(form(syncmer(64, 54, 10000)) == F::WindowsRoll);
    CHECK(form(syncmer(65, 55, 10000)) == F::WindowsWave);
    CHECK(form(syncmer(66, 56, 10000)) == F::Wg);
    K1Shape s = syncmer(21, 11, 10000);
    s.paired = true;
    CHECK(form(s) == F::WindowsWave && k1_plan(s).adj_done && k1_plan(s).side_words == 0 && !k1_plan(s).list_fallback);
    s = syncmer(21, 11, 10000);
    s.have_scratch = false;
    CHECK(form(s) == F::Wg && !k1_plan(s).adj_done && k1_plan(s).side_words == 0);
    for (int fl : {0, 1, 2, 3, 8, 16, 19}) CHECK(form(with_flags(syncmer(21, 11, 10000), fl)) == F::WindowsRoll);
    for (int fl : {32, 35}) CHECK(form(with_flags(syncmer(21, 11, 10000), fl)) == F::WindowsWave);
    for (int fl : {4, 7, 4 | 32}) CHECK(form(with_flags(syncmer(21, 11, 10000), fl)) == F::Wg);
    // no read can be above max(-u, 512): the fused path is nobody's
    s = syncmer(21, 11, 3000);
    s.dedup_threshold = 3000;
    CHECK(form(s) == F::WindowsWave);
    s.max_read_len = 3001;
    CHECK(form(s) == F::WindowsRoll);
    s = syncmer(21, 11, 2049);
    s.dedup_threshold = 0;  // (the floor of 512 lies below the 2048 of this row)
    CHECK(form(s) == F::WindowsRoll);
    s.dedup_threshold = 0x7fffffff;
    s.max_read_len = 20000;
    CHECK(form(s) == F::WindowsWave);
    // LDS of k = 21, s = 11 (ring of 16 slots = 8192 bytes per wave): 1024 + waves * (8192 + 4 * words) <= 65536, words = (L + 1295) / 16 + 4
    //   2 waves: words <= 6016, L <= 94912;  1 wave: words <= 14080, L <= 223936;  4 waves: words <= 1984, L <= 30400
    p = k1_plan(syncmer(21, 11, 94912));
    CHECK(p.form == F::WindowsRoll && p.waves == 2 && p.words == 6016 && p.lds_bytes == 65536);
    p = k1_plan(syncmer(21, 11, 94913));
    CHECK(p.form == F::WindowsRoll && p.waves == 1 && p.grid == 1000);
    p = k1_plan(syncmer(21, 11, 223936));
    CHECK(p.form == F::WindowsRoll && p.waves == 1 && p.words == 14080 && p.lds_bytes == 65536);
    CHECK(form(syncmer(21, 11, 223937)) == F::WindowsWave && k1_plan(syncmer(21, 11, 223937)).adj_done);
    s = syncmer(21, 11, 30400);
    s.knobs.wr_waves = 4;
    CHECK(k1_plan(s).waves == 4 && k1_plan(s).grid == 250 && k1_plan(s).lds_bytes == 65536);
    s.max_read_len = 30401;
    CHECK(k1_plan(s).waves == 2);
    s.knobs.wr_waves = 1;
    CHECK(k1_plan(s).waves == 1 && k1_plan(s).grid == 1000);
    for (int wv : {0, 2, 3, 8, -1}) {
      s.knobs.wr_waves = wv;
      CHECK(k1_plan(s).waves == 2);
    }
    // a ring of 32 slots (window of 32 s-mers): 1024 + 2 * (16384 + 4 * words) <= 65536, words <= 3968, L <= 62144
    CHECK(k1_plan(syncmer(31, 15, 62144)).waves == 2 && k1_plan(syncmer(31, 15, 62145)).waves == 1);
    // minimizers: always k1_windows_wave<1>
    p = k1_plan(minimizer(21, 20, 10000));
    CHECK(p.form == F::WindowsWave && p.adj_done && p.grid == 1000 && p.side_words == 0);
    CHECK(form(minimizer(21, 60, 10000)) == F::WindowsWave && form(minimizer(21, 61, 10000)) == F::Wg);
    CHECK(form(with_flags(minimizer(21, 20, 10000), 7)) == F::Wg);
    CHECK(k1_plan(minimizer(21, 20, 10000)).grid == 1000 && k1_plan(syncmer(21, 14, 10000, 70000)).grid == 65536);
  }
  // ---- rows 7-9
  {
    CHECK(form(plain(2048)) == F::Short && k1_plan(plain(2048)).grid == 250 && k1_plan(plain(2048, 1001)).grid == 251);
    CHECK(k1_plan(plain(150, 200000)).grid == 32768 && k1_plan(plain(150, 131072)).grid == 32768 && k1_plan(plain(150, 131068)).grid == 32767);
    CHECK(form(plain(2049)) == F::Wg && k1_plan(plain(2049)).grid == 1000 && !k1_plan(plain(2049)).adj_done && k1_plan(plain(2049, 70000)).grid == 65536);
    K1Shape s = plain(3000);
    s.k = 255;
    CHECK(form(s) == F::Wg);
    s.k = 256;
    CHECK(form(s) == F::WgGlobal && k1_plan(s).grid == 1000 && !k1_plan(s).adj_done);
    CHECK(form(syncmer(262, 11, 3000)) == F::WgGlobal);  // 2 k - s - 1 = 512 fits the halo, k > 255 does not
    CHECK(form(syncmer(255, 11, 3000)) == F::Wg);        // 498
    CHECK(form(syncmer(255, 1, 3000)) == F::Wg);         // 508
    CHECK(form(syncmer(200, 100, 3000)) == F::Wg && form(syncmer(200, 0, 3000)) == F::WgGlobal && form(syncmer(200, 201, 3000)) == F::WgGlobal);
    CHECK(form(minimizer(21, 510, 3000)) == F::Wg && form(minimizer(21, 511, 3000)) == F::WgGlobal && form(minimizer(21, 0, 3000)) == F::WgGlobal);
    // row 8 drops adjacent repeats itself for window sketches with scratch and flag bit 1
    CHECK(k1_plan(with_flags(syncmer(21, 11, 3000), 7)).adj_done && k1_plan(with_flags(syncmer(21, 11, 3000), 6)).adj_done);
    CHECK(!k1_plan(with_flags(syncmer(21, 11, 3000), 5)).adj_done && !k1_plan(with_flags(syncmer(21, 11, 3000), 4)).adj_done);
    s = with_flags(syncmer(21, 11, 3000), 7);
    s.have_scratch = false;
    CHECK(form(s) == F::Wg && !k1_plan(s).adj_done);
    CHECK(!k1_plan(with_flags(plain(3000), 7)).adj_done);
    s = syncmer(21, 11, 150);
    s.paired = true;
    CHECK(form(s) == F::Short && k1_plan(s).side_words == 0);
  }
  // ---- the named bits are the documented numbers
  CHECK(K1F_TWO_LEVEL == 1 && K1F_FUSED_ADJ == 2 && K1F_NO_WAVE == 4 && K1F_SEG_HASH == 8 && K1F_SEG_ROLL == 16 && K1F_NO_ROLL == 32 && K1Knobs().flags == 3);
  // ---- invariants over a sweep of shapes
  unsigned long long shapes = 0;
  for (int mode = 0; mode < 3; mode++)
    for (int k : {1, 21, 31, 64, 65, 66, 128, 129, 255, 256})
      for (uint32_t ws : {0u, 1u, 11u, 15u, 19u, 60u, 61u, 300u})
        for (uint32_t len : {0u, 150u, 2048u, 2049u, 30401u, 65536u, 65537u, 94913u, 223937u, 4000000u})
          for (uint32_t n : {0u, 1u, 3u, 1000u, 70000u, 1u << 20, (1u << 20) + 1})
            for (int fl : {0, 3, 4, 7, 8, 16, 19, 32, 35, 63})
              for (int v = 0; v < 48; v++) {
                K1Shape s;
                s.mode = mode;
                s.k = k;
                s.w_or_s = ws;
                s.max_read_len = len;
                s.n_reads = n;
                s.knobs.flags = fl;
                s.paired = v & 1;
                s.have_scratch = v & 2;
                s.dedup_threshold = (v & 4) ? 0x7fffffff : 256;
                s.packed.present = v & 8;
                s.packed.text_is_seqs = true;
                s.packed.n_exc = (v & 16) ? 5 : 0;
                s.packed.n_bases = (uint64_t)n * len;
                s.knobs.codes_mode = v >= 32 ? 2 : 1;
                if (v >= 40) s = windows(s, (v & 1) ? len : len / 2, len, (uint64_t)n * len, n);
                s.knobs.wr_waves = 1 << (v % 3);
                invariants(s);
                shapes++;
              }
  printf("%llu checks over %llu swept shapes and the table's cases, %llu wrong\n", checked, shapes, bad);
  return bad ? 1 : 0;
}
