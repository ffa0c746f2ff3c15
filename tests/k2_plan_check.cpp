// k2_plan_check.cpp — host instantiation of kmcp_amd/csrc/k2_plan.hpp (which COBS kernels a batch gets): every row of the table in
// DESIGN.md §4 with the shapes on either side of each boundary it names, the grid pieces around K2_MAX_BLOCKS (no test-sized batch
// reaches them on a GPU), the lane cutting of a row under each open knob, and over a sweep of shapes the invariants the launchers and
// query_device_after rely on.  The expected values are written out here by hand.  Built and run by tests/test_k2_plan_cpu.py.
#include <stdio.h>

#include <initializer_list>
#include <string>

#include "../kmcp_amd/csrc/k2_plan.hpp"

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

typedef K2Kind Kd;

static K2Shape shape(uint32_t n_reads, uint64_t max_n, std::initializer_list<K2Class> cls, int nh = 1) {
  K2Shape s;
  s.n_reads = n_reads;
  s.max_n = max_n;
  s.num_hashes = nh;
  s.n_cols = 1000;
  for (const K2Class& c : cls) s.classes[s.n_classes++] = c;
  return s;
}
// a database of two 1-KiB tiles per row
static K2Shape wide(uint32_t n_reads, uint64_t max_n) { return shape(n_reads, max_n, {{64, 2, 1}}); }
// ... of 1280-byte rows: a 1-KiB tile and a 16-lane remainder
static K2Shape two(uint32_t n_reads, uint64_t max_n, int nh = 1) { return shape(n_reads, max_n, {{64, 1, 0}, {16, 1, 0}}, nh); }
static K2Shape split_min(K2Shape s, int32_t v) {
  s.knobs.split_min = v;
  s.knobs.split_min_set = true;
  return s;
}
static K2Shape group_rows(K2Shape s, int v) {
  s.knobs.group_rows = v;
  s.knobs.group_rows_set = true;
  return s;
}
static K2Shape bytes(K2Shape s, uint64_t b) {
  s.matrix_bytes_local = b;
  return s;
}
// nobody asked the device
static K2Plan plain(const K2Shape& s) { return k2_plan(s, false, 0, 0); }
static int npl_of(uint64_t max_n) { return plain(wide(100000, max_n)).npl; }

// the tiles of a row as "lpr@byte+lpr@byte", the bytes counted from the end of the whole 1-KiB tiles (which must be there, in order)
static std::string parts(uint32_t stride, int nh, const K2OpenKnobs& kn) {
  const K2RowParts p = k2_row_parts(stride, nh, kn);
  std::string out;
  if (p.full != stride / 1024u) return "full tiles wrong";
  for (uint32_t i = 0; i < p.size(); i++) {
    const K2RowPart t = p[i];
    if (i < p.full) {
      if (t.lpr != 64 || t.byte0 != i * 1024u) return "full tiles wrong";
      continue;
    }
    if (t.byte0 % ((uint32_t)t.lpr * 16u)) return "tile off its own grid";
    out += (out.empty() ? "" : "+") + std::to_string(t.lpr) + "@" + std::to_string(t.byte0 - p.full * 1024u);
  }
  return out;
}

static void invariants(const K2Shape& s, bool asked, uint32_t listed, uint32_t max_long) {
  const K2Plan p = k2_plan(s, asked, listed, max_long);
  if (!p.npl) {
    CHECK(p.n_launches == 0 && p.max_short > K2_MAX_N_24);
    return;
  }
  CHECK(p.n_launches <= K2_MAX_LAUNCHES && (p.group_rows == 4 || p.group_rows == 8));
  CHECK(p.max_short <= (p.npl == 8 ? 254u : p.npl == 10 ? 1022u : p.npl == 16 ? 65534u : 16777214u));
  CHECK(p.n_long <= listed && (asked || p.n_long == 0) && (p.split_min != 0) == (p.n_long != 0));
  int n_first = 0, n_split = 0, n_pair = 0;
  for (int i = 0; i < p.n_launches; i++) {
    const K2Launch& l = p.launches[i];
    CHECK(l.cls >= 0 && l.cls < s.n_classes && l.lpr == s.classes[l.cls].lpr && l.multi == (s.num_hashes > 1));
    CHECK(l.gr == 8 || (l.gr == 4 && l.npl <= 10 && l.kind == Kd::Plain));
    CHECK(!l.k2_flags || (l.kind == Kd::Plain && l.lpr == 64 && l.gr == 4 && s.num_hashes == 1));
    CHECK(l.block_units == ((l.k2_flags & K2F_BLOCK_UNITS) != 0) && (!l.block_units || s.classes[l.cls].nbslots));
    // the persistent kernel: the short-read unit tile by tile on the 64-lane form, where the knob allows it, and nothing else
    CHECK(!l.persist || (l.kind == Kd::Plain && l.lpr == 64 && l.gr == 4 && l.npl <= 10 && !l.multi && l.k2_flags != 0 && !(l.k2_flags & K2F_BLOCK_UNITS) &&
                         !l.block_units && s.knobs.persist));
    if (l.kind == Kd::Split) {
      CHECK(l.npl == 16 && l.cls == n_split && l.units == 0 && p.n_long);
      n_split++;
      continue;
    }
    CHECK(n_split == 0 && l.npl == p.npl);  // the chunked launches come last
    if (l.kind == Kd::Pair) {
      CHECK(l.npl == 16 && l.lpr == 64 && l.lprb == s.classes[1].lpr && l.cls == 0 && l.cls_b == 1 && l.nba && l.nbb && (uint64_t)l.nba + l.nbb <= K2_MAX_BLOCKS);
      n_pair++;
    } else {
      CHECK(l.cls == n_first);
      // the pieces tile the grid (a grid of very many: its first three and its last)
      const uint64_t n = k2_n_pieces(l), G = 64 / (uint64_t)l.lpr, wgs = k2_workgroups(l.units, l.lpr);
      CHECK(n == (wgs + K2_MAX_BLOCKS - 1) / K2_MAX_BLOCKS && wgs * 4 * G >= l.units && (wgs == 0 || (wgs - 1) * 4 * G < l.units));
      for (uint64_t j = 0; j < n; j = (j == 2 && n > 4) ? n - 1 : j + 1) {
        const K2Piece pc = k2_piece(l, j);
        CHECK(pc.unit_base == j * K2_MAX_BLOCKS * 4 * G && pc.workgroups == (j + 1 < n ? K2_MAX_BLOCKS : wgs - j * K2_MAX_BLOCKS) && pc.workgroups >= 1);
      }
    }
    n_first++;
  }
  CHECK(n_pair <= 1 && n_first == (n_pair ? 1 : s.n_classes) && n_split == (p.n_long ? s.n_classes : 0));
  CHECK(!p.n_long || (p.split_chk >= 64 && p.split_chk <= 8192 && (uint64_t)p.split_chk * p.split_chunks >= max_long && p.group >= 1));
}

int main() {
  // ---- the named constants are the documented numbers
  CHECK(K2_MAX_BLOCKS == (1ull << 23) && K2_MAX_N_8 == 254 && K2_MAX_N_10 == 1022 && K2_MAX_N_16 == 65534 && K2_MAX_N_24 == 16777214);
  CHECK(K2_GR4_MIN_BYTES == 4294967296ull && K2_ASK_MAX_UNITS == 16384 && K2_ASK_MAX_N == 32768 && K2_PLAIN_MIN_LONG_UNITS == 1536 && K2_SPLIT_MIN_DEFAULT == 2048);
  CHECK(K2_CHUNK_MIN == 1024 && K2_CHUNK_MAX == 8192 && K2_CHUNKS_AIM == 64 && K2_CHUNK_ENV_MIN == 64 && K2_COUNTS_BYTES == 2147483648ull);
  CHECK(K2F_BLOCK_UNITS == 1 && K2F_EXACT_STOP == 2 && !K2_BLOCK_UNITS_DEFAULT && K2_EXACT_STOP_DEFAULT);
  CHECK((int)Kd::Plain == 0 && (int)Kd::Split == 1 && (int)Kd::Pair == 2);
  {
    const K2Knobs kn;
    CHECK(kn.split_min == 2048 && !kn.split_min_set && !kn.split_chunk_set && kn.nt_loads == 1 && kn.prune == 1 && !kn.group_rows_set && kn.prune_every == 1);
    CHECK(kn.slot_major == 1 && kn.tail_sectors == 2 && kn.tail_min == 64 && kn.pair && !kn.block_units && kn.exact_stop);
    CHECK(kn.persist && kn.persist_wgs == 0 && !K2Launch().persist);
  }
  // ---- planes: the largest NumKmers the plain kernel meets
  CHECK(npl_of(0) == 8 && npl_of(254) == 8 && npl_of(255) == 10 && npl_of(1022) == 10 && npl_of(1023) == 16 && npl_of(65534) == 16 && npl_of(65535) == 24);
  CHECK(npl_of(16777214) == 24 && npl_of(16777215) == 0 && plain(wide(100000, 16777215)).n_launches == 0);
  {
    // ... which, once the long queries are listed, is split_min (they leave) or the largest one listed (they stay: the 1536 rule)
    K2Plan p = k2_plan(wide(100, 70000), true, 3, 70000);
    CHECK(p.n_long == 3 && p.max_short == 2048 && p.npl == 16 && p.split_min == 2048);
    p = k2_plan(wide(100, 70000), true, 0, 0);  // the read-length bound was 70000, no query above 2048
    CHECK(p.n_long == 0 && p.max_short == 2048 && p.npl == 16 && p.split_min == 0);
    CHECK(k2_plan(split_min(wide(100, 70000), 254), true, 3, 70000).npl == 8 && k2_plan(split_min(wide(100, 70000), 255), true, 3, 70000).npl == 10);
    CHECK(k2_plan(split_min(wide(100, 70000), 1022), true, 3, 70000).npl == 10 && k2_plan(split_min(wide(100, 70000), 1023), true, 3, 70000).npl == 16);
    CHECK(k2_plan(split_min(wide(100, 70000), 16), true, 3, 70000).split_min == 16);
  }
  // ---- whether to ask the device which queries are long
  {
    CHECK(!k2_ask_long(wide(100, 2048)) && k2_ask_long(wide(100, 2049)));
    // 16384 / 16385 (query, slot) pairs: 4096 x 4, 3277 x 5
    const K2Shape at = shape(4096, 3000, {{64, 3, 0}, {16, 1, 0}}), above = shape(3277, 3000, {{64, 4, 0}, {8, 1, 0}});
    CHECK(k2_ask_long(at) && !k2_ask_long(above));
    CHECK(k2_ask_long(split_min(at, 2048)) && k2_ask_long(split_min(above, 2048)));  // the variable's presence: always
    K2Shape s = above;
    s.max_n = 32768;
    CHECK(!k2_ask_long(s) && k2_ask_long(split_min(s, 2048)) && k2_ask_long(split_min(s, 32767)) && !k2_ask_long(split_min(s, 32768)));
    s.max_n = 32769;
    CHECK(k2_ask_long(s) && k2_ask_long(split_min(s, 2048)));
    s = at;
    s.max_n = 32768;
    CHECK(k2_ask_long(s));
    CHECK(!k2_ask_long(split_min(wide(100, 1u << 30), 0)) && !k2_ask_long(split_min(wide(100, 1u << 30), -1)) && k2_ask_long(split_min(wide(100, 17), 16)) &&
          !k2_ask_long(split_min(wide(100, 16), 16)));
  }
  // ---- the 1536-unit rule: long queries that fill the chip by themselves keep the plain kernel
  {
    const K2Shape one = shape(5000, 40000, {{64, 1, 0}}), three = shape(5000, 40000, {{64, 2, 0}, {16, 1, 0}});
    K2Plan p = k2_plan(one, true, 1535, 40000);
    CHECK(p.n_long == 1535 && p.npl == 16 && p.max_short == 2048 && p.n_launches == 2 && p.launches[1].kind == Kd::Split);
    p = k2_plan(one, true, 1536, 40000);
    CHECK(p.n_long == 0 && p.npl == 16 && p.max_short == 40000 && p.split_min == 0 && p.n_launches == 1 && p.launches[0].kind == Kd::Plain && p.split_chk == 0);
    CHECK(k2_plan(three, true, 511, 40000).n_long == 511 && k2_plan(three, true, 512, 40000).n_long == 0);
    CHECK(k2_plan(one, true, 1536, 65534).n_long == 0 && k2_plan(one, true, 1536, 65534).npl == 16);
    CHECK(k2_plan(one, true, 1536, 65535).n_long == 1536 && k2_plan(one, true, 1536, 65535).npl == 16);  // 24 planes are what the chunked form avoids
    CHECK(k2_plan(split_min(one, 2048), true, 1536, 40000).n_long == 1536 && k2_plan(split_min(one, 2048), true, 5000, 40000).n_long == 5000);
    CHECK(k2_plan(one, false, 1535, 40000).n_long == 0 && k2_plan(one, false, 1535, 40000).max_short == 40000);  // not asked: nothing was listed
  }
  // ---- rows per group: 4 where the 8/10-plane kernels wait for HBM (an index of 4 GiB and more)
  {
    const uint64_t G4 = 4294967296ull;
    K2Plan p = plain(bytes(wide(1000, 150), G4 - 1));
    CHECK(p.group_rows == 8 && p.launches[0].gr == 8 && p.launches[0].k2_flags == 0);
    p = plain(bytes(wide(1000, 150), G4));
    CHECK(p.group_rows == 4 && p.launches[0].gr == 4 && p.npl == 8);
    CHECK(plain(bytes(wide(1000, 1022), G4)).launches[0].gr == 4 && plain(bytes(wide(1000, 1022), G4)).npl == 10);
    p = plain(bytes(wide(100000, 1023), G4));
    CHECK(p.group_rows == 8 && p.launches[0].gr == 8 && p.npl == 16);
    K2Shape s = bytes(wide(1000, 150), G4);
    s.knobs.prune = 0;
    CHECK(plain(s).group_rows == 8);
    // KMCPG_GROUP_ROWS overrides; at 16 / 24 planes the setting stays 4 and the kernel 8-row
    CHECK(plain(group_rows(wide(1000, 150), 4)).launches[0].gr == 4 && plain(group_rows(bytes(wide(1000, 150), G4), 8)).launches[0].gr == 8);
    CHECK(plain(group_rows(wide(1000, 150), 5)).group_rows == 8 && plain(group_rows(bytes(wide(1000, 150), G4), 0)).group_rows == 8);
    s.knobs.prune = 0;
    CHECK(plain(group_rows(s, 4)).group_rows == 4);
    for (uint64_t n : {1023u, 65534u, 65535u}) {
      p = plain(group_rows(wide(100000, n), 4));
      CHECK(p.group_rows == 4 && p.n_launches == 1 && p.launches[0].gr == 8 && p.launches[0].npl == (n == 65535 ? 24 : 16) && p.launches[0].k2_flags == 0);
    }
    for (int v : {2, 4, 8}) {
      s = wide(1000, 150);
      s.knobs.prune_every = v;
      CHECK(plain(s).prune_every == v);
    }
    for (int v : {-1, 0, 1, 3, 16}) {
      s = wide(1000, 150);
      s.knobs.prune_every = v;
      CHECK(plain(s).prune_every == 1);
    }
  }
  // ---- the pair: 16 planes, the 8-row setting, a 64-lane class and one narrower class, two non-empty halves in one grid
  {
    K2Plan p = plain(two(20001, 3000, 3));  // 20001 units each: 5001 workgroups of 4 units, 1251 of 16
    CHECK(!k2_ask_long(two(20001, 3000, 3)));
    CHECK(p.npl == 16 && p.n_launches == 1);
    const K2Launch& l = p.launches[0];
    CHECK(l.kind == Kd::Pair && l.lpr == 64 && l.lprb == 16 && l.npl == 16 && l.multi && l.gr == 8 && l.cls == 0 && l.cls_b == 1 && l.nba == 5001 && l.nbb == 1251 &&
          l.k2_flags == 0 && !l.block_units);
    CHECK(!plain(two(20001, 3000)).launches[0].multi && plain(two(20001, 3000)).launches[0].kind == Kd::Pair);
    for (int lb : {4, 8, 32}) CHECK(plain(shape(20001, 3000, {{64, 1, 0}, {lb, 1, 0}})).launches[0].lprb == lb);
    // declined: the plain launches class by class
    auto declined = [](const K2Plan& q, int npl) {
      return q.n_launches == 2 && q.launches[0].kind == Kd::Plain && q.launches[1].kind == Kd::Plain && q.launches[0].lpr == 64 && q.launches[1].lpr == 16 &&
             q.launches[0].npl == npl && q.launches[1].npl == npl && q.launches[0].cls == 0 && q.launches[1].cls == 1 && q.launches[0].units == 20001 &&
             q.launches[1].units == 20001;
    };
    CHECK(declined(plain(two(20001, 65535)), 24));          // 24 planes
    CHECK(declined(plain(two(20001, 1022)), 10));           // short reads
    CHECK(declined(plain(group_rows(two(20001, 3000), 4)), 16) && plain(group_rows(two(20001, 3000), 4)).launches[0].gr == 8);  // under the 4-row setting
    CHECK(plain(group_rows(two(20001, 3000), 8)).launches[0].kind == Kd::Pair);
    K2Shape s = two(20001, 3000);
    s.knobs.pair = false;
    CHECK(declined(plain(s), 16));
    CHECK(plain(shape(20001, 3000, {{64, 1, 0}, {16, 1, 0}, {4, 1, 0}})).n_launches == 3);    // three classes
    CHECK(plain(shape(20001, 3000, {{32, 1, 0}, {16, 1, 0}})).launches[0].kind == Kd::Plain);  // no 64-lane class in front
    CHECK(plain(shape(20001, 3000, {{16, 1, 0}, {64, 1, 0}})).launches[0].kind == Kd::Plain);
    CHECK(plain(two(0, 3000)).n_launches == 2 && plain(two(0, 3000)).launches[0].kind == Kd::Plain && k2_n_pieces(plain(two(0, 3000)).launches[0]) == 0);  // empty halves
    CHECK(plain(shape(20001, 3000, {{64, 1, 0}, {16, 0, 0}})).launches[0].kind == Kd::Plain);
    // nba + nbb against 2^23: 2^24 reads x (one 64-lane slot + four 16-lane slots) = 2^22 + 2^22 workgroups
    const K2Plan fits = plain(shape(1u << 24, 3000, {{64, 1, 0}, {16, 4, 0}})), over = plain(shape((1u << 24) + 1, 3000, {{64, 1, 0}, {16, 4, 0}}));
    CHECK(fits.n_launches == 1 && fits.launches[0].kind == Kd::Pair && fits.launches[0].nba == (1u << 22) && fits.launches[0].nbb == (1u << 22));
    CHECK(over.n_launches == 2 && over.launches[0].kind == Kd::Plain && over.launches[1].kind == Kd::Plain && over.launches[1].units == 4 * ((1ull << 24) + 1));
    // with the long queries on the chunked form: the pair for the rest, then the chunked launches
    p = k2_plan(split_min(two(20001, 70000), 2048), true, 7, 70000);
    CHECK(p.n_launches == 3 && p.launches[0].kind == Kd::Pair && p.launches[1].kind == Kd::Split && p.launches[2].kind == Kd::Split && p.launches[2].lpr == 16);
  }
  // ---- block units and the exact stop: the flags of the 64-lane class of a short-read batch on 4-row kernels
  {
    const uint64_t G4 = 4294967296ull;
    K2Shape s = bytes(shape(1000, 150, {{64, 10, 3}, {8, 5, 0}}), G4);
    K2Plan p = plain(s);
    CHECK(p.n_launches == 2 && p.launches[0].k2_flags == K2F_EXACT_STOP && !p.launches[0].block_units && p.launches[0].units == 10000 && p.launches[1].k2_flags == 0 &&
          p.launches[1].units == 5000 && p.launches[1].gr == 4);
    s.knobs.block_units = true;
    p = plain(s);
    CHECK(p.launches[0].k2_flags == (K2F_BLOCK_UNITS | K2F_EXACT_STOP) && p.launches[0].block_units && p.launches[0].units == 3000 && p.launches[1].k2_flags == 0 &&
          !p.launches[1].block_units);
    s.knobs.exact_stop = false;
    CHECK(plain(s).launches[0].k2_flags == K2F_BLOCK_UNITS && plain(s).launches[0].block_units);
    s.classes[0].nbslots = 0;  // a class without the list: tile by tile, the bit cleared
    CHECK(plain(s).launches[0].k2_flags == 0 && !plain(s).launches[0].block_units && plain(s).launches[0].units == 10000);
    s.knobs.exact_stop = true;
    CHECK(plain(s).launches[0].k2_flags == K2F_EXACT_STOP && plain(s).launches[0].units == 10000);
    s.classes[0].nbslots = 3;
    // ... only there: several hash functions, no pruning, a sparser test, 8 rows, more planes
    K2Shape t = s;
    t.num_hashes = 2;
    CHECK(plain(t).launches[0].k2_flags == 0 && plain(t).launches[0].gr == 4);
    t = s;
    t.knobs.prune_every = 2;
    CHECK(plain(t).launches[0].k2_flags == 0);
    t = s;
    t.knobs.prune = 0;
    CHECK(plain(t).launches[0].k2_flags == 0 && plain(group_rows(t, 4)).launches[0].k2_flags == 0 && plain(group_rows(t, 4)).launches[0].gr == 4);
    CHECK(plain(group_rows(s, 8)).launches[0].k2_flags == 0 && plain(bytes(s, G4 - 1)).launches[0].k2_flags == 0);
    CHECK(plain(group_rows(bytes(s, 0), 4)).launches[0].k2_flags == 3);
    t = s;
    t.max_n = 1022;
    CHECK(plain(t).launches[0].k2_flags == 3);
    t.max_n = 1023;
    t.n_reads = 100000;
    CHECK(plain(t).launches[0].k2_flags == 0 && plain(group_rows(t, 4)).launches[0].k2_flags == 0);
  }
  // ---- the persistent kernel: the launch of the 64-lane class that takes the short-read unit tile by tile, unless KMCPG_K2_PERSIST=0
  {
    const uint64_t G4 = 4294967296ull;
    const K2Shape s = bytes(shape(1000, 150, {{64, 10, 3}, {8, 5, 0}}), G4);  // the default short-read shape of the block above
    K2Plan p = plain(s);
    CHECK(p.n_launches == 2 && p.launches[0].persist && p.launches[0].k2_flags == K2F_EXACT_STOP && p.launches[0].units == 10000 && !p.launches[1].persist);
    K2Shape t = s;
    t.max_n = 1022;  // 10 planes: the other instantiation
    CHECK(plain(t).launches[0].persist && plain(t).launches[0].npl == 10);
    t = s;
    t.knobs.persist_wgs = 3;  // the grid is the launcher's business
    CHECK(plain(t).launches[0].persist);
    t = s;
    t.knobs.persist = false;
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].k2_flags == K2F_EXACT_STOP && plain(t).launches[0].gr == 4);
    t = s;
    t.knobs.block_units = true;  // block units with a list: several tiles per unit, the launched form
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].block_units && plain(t).launches[0].k2_flags == 3);
    t.classes[0].nbslots = 0;  // a class without the list: the bit is cleared, tile by tile again
    CHECK(plain(t).launches[0].persist && plain(t).launches[0].k2_flags == K2F_EXACT_STOP && !plain(t).launches[0].block_units);
    t.knobs.exact_stop = false;  // ... and with no bit left the plain loop of the body
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].k2_flags == 0);
    t = s;
    t.knobs.exact_stop = false;
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].k2_flags == 0);
    t = s;
    t.num_hashes = 2;
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].multi && plain(t).launches[0].gr == 4);
    t = s;
    t.knobs.prune = 0;
    CHECK(!plain(t).launches[0].persist && !plain(group_rows(t, 4)).launches[0].persist && plain(group_rows(t, 4)).launches[0].gr == 4);
    t = s;
    t.knobs.prune_every = 2;
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].gr == 4);
    CHECK(!plain(group_rows(s, 8)).launches[0].persist && plain(group_rows(s, 8)).launches[0].gr == 8);
    CHECK(!plain(bytes(s, G4 - 1)).launches[0].persist && plain(group_rows(bytes(s, 0), 4)).launches[0].persist);
    t = s;
    t.max_n = 1023;  // 16 planes
    t.n_reads = 100000;
    CHECK(!plain(t).launches[0].persist && plain(t).launches[0].npl == 16 && !plain(group_rows(t, 4)).launches[0].persist);
    // lane classes below 64: never, whatever their order
    p = plain(bytes(shape(1000, 150, {{32, 4, 0}, {16, 2, 0}, {8, 1, 0}, {4, 1, 0}}), G4));
    CHECK(p.n_launches == 4 && !p.launches[0].persist && !p.launches[1].persist && !p.launches[2].persist && !p.launches[3].persist && p.launches[0].gr == 4);
    p = plain(bytes(shape(1000, 150, {{16, 2, 0}, {64, 10, 0}}), G4));
    CHECK(!p.launches[0].persist && p.launches[1].persist);
    // a pair plan, and the chunked launches behind a persistent one
    p = plain(group_rows(two(20001, 3000), 8));
    CHECK(p.n_launches == 1 && p.launches[0].kind == Kd::Pair && !p.launches[0].persist);
    p = k2_plan(split_min(bytes(wide(100, 70000), G4), 254), true, 3, 70000);
    CHECK(p.npl == 8 && p.n_launches == 2 && p.launches[0].persist && p.launches[1].kind == Kd::Split && !p.launches[1].persist);
  }
  // ---- units, workgroups and the grid pieces under K2_MAX_BLOCKS
  {
    CHECK(k2_units(7, 5, 16, 1) == 35 && k2_units(7, 5, 16, 0) == 35 && k2_units(7, 5, 16, 2) == 56 && k2_units(7, 8, 16, 2) == 56 && k2_units(7, 9, 16, 2) == 84);
    CHECK(k2_units(7, 5, 64, 2) == 35 && k2_units(7, 5, 32, 2) == 42 && k2_units(7, 5, 4, 2) == 112 && k2_units(1u << 31, 1u << 31, 64, 1) == (1ull << 62));
    CHECK(k2_workgroups(0, 64) == 0 && k2_workgroups(1, 64) == 1 && k2_workgroups(4, 64) == 1 && k2_workgroups(5, 64) == 2 && k2_workgroups(64, 4) == 1 &&
          k2_workgroups(65, 4) == 2 && k2_workgroups(16, 16) == 1 && k2_workgroups(17, 16) == 2);
    K2Shape s = shape(7, 150, {{16, 5, 0}});
    s.knobs.slot_major = 2;
    CHECK(plain(s).launches[0].units == 56 && plain(shape(7, 150, {{16, 5, 0}})).launches[0].units == 35);
    s = two(20001, 3000);  // the pair's second half rounds its slots up to a wave's 4 units
    s.knobs.slot_major = 2;
    CHECK(plain(s).launches[0].kind == Kd::Pair && plain(s).launches[0].nba == 5001 && plain(s).launches[0].nbb == 5001);
    for (int lpr : {64, 4}) {
      const uint64_t G = 64 / (uint64_t)lpr, full = K2_MAX_BLOCKS * 4 * G;  // units of one full piece: 2^25, 2^29
      K2Launch l;
      l.lpr = lpr;
      l.units = full - 1;
      CHECK(k2_n_pieces(l) == 1 && k2_piece(l, 0).unit_base == 0 && k2_piece(l, 0).workgroups == (1u << 23));
      l.units = full - 4 * G;
      CHECK(k2_n_pieces(l) == 1 && k2_piece(l, 0).workgroups == (1u << 23) - 1);
      l.units = full;
      CHECK(k2_n_pieces(l) == 1 && k2_piece(l, 0).unit_base == 0 && k2_piece(l, 0).workgroups == (1u << 23));
      l.units = full + 1;
      CHECK(k2_n_pieces(l) == 2 && k2_piece(l, 0).unit_base == 0 && k2_piece(l, 0).workgroups == (1u << 23) && k2_piece(l, 1).unit_base == full &&
            k2_piece(l, 1).workgroups == 1);
      l.units = 2 * full + 4 * G + 1;
      CHECK(k2_n_pieces(l) == 3 && k2_piece(l, 1).unit_base == full && k2_piece(l, 1).workgroups == (1u << 23) && k2_piece(l, 2).unit_base == 2 * full &&
            k2_piece(l, 2).workgroups == 2);
      CHECK(full == (lpr == 64 ? 1ull << 25 : 1ull << 29));
    }
    // ... through the plan: 2^25 + 1 reads on one 64-lane slot, 2^25 reads on 16 + 1 4-lane slots; the chunked form's units per group
    K2Plan p = plain(shape((1u << 25) + 1, 150, {{64, 1, 0}}));
    CHECK(k2_n_pieces(p.launches[0]) == 2 && k2_piece(p.launches[0], 1).unit_base == (1ull << 25) && k2_piece(p.launches[0], 1).workgroups == 1);
    p = plain(shape(1u << 25, 150, {{4, 17, 0}}));
    CHECK(p.launches[0].units == 17 * (1ull << 25) && k2_n_pieces(p.launches[0]) == 2 && k2_piece(p.launches[0], 1).unit_base == (1ull << 29) &&
          k2_piece(p.launches[0], 1).workgroups == (1u << 19));
    const K2Shape g = shape(100, 1u << 24, {{64, 3, 0}, {4, 2, 0}});
    p = k2_plan(g, true, 40, 1u << 24);  // 2048 chunks of 8192 k-mers; the other queries on the pair
    CHECK(p.n_long == 40 && p.split_chk == 8192 && p.split_chunks == 2048 && p.n_launches == 3 && p.launches[0].kind == Kd::Pair && p.launches[1].kind == Kd::Split &&
          p.launches[2].kind == Kd::Split && p.launches[2].lpr == 4);
    const K2Launch a40 = k2_split_launch(p, g, p.launches[1], 40), b7 = k2_split_launch(p, g, p.launches[2], 7);
    CHECK(a40.units == 40ull * 3 * 2048 && b7.units == 7ull * 2 * 2048 && b7.kind == Kd::Split && b7.lpr == 4 && p.launches[2].units == 0);
    CHECK(k2_n_pieces(a40) == 1 && k2_piece(a40, 0).workgroups == 61440 && k2_piece(b7, 0).workgroups == 448);  // 28672 units, 16 to a wave
  }
  // ---- the chunked form: chunk size, chunks, long queries per count array
  {
    auto chunks = [](uint32_t max_long, int env = -1, uint64_t n_cols = 1000) {
      K2Shape s = wide(100, max_long);
      s.n_cols = n_cols;
      if (env >= 0) s.knobs.split_chunk = env, s.knobs.split_chunk_set = true;
      return k2_plan(s, true, 5, max_long);
    };
    CHECK(chunks(2049).split_chk == 1024 && chunks(2049).split_chunks == 3 && chunks(65536).split_chk == 1024 && chunks(65536).split_chunks == 64);
    CHECK(chunks(65537).split_chk == 2048 && chunks(65537).split_chunks == 33 && chunks(131073).split_chk == 4096 && chunks(262144).split_chk == 4096);
    CHECK(chunks(262145).split_chk == 8192 && chunks(1u << 30).split_chk == 8192 && chunks(1u << 30).split_chunks == (1u << 17) && chunks(1000001).split_chunks == 123);
    CHECK(chunks(70000, 0).split_chk == 64 && chunks(70000, 63).split_chk == 64 && chunks(70000, 64).split_chk == 64 && chunks(70000, 65).split_chk == 65 &&
          chunks(70000, 65).split_chunks == 1077);
    CHECK(chunks(70000, 8192).split_chk == 8192 && chunks(70000, 8193).split_chk == 8192 && chunks(70000, 1 << 30).split_chk == 8192 && chunks(70000, 8192).split_chunks == 9);
    CHECK(chunks(70000).group == 536870 && chunks(70000, -1, 1u << 28).group == 2 && chunks(70000, -1, (1u << 28) + 1).group == 1 && chunks(70000, -1, 1u << 29).group == 1 &&
          chunks(70000, -1, (1u << 29) + 1).group == 1 && chunks(70000, -1, 1).group == (1u << 29));
    const K2Plan p = chunks(70000);
    CHECK(p.n_launches == 2 && p.launches[1].kind == Kd::Split && p.launches[1].npl == 16 && p.launches[1].gr == 8 && p.launches[1].lpr == 64 && p.launches[1].cls == 0 &&
          !p.launches[1].block_units && p.launches[1].k2_flags == 0 && !p.launches[1].multi);
    CHECK(k2_plan(shape(100, 70000, {{64, 1, 0}}, 3), true, 5, 70000).launches[1].multi);
    CHECK(plain(wide(100000, 3000)).split_chk == 0 && plain(wide(100000, 3000)).group == 0);
  }
  // ---- the lane forms of a row (remainders other than 16 and 32 are multiples of 64 in a database: the others are pinned as the rule stands)
  {
    K2OpenKnobs def, no8, no32, st0, st1, st2;
    no8.lpr8 = false;
    no32.lpr32 = false;
    st0.split_tiles = 0;
    st1.split_tiles = 1;
    st2.split_tiles = 2;
    CHECK(def.lpr8 && def.lpr32 && def.split_tiles == -1);
    struct Row {
      uint32_t rem;
      const char *def1, *def3, *no8, *no32, *all;  // default rule with 1 / 3 hash functions; KMCPG_LPR8=0; KMCPG_LPR32=0; KMCPG_SPLIT_TILES=2
    };
    const Row rows[] = {
        {0, "", "", "", "", ""},
        {16, "4@0", "4@0", "4@0", "4@0", "4@0"},
        {64, "4@0", "4@0", "4@0", "4@0", "4@0"},
        {65, "8@0", "8@0", "16@0", "8@0", "8@0"},
        {128, "8@0", "8@0", "16@0", "8@0", "8@0"},
        {129, "16@0", "16@0", "16@0", "16@0", "16@0"},
        {256, "16@0", "16@0", "16@0", "16@0", "16@0"},
        {257, "32@0", "32@0", "64@0", "64@0", "16@0"},
        {512, "32@0", "32@0", "64@0", "64@0", "32@0"},
        {513, "64@0", "64@0", "64@0", "64@0", "32@0"},
        {576, "64@0", "64@0", "64@0", "64@0", "32@0+4@512"},
        {640, "32@0+8@512", "64@0", "32@0+8@512", "32@0+8@512", "32@0+8@512"},
        {768, "64@0", "64@0", "64@0", "64@0", "32@0+16@512"},
        {832, "64@0", "64@0", "64@0", "64@0", "32@0+16@512+4@768"},
        {896, "64@0", "64@0", "64@0", "64@0", "32@0+16@512+8@768"},
        {960, "64@0", "64@0", "64@0", "64@0", "64@0"},
    };
    for (const Row& r : rows)
      for (uint32_t full : {0u, 1u, 3u}) {
        const uint32_t stride = full * 1024u + r.rem;
        CHECK(parts(stride, 1, def) == r.def1 && parts(stride, 3, def) == r.def3);
        CHECK(parts(stride, 1, no8) == r.no8 && parts(stride, 3, no8) == (r.rem == 640 ? "64@0" : r.no8));
        CHECK(parts(stride, 1, no32) == r.no32 && parts(stride, 3, no32) == (r.rem == 640 ? "64@0" : r.no32));
        CHECK(parts(stride, 1, st2) == r.all && parts(stride, 3, st2) == r.all);
        CHECK(parts(stride, 1, st1) == r.def3 && parts(stride, 3, st1) == r.all);  // 1: databases with several hash functions only
        CHECK(parts(stride, 1, st0) == r.def3 && parts(stride, 3, st0) == r.def3);  // 0: nobody, the 640-byte rule included
        CHECK(k2_row_parts(stride, 1, def).full == full && k2_row_parts(stride, 1, def).size() == full + (r.rem ? (r.rem == 640 ? 2u : 1u) : 0u));
      }
    CHECK(lpr_for_stride(64, def) == 4 && lpr_for_stride(65, def) == 8 && lpr_for_stride(1023, def) == 64 && lpr_for_stride(256, no8) == 16 && lpr_for_stride(257, no8) == 64);
  }
  // ---- invariants over a sweep of shapes
  unsigned long long shapes = 0;
  const K2Class c64{64, 3, 2}, c32{32, 1, 0}, c16{16, 2, 0}, c8{8, 1, 0}, c4{4, 5, 0}, big64{64, 1u << 20, 0}, big4{4, 1u << 12, 0};
  const std::initializer_list<K2Class> sets[] = {{c64}, {c4}, {c64, c16}, {c64, c32, c8}, {c16, c64}, {big64, c4}, {big64, big4}, {c64, c32, c16, c8, c4}, {}};
  for (const auto& set : sets)
    for (uint32_t n_reads : {0u, 1u, 37u, 5000u, 1u << 20, (1u << 25) + 3, 0xffffffffu})
      for (uint64_t max_n : {0ull, 254ull, 255ull, 1022ull, 1023ull, 2048ull, 2049ull, 32768ull, 32769ull, 65534ull, 65535ull, 16777214ull, 16777215ull})
        for (int v = 0; v < 96; v++) {
          K2Shape s = shape(n_reads, max_n, set, (v & 1) ? 3 : 1);
          s.matrix_bytes_local = (v & 2) ? 5ull << 30 : 1ull << 30;
          if (v & 4) s = split_min(s, (v & 8) ? 16 : 0);
          if (v & 16) s = group_rows(s, (v & 8) ? 4 : 8);
          s.knobs.slot_major = v >> 5;
          s.knobs.block_units = (v & 8) != 0;
          s.knobs.pair = (v & 64) == 0;
          s.knobs.persist = (v & 3) != 3;
          const bool ask = k2_ask_long(s);
          for (uint32_t listed : {0u, 1u, 511u, 1536u}) {
            if (listed > n_reads) continue;
            const uint32_t max_long = listed ? (uint32_t)max_n : 0;
            if (listed && max_n <= (uint64_t)s.knobs.split_min) continue;
            invariants(s, ask, listed, max_long);
            shapes++;
          }
        }
  printf("%llu checks over %llu swept shapes and the table's cases, %llu wrong\n", checked, shapes, bad);
  return bad ? 1 : 0;
}
