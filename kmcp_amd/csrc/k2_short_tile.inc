// k2_short_tile.inc — one tile of a short-read unit (k2_short.hpp), stated once and included where a kernel runs it: the SHORT branch of
// k2_cobs_body.inc and k2_cobs_persist (k2_cobs.hip).  Text, not a function: through a function boundary the compiler keeps the counters as
// one 32- / 40-word vector value instead of 32 / 40 scalars, which costs each of the four kernels 12-14 VGPRs and a dozen more moves
// (profiles/k2_short_once.txt); written into the kernel they compile as they always have.
// In scope: template <int NPL>, `a` (K2Args), `lane`, `exact` (K2F_EXACT_STOP), and the macros K2T_ROW (the wave's row of indices in LDS),
// K2T_BASE (the lane's 16 bytes of row 0 of the tile), K2T_N (k-mers of the read) and K2T_CM (k2_short_clamp of its threshold), the last
// two wave-uniform.  `bool lv` — in: the lane has columns in the row at all; out: its sector was alive at the end — and `uint32_t g_rows`,
// the lane's 16-byte row loads (profiling level 2), are the includer's variables.  Declares cp[4][NPL], the counts of the lane's 128
// columns, for the k2_emit_tile that follows.
// With the indices of the whole read at hand a sector (8 lanes, 128 bytes) need not march with the wave: it keeps its own row
// cursor.  `exact` (K2F_EXACT_STOP): before every group the sector asks how many rows its best column proves necessary — with `need`
// = the count a column must hold NOW to stay in the race, a column at need + j keeps the sector alive for j more rows whatever they
// hold, so rows done + 1 .. done + j + 1 will be asked for in any case — and loads exactly those, at most 4 at a time: no row is
// requested after the sector is lost, none past the end of the read.  Proven rows are kept as a credit and used up before the next
// test: counts are >= 0, so the first n - cmin + 1 rows of a read need no test at all; after that one test for 16 rows while some
// column is 15 ahead, then the test for 4, and the two finer ones (3 / 2 / 1 / lost) only when some sector of the wave fails that.
// The tests are what this loop can afford least (profiles/k2_exact_stop_ab.txt).  Without the bit: 4 rows (what is left of the
// read, if less) while the sector is alive, tested before every group.  Counts and hits are the same either way.
  const int sec0 = lane & ~7;  // first lane of this lane's sector
  uint32_t cp[4][NPL];
#pragma unroll
  for (int d = 0; d < 4; d++)
#pragma unroll
    for (int p = 0; p < NPL; p++) cp[d][p] = 0;
  // some column of this lane holds a count >= t_: the bit-sliced compare, LSB to MSB.  The plain form picks `&` or `|` per plane by a
  // wave-uniform bit; here t_ may differ from sector to sector, and the choice is a mask word into a majority (csa.hpp MAJ3)
  auto at_least = [&](int t_) __attribute__((always_inline)) -> bool {
    uint32_t w[NPL];
#pragma unroll
    for (int p = 0; p < NPL; p++) w[p] = (((uint32_t)t_ >> p) & 1u) - 1u;  // all ones where bit p of t_ is clear
    uint32_t any = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      uint32_t ge = 0xffffffffu;
#pragma unroll
      for (int p = 0; p < NPL; p++) ge = MAJ3(ge, cp[d][p], w[p]);
      any |= ge;
    }
    return t_ <= 0 || (((uint32_t)t_ >> NPL) == 0 && any != 0);
  };
  auto in_sector = [&](bool b) __attribute__((always_inline)) -> bool { return ((__ballot(b) >> sec0) & 0xffull) != 0; };
  int done = 0;         // rows this sector has added (the same in its 8 lanes)
  int sdone = 0;        // ... without K2F_EXACT_STOP: every live sector has added the same rows, a wave-uniform count
  int credit = 0;       // K2F_EXACT_STOP: rows from the cursor on that are already proven necessary (no test until they are used up)
  bool try_far = true;  // ... and whether the 16-row test is still worth its cost in this tile (wave-uniform)
  for (;;) {
    // L: the rows from its cursor on that the sector is certain to need (before the end of the read cuts it); a column must hold
    // `need` now to stay in the race
    int L, rem;
    if (exact) {
      rem = K2T_N - done;
      const int need = K2T_CM - rem;
      credit = max(credit, 1 - need);  // counts are >= 0: the first n - cmin + 1 rows of a read need no test at all
      const int want_rows = min(4, rem);
      bool ask = lv && credit < want_rows;
      if (__ballot(ask) != 0) {
        if (try_far) {  // a column 15 above `need` pays for four groups
          const bool far = in_sector(lv && at_least(need + 15));
          credit = ask && far ? 16 : credit;
          ask = ask && !far;
          try_far = __ballot(ask) == 0;
        }
        if (__ballot(ask) != 0) {
          const bool top = in_sector(lv && at_least(need + 3));
          credit = ask && top ? 4 : credit;
          ask = ask && !top;
          if (__ballot(ask) != 0) {  // some sector of the wave is within 3 rows of its end: which of 0..3, in two steps
            const bool r1 = in_sector(lv && at_least(need + 1));
            const bool r2 = in_sector(lv && at_least(r1 ? need + 2 : need));
            const int fine = r1 ? (r2 ? 3 : 2) : (r2 ? 1 : 0);
            credit = ask ? fine : credit;
            lv = lv && !(ask && fine == 0);  // no column can reach the threshold any more
          }
        }
      }
      L = lv ? min(credit, want_rows) : 0;
      credit -= L;
    } else {
      rem = K2T_N - sdone;
      L = in_sector(lv && at_least(K2T_CM - rem)) ? 4 : 0;
      sdone += min(4, rem);
      lv = lv && L > 0;  // L == 0: no column can reach the threshold any more (at the end of the read: none has)
      L = lv ? min(L, rem) : 0;
    }
    if (__ballot(L > 0) == 0) break;
    uint32_t ri[4];
    uint4 x[4];
#pragma unroll
    for (int i = 0; i < 4; i++) ri[i] = K2T_ROW[done + i];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      x[i] = make_uint4(0, 0, 0, 0);
      if (i < L) x[i] = load_row16_global(K2T_BASE + ((uint64_t)ri[i] << 4), a.nt_loads);
    }
    csa4<NPL>(cp[0], x[0].x, x[1].x, x[2].x, x[3].x);
    csa4<NPL>(cp[1], x[0].y, x[1].y, x[2].y, x[3].y);
    csa4<NPL>(cp[2], x[0].z, x[1].z, x[2].z, x[3].z);
    csa4<NPL>(cp[3], x[0].w, x[1].w, x[2].w, x[3].w);
    done += L;
    g_rows += (uint32_t)L;
  }
