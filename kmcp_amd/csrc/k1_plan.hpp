// k1_plan.hpp — which k-mer kernels (K1) a batch gets, decided once: the shape of the batch and the knobs in, the kernel form, its grids
// and the layout of its side buffer out.  query.cpp run_kmers builds the shape and fills K1Args from the plan; k1_kmers.hip launch_k1 is a
// switch over the form.  Host-only arithmetic in plain C++17 (tests/k1_plan_check.cpp compiles it with g++); the constants and the small
// predicates are shared with the kernels.  The table of forms: DESIGN.md §4.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define K1_HD __host__ __device__ __forceinline__
#else
#define K1_HD inline
#endif

namespace kmcpg {

constexpr int K1SEG = 65536;              // whole genomes: k-mer positions of a read one workgroup hashes (a segment)
constexpr int K1_SEG_MAX_K = 128;         // the rolling segment kernels: what their staging halo holds
constexpr uint64_t K1_SEG_MAX_WGS = 1ull << 21;  // one workgroup of 1024 threads per segment, < 2^32 threads per launch
constexpr int K1_LONG_READ = 2048;        // a batch with a longer query: a workgroup (or a wave) per read instead of four reads per workgroup
constexpr int K1_SCAN_MAX_K = 65;         // a k-mer may reach into the next tile only
constexpr int K1_WAVE_SORT_CAP = 512;     // = DEDUP_WAVE_CAP (kernels.hpp): queries the wave sort takes keep their raw emissions
constexpr int K1H = 512;                  // halo of the workgroup-per-read window kernels
constexpr int WR_PAD_BASES = 1024 + 256;  // k1_windows_roll: what the last lanes' (predicated-off) steps and the refills may still read: zeros
constexpr size_t K1_LDS_MAX = 65536;      // LDS a workgroup may ask for

// KMCPG_K1_FLAGS, default 3
enum : int {
  K1F_TWO_LEVEL = 1,  // bit 0: two-level window arg-min
  K1F_FUSED_ADJ = 2,  // bit 1: k1_kmers_wg<1|2> drops adjacent repeats itself
  K1F_NO_WAVE = 4,    // bit 2: window sketches of long reads on the workgroup form, not k1_windows_wave
  K1F_SEG_HASH = 8,   // bit 3: whole genomes on the prefix-XOR kernel k1_seg_hash
  K1F_SEG_ROLL = 16,  // bit 4: whole genomes on the byte kernel k1_seg_roll alone
  K1F_NO_ROLL = 32,   // bit 5: k1_windows_wave alone, without k1_windows_roll in front
};

K1_HD bool wg_lds_usable(int mode, int k, int ws) {
  if (k > 255) return false;
  if (mode == 2) return 2 * k - ws - 1 <= K1H && ws >= 1 && ws <= k;
  if (mode == 1) return ws >= 1 && ws + 1 < K1H;
  return true;
}
K1_HD bool wave_windows_usable(int mode, int k, int ws) {
  if (k > K1_SCAN_MAX_K || k < 1) return false;
  if (mode == 2) return ws >= 1 && ws <= k && 2 * (k - ws) <= 60;
  if (mode == 1) return ws >= 1 && ws <= 60;
  return false;
}
K1_HD int wr_words_for(int max_read_len) { return (max_read_len + WR_PAD_BASES + 15) / 16 + 4; }
K1_HD int wr_ring(int wsz) { return wsz <= 30 ? 16 : 32; }  // >= k - s + 1 = wsz / 2 + 1 slots
K1_HD size_t wr_lds_bytes(int wsz, int words, int waves) { return 1024 + (size_t)waves * ((size_t)wr_ring(wsz) * 64 * 8 + (size_t)words * 4); }

struct K1Knobs {
  int flags = K1F_TWO_LEVEL | K1F_FUSED_ADJ;  // KMCPG_K1_FLAGS
  int codes_mode = 1;    // KMCPG_K1_CODES: 0 expand every packed batch, 1 codes read directly unless runs are dense, 2 whatever the runs
  bool win_once = true;  // KMCPG_WIN_ONCE
  int wr_waves = 2;      // KMCPG_WR_WAVES
  bool debug = false;    // KMCPG_K1_DEBUG
};

// everything the choice depends on
struct K1Shape {
  int mode = 0;  // 0 plain (+scaled), 1 minimizer, 2 syncmer
  int k = 0;
  uint32_t w_or_s = 0;
  bool paired = false;
  uint32_t n_reads = 0, max_read_len = 0;
  bool have_scratch = false;
  int32_t dedup_threshold = 0;
  struct {
    bool present = false;
    uint64_t step = 0, window = 0, sb = 0, n_chunks = 0;
  } win;  // sliding windows (WindowSrc)
  struct {
    bool present = false;
    uint32_t n_exc = 0;
    uint64_t n_bases = 0;
    bool text_is_seqs = false;  // the expansion would land where the kernels read text
  } packed;  // 2-bit source (PackedSrc)
  K1Knobs knobs;
};

// one value per row of the table in DESIGN.md §4
enum class K1Form { None, WinOnce, SegRoll2, SegRoll, SegHash, WindowsRoll, WindowsWave, WgGlobal, Wg, Short };

struct K1Region {  // 32-bit words of the side buffer; len 0: the plan has no such region
  size_t off = 0, len = 0;
};

struct K1Plan {
  K1Form form = K1Form::None;
  bool codes_direct = false;   // SegRoll2 reads the batch's 2-bit codes as they are: nothing is expanded beforehand
  bool list_fallback = false;  // a second kernel walks the list the first one leaves (SegRoll2: k1_seg_roll; WindowsRoll: k1_windows_wave<2>)
  bool adj_done = false;       // the kernels drop adjacent repeats themselves (scratch[] + nk_adj[]): K1d skips that pass
  bool debug = false;          // the knob, for the launcher: report what WindowsRoll left on its list
  uint32_t max_read_len = 0;   // ... and the shape's, for that line
  uint32_t segs = 0;           // Seg*: segments per read
  int wsz = 0, waves = 0, words = 0;  // WindowsRoll: window in s-mers, reads per workgroup, code words per read
  size_t lds_bytes = 0;        // ... and its dynamic LDS
  unsigned grid = 0;           // workgroups of the form's main kernels (WinOnce: the chunk passes, 0 = no chunks)
  unsigned grid2 = 0;          // ... of the list walker behind them (WinOnce: of the gather)
  // side buffer: counts per (read, segment); the list's counter; the list (segments or reads left to the fallback); marks per segment
  size_t side_words = 0;
  K1Region counts, counter, list, marks;
  size_t win_words = 0, win_chunk_words = 0;  // WinOnce: h / kept / rank, cnt / cbase
};

inline unsigned k1_min_u(uint64_t a, uint64_t b) { return (unsigned)(a < b ? a : b); }

// Batches of whole genomes, asked before a batch is staged (which streams and workspace slot it gets): the segment forms' condition below
// without its terms on scratch and on n_reads * segs, which are not known yet.  Harmless: the answer places work, it chooses no kernel — a
// batch of such reads that the plan then serves with the workgroup-per-read form (no scratch: nothing above -u; more than 2^21 segments)
// runs on the streams of a whole-genome batch, with the same results.
inline bool k1_whole_genomes(int mode, bool paired, uint32_t max_read_len) { return !paired && mode == 0 && max_read_len > (uint32_t)K1SEG; }

inline K1Plan k1_plan(const K1Shape& s) {
  K1Plan p;
  p.debug = s.knobs.debug;
  p.max_read_len = s.max_read_len;
  if (s.n_reads == 0) return p;
  const int f = s.knobs.flags, ws = (int)s.w_or_s;
  auto place = [&p](K1Region& r, size_t len) {
    r.off = p.side_words;
    r.len = len;
    p.side_words += len;
  };
  // sliding windows of plain / FracMinHash k-mers that overlap: each staged base hashed once
  if (s.win.present && s.knobs.win_once && s.mode == 0 && !s.paired && s.k <= K1_SCAN_MAX_K && s.win.step < s.win.window) {
    p.form = K1Form::WinOnce;
    p.grid = s.win.n_chunks ? k1_min_u((s.win.n_chunks + 3) / 4, 65536) : 0;
    p.grid2 = k1_min_u(((uint64_t)s.n_reads + 3) / 4, 65536);
    p.win_words = s.win.sb + 1;
    p.win_chunk_words = s.win.n_chunks + 1;
    return p;
  }
  // whole genomes: segments of a read on their own workgroups, then an ordered pack
  const uint32_t segs = (s.max_read_len + (uint32_t)K1SEG - 1) / (uint32_t)K1SEG;
  if (s.mode == 0 && !s.paired && segs > 1 && s.have_scratch && (uint64_t)s.n_reads * segs <= K1_SEG_MAX_WGS) {
    const unsigned wgs = s.n_reads * segs;
    p.segs = segs;
    p.grid = wgs;
    place(p.counts, wgs);
    if (s.k <= K1_SEG_MAX_K && !(f & (K1F_SEG_HASH | K1F_SEG_ROLL))) {
      p.form = K1Form::SegRoll2;  // 2-bit codes; the segments it cannot take go on a list for the byte kernel
      // a packed batch with a run of foreign bytes per 4 kb or more is not what the direct form is for: expanded whole
      p.codes_direct = s.packed.present && s.knobs.codes_mode != 0 && !s.win.present && s.packed.text_is_seqs &&
                       (s.knobs.codes_mode == 2 || (uint64_t)s.packed.n_exc <= s.packed.n_bases / 4096 + 64);
      const bool runs = p.codes_direct && s.packed.n_exc > 0;
      p.list_fallback = !p.codes_direct || runs;  // (codes without a foreign byte: nothing gets on the list, nothing reads text)
      // a grid that fills the chip once (2 workgroups of 8 waves per CU) walks the list
      p.grid2 = k1_min_u(wgs, 512);
      place(p.counter, 1);
      place(p.list, wgs);
      if (runs) place(p.marks, wgs);
    } else {
      p.form = s.k <= K1_SEG_MAX_K && !(f & K1F_SEG_HASH) ? K1Form::SegRoll : K1Form::SegHash;
    }
    return p;
  }
  if (s.max_read_len <= (uint32_t)K1_LONG_READ) {
    p.form = K1Form::Short;
    p.grid = k1_min_u(((uint64_t)s.n_reads + 3) / 4, 32768);
    return p;
  }
  p.grid = k1_min_u(s.n_reads, 65536);
  if (s.mode != 0 && s.have_scratch && wave_windows_usable(s.mode, s.k, ws) && !(f & K1F_NO_WAVE)) {  // window sketches: the barrier-free form
    p.form = K1Form::WindowsWave;
    p.adj_done = true;
    // closed syncmers with a window of 12 / 16 / 20 / 24 / 32 s-mers (k - s = 6 .. 16), single-end: the rolling kernel first, k1_windows_wave
    // behind it for the reads it leaves on its list
    const int wsz = s.mode == 2 ? 2 * (s.k - ws) : 0;
    const int words = wr_words_for((int)s.max_read_len);
    // reads (= waves) per workgroup: LDS per wave (k-mer ring 8 KB + 2-bit codes of the longest read) decides how many waves a CU holds
    int waves = s.knobs.wr_waves == 1 || s.knobs.wr_waves == 4 ? s.knobs.wr_waves : 2;
    while (waves > 1 && wr_lds_bytes(wsz, words, waves) > K1_LDS_MAX) waves >>= 1;
    // (no read of the batch can exceed the -u / wave-sort bound — planting, a huge -u —: the fused path is nobody's, the old kernel alone)
    const bool any_fused = (long long)s.max_read_len > (long long)(s.dedup_threshold > K1_WAVE_SORT_CAP ? s.dedup_threshold : K1_WAVE_SORT_CAP);
    const bool wsz_ok = wsz == 12 || wsz == 16 || wsz == 20 || wsz == 24 || wsz == 32;
    if (s.mode == 2 && wsz_ok && s.k <= 64 && !s.paired && !(f & K1F_NO_ROLL) && any_fused && wr_lds_bytes(wsz, words, waves) <= K1_LDS_MAX) {
      p.form = K1Form::WindowsRoll;
      p.list_fallback = true;
      p.wsz = wsz;
      p.waves = waves;
      p.words = words;
      p.lds_bytes = wr_lds_bytes(wsz, words, waves);
      p.grid = (s.n_reads + waves - 1) / waves;
      p.grid2 = k1_min_u(k1_min_u(s.n_reads, 65536), 1024);
      place(p.counter, 1);
      place(p.list, s.n_reads);
    }
    return p;
  }
  if (!wg_lds_usable(s.mode, s.k, ws)) {
    p.form = K1Form::WgGlobal;
    return p;
  }
  p.form = K1Form::Wg;
  p.adj_done = s.mode != 0 && s.have_scratch && (f & K1F_FUSED_ADJ);
  return p;
}

}  // namespace kmcpg
