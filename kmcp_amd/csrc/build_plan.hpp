// build_plan.hpp — the block layout of `kmcp index` as a function of the per-column k-mer counts (kmcp/cmd/index.go:657-682, :787-894,
// :936-946, :1023), the partition of the blocks into rounds that fit a matrix budget, and the writers of the files that do not depend on
// the matrices (.uniki header, index/serialization.go:159-300; __db.yml, util-db-info.go:46-79; __name_mapping.tsv, index.go:1375-1393).
// Host-only C++17 without HIP (tests/build_plan_check.cpp compiles it with g++; go_pow comes from fpr.cpp).  kmcpg_build_db (build.cpp)
// and the kmcpg_builder handle (builder.cpp) both take layout and files from here, so the two ways to build cannot drift apart.
//
//   order      columns sorted by k-mer count ascending (index.go:667); the reference's parallel quicksort is unstable, input order
//              breaks ties here
//   sblock     -b, or ((int)(#cols / -j) + 7) / 8 * 8, clamped to [8, #cols]                                       (index.go:671-682)
//   tiers      up to -x k-mers, up to -8, up to -1, above: blocks of -b, -X, 8 and 1 columns, a tier change closing the open block;
//              when -X >= -b the -x tier does not exist (index.go:684-689) and the columns between -8 and -1 keep blocks of -b columns
//   empties    a column without k-mers is in no block                                                               (index.go:799-801)
//   NumSigs    CalcSignatureSize of the block's fullest column (util-hash.go:46-50), then uniform_sigs 1 / 2 (kmcp_gpu.h)
//   rounds     blocks in file order; a round closes when the next block's matrix_bytes + 8 would exceed the budget
#pragma once
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/kmcp_gpu.h"
#include "fpr.hpp"

namespace kmcpg {

// what the layout and the file headers need of a column
struct PlanCol {
  const char* name;
  uint64_t gsize;
  uint32_t chunk_idx, chunks;
  uint64_t n_hashes;
};

struct PlanBlock {
  std::vector<uint32_t> cols;  // input indices, in block order
  int tier = 0;
  uint64_t num_sigs = 0;
  uint32_t row_bytes = 0;
  uint64_t matrix_bytes = 0;  // num_sigs * row_bytes
};

struct BuildPlan {
  int sblock = 0;
  uint64_t total_kmers = 0;
  std::vector<PlanBlock> blocks;
};

// CalcSignatureSize (util-hash.go:46-50)
inline uint64_t signature_size(uint64_t n, int h, double fpr) {
  const double ratio = (double)(-h) / log(1.0 - go_pow(fpr, 1.0 / (double)h));
  return (uint64_t)ceil((double)n * ratio);
}

// the checks of kmcpg_build_db on its configuration that need no column; "" = fine
inline std::string build_cfg_error(const kmcpg_build_cfg& cfg) {
  if (cfg.num_hashes < 1 || cfg.num_hashes > 4 || !(cfg.fpr > 0 && cfg.fpr < 1) || cfg.k < 1 || cfg.k > 255) return "bad build configuration";
  return "";
}

// counts[i] = k-mers of column i (input order).  Returns "" and fills *out, or the message of the refusal.
inline std::string build_plan(const uint64_t* counts, uint32_t n_cols, const kmcpg_build_cfg& cfg, BuildPlan* out) {
  char msg[160];
  out->blocks.clear();
  out->total_kmers = 0;
  std::vector<uint32_t> order(n_cols);
  for (uint32_t i = 0; i < n_cols; i++) {
    order[i] = i;
    out->total_kmers += counts[i];
  }
  std::stable_sort(order.begin(), order.end(), [counts](uint32_t a, uint32_t b) { return counts[a] < counts[b]; });
  int sblock = cfg.block_size > 0 ? cfg.block_size : ((int)((double)n_cols / (double)std::max(1, cfg.threads)) + 7) / 8 * 8;  // index.go:671-682
  if (sblock > (int)n_cols) sblock = (int)n_cols;
  if (sblock < 8) sblock = 8;
  out->sblock = sblock;
  const uint64_t thr_x = cfg.kmers_x ? cfg.kmers_x : 10ull << 20, thr_8 = cfg.kmers_8 ? cfg.kmers_8 : 20ull << 20,
                 thr_1 = cfg.kmers_1 ? cfg.kmers_1 : 200ull << 20;
  if (!(thr_x < thr_8 && thr_8 < thr_1)) return "block thresholds must satisfy -x < -8 < -1";  // index.go:242-257
  const int size_x = cfg.block_size_x ? cfg.block_size_x : 256;
  if (size_x <= 8 || size_x % 8) {  // index.go:225-230
    snprintf(msg, sizeof msg, "-X/--block-sizeX should be a multiple of 8 greater than 8: %d", size_x);
    return msg;
  }
  if (cfg.uniform_sigs < 0 || cfg.uniform_sigs > 2) return "uniform_sigs must be 0, 1 or 2";
  const bool skip_x = size_x >= sblock;
  auto tier = [&](uint64_t km) { return km > thr_1 ? 3 : km > thr_8 ? 2 : (!skip_x && km > thr_x) ? 1 : 0; };
  const int tier_size[4] = {sblock, size_x, skip_x ? sblock : 8, 1};
  for (size_t i = 0; i < order.size();) {
    if (counts[order[i]] == 0) {  // empty inputs are skipped (index.go:799-801)
      i++;
      continue;
    }
    const int t = tier(counts[order[i]]);
    PlanBlock b;
    b.tier = t;
    uint64_t max_elems = 0;
    while ((int)b.cols.size() < tier_size[t] && i < order.size() && tier(counts[order[i]]) == t) {
      max_elems = std::max(max_elems, counts[order[i]]);
      b.cols.push_back(order[i++]);
    }
    b.num_sigs = signature_size(max_elems, cfg.num_hashes, cfg.fpr);  // from the fullest column (index.go:936-946, :1023)
    out->blocks.push_back(std::move(b));
  }
  // uniform_sigs (not in the reference; kmcp_gpu.h says why): a larger filter only lowers a block's false-positive rate, so rounding
  // NumSigs UP is always safe.  1: every block of a tier gets the tier's largest NumSigs; 2: NumSigs is rounded up to a geometric ladder
  // of ratio 5/4 above the tier's smallest
  if (cfg.uniform_sigs == 1 || cfg.uniform_sigs == 2) {
    for (int t = 0; t < 4; t++) {
      uint64_t lo = ~0ull, hi = 0;
      for (const auto& b : out->blocks)
        if (b.tier == t) {
          lo = std::min(lo, b.num_sigs);
          hi = std::max(hi, b.num_sigs);
        }
      if (hi == 0) continue;
      for (auto& b : out->blocks) {
        if (b.tier != t) continue;
        if (cfg.uniform_sigs == 1) b.num_sigs = hi;
        else {
          uint64_t step = lo;
          while (step < b.num_sigs) step = step + step / 4 + 1;
          b.num_sigs = std::min(step, std::max(hi, b.num_sigs));
        }
      }
    }
  }
  for (auto& b : out->blocks) {
    b.row_bytes = ((uint32_t)b.cols.size() + 7) / 8;
    b.matrix_bytes = b.num_sigs * (uint64_t)b.row_bytes;
  }
  return "";
}

// round[b] = the round block b is built in, *n_rounds = how many.  A matrix is resident with 8 bytes behind it (the aligned word of its
// last byte may reach past the end), so a block counts matrix_bytes + 8.  "" = fine; a block above the budget is named.
inline std::string build_rounds(const BuildPlan& plan, uint64_t budget, std::vector<uint32_t>* round, uint32_t* n_rounds) {
  round->assign(plan.blocks.size(), 0);
  uint32_t r = 0;
  uint64_t used = 0;
  for (size_t b = 0; b < plan.blocks.size(); b++) {
    const uint64_t need = plan.blocks[b].matrix_bytes + 8;
    if (need > budget) {
      char msg[200];
      snprintf(msg, sizeof msg, "block %zu needs %llu bytes (its matrix of %llu + 8), above the matrix budget of %llu bytes", b + 1,
               (unsigned long long)need, (unsigned long long)plan.blocks[b].matrix_bytes, (unsigned long long)budget);
      return msg;
    }
    if (used && used + need > budget) {
      r++;
      used = 0;
    }
    used += need;
    (*round)[b] = r;
  }
  *n_rounds = plan.blocks.empty() ? 0 : r + 1;
  return "";
}

inline void plan_be32(FILE* f, uint32_t v) {
  const uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
  fwrite(b, 1, 4, f);
}
inline void plan_be64(FILE* f, uint64_t v) {
  plan_be32(f, (uint32_t)(v >> 32));
  plan_be32(f, (uint32_t)v);
}

// mkdir -p; -1 with errno set when a component cannot be made
inline int plan_mkdirs(const std::string& d) {
  std::string cur;
  for (size_t i = 0; i <= d.size(); i++) {
    if (i == d.size() || d[i] == '/') {
      if (!cur.empty() && mkdir(cur.c_str(), 0755) != 0 && errno != EEXIST) return -1;
    }
    if (i < d.size()) cur.push_back(d[i]);
  }
  return 0;
}

inline std::string block_file_name(size_t block) {
  char name[64];
  snprintf(name, sizeof name, "_block%03zu.uniki", block + 1);  // index.go:1283-1285
  return name;
}

// everything of a .uniki file in front of the matrix (index/serialization.go:159-300)
inline void write_uniki_header(FILE* f, const kmcpg_build_cfg& cfg, const PlanCol* cols, const PlanBlock& b) {
  const uint32_t n = (uint32_t)b.cols.size();
  fwrite(".kmcpidx", 1, 8, f);
  const uint8_t meta[4] = {4, (uint8_t)cfg.k, (uint8_t)((cfg.canonical ? 1 : 0) | 2 /* COMPACT = !faster (index.go:207) */), (uint8_t)cfg.num_hashes};
  fwrite(meta, 1, 4, f);
  plan_be64(f, b.num_sigs);
  plan_be32(f, n);
  for (uint32_t c : b.cols) {
    plan_be32(f, (uint32_t)strlen(cols[c].name) + 1);
    fwrite(cols[c].name, 1, strlen(cols[c].name), f);
    fputc('\n', f);
  }
  plan_be32(f, n);
  for (uint32_t c : b.cols) {
    plan_be32(f, 1);
    plan_be64(f, cols[c].gsize);
  }
  plan_be32(f, n);
  for (uint32_t c : b.cols) {
    plan_be32(f, 1);
    plan_be32(f, cols[c].chunk_idx + (cols[c].chunks << 16));  // index.go:1096
  }
  for (uint32_t c : b.cols) plan_be64(f, cols[c].n_hashes);
}

// <dir>/__db.yml (util-db-info.go:46-79); false when the file cannot be written
inline bool write_db_yml(const std::string& dir, const kmcpg_build_cfg& cfg, uint32_t n_cols, const BuildPlan& plan) {
  FILE* f = fopen((dir + "/__db.yml").c_str(), "w");
  if (!f) return false;
  auto b = [](int v) { return v ? "true" : "false"; };
  fprintf(f, "version: 4\nunikiVersion: 4\nalias: %s\nk: %d\nks:\n- %d\nhashed: true\ncanonical: %s\n", cfg.alias ? cfg.alias : "kmcp-gpu-db", cfg.k, cfg.k,
          b(cfg.canonical));
  fprintf(f, "scaled: %s\nscale: %u\nminimizer: %s\nminimizer-w: %u\nsyncmer: %s\nsyncmer-s: %u\n", b(cfg.scale > 1), cfg.scale > 1 ? cfg.scale : 1,
          b(cfg.minimizer_w > 0), cfg.minimizer_w, b(cfg.syncmer_s > 0), cfg.syncmer_s);
  fprintf(f, "split-seq: %s\nsplit-size: %d\nsplit-num: %d\nsplit-overlap: %d\ncompact-size: true\n", b(cfg.split_seq), cfg.split_size, cfg.split_num,
          cfg.split_overlap);
  fprintf(f, "hashes: %d\nfpr: %.17g\nnumNameGroups: %u\nblocksize: %d\ntotalKmers: %llu\nfiles:\n", cfg.num_hashes, cfg.fpr, n_cols, plan.sblock,
          (unsigned long long)plan.total_kmers);
  for (size_t i = 0; i < plan.blocks.size(); i++) fprintf(f, "- %s\n", block_file_name(i).c_str());
  return fclose(f) == 0;
}

// <dir>/__name_mapping.tsv (index.go:1375-1393): every input column, empty ones included
inline void write_name_mapping(const std::string& dir, const PlanCol* cols, uint32_t n_cols) {
  FILE* f = fopen((dir + "/__name_mapping.tsv").c_str(), "w");
  if (!f) return;
  for (uint32_t i = 0; i < n_cols; i++) fprintf(f, "%s\t%s\n", cols[i].name, cols[i].name);
  fclose(f);
}

}  // namespace kmcpg
