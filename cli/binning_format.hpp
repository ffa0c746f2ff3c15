// binning_format.hpp — the binning file of `kmcp profile -B` (kmcp/cmd/profile.go:503-507, :2608-2612, :2677): the CAMI / bioboxes.org
// binning format, one line `query<TAB>TaxId` per binned read.  Shared by kmcp-refstats --binning and kmcp-search --binning.
#pragma once
#include <cstdint>
#include <string>

#include "tsv_out.hpp"

namespace binning_format {

// the file the reference writes for a -B value: as given when it ends in .binning or .binning.gz, else with .binning.gz appended
inline std::string file_name(const std::string& flag) {
  const auto ends = [&](const char* s) {
    const size_t n = strlen(s);
    return flag.size() >= n && flag.compare(flag.size() - n, n, s) == 0;
  };
  return ends(".binning") || ends(".binning.gz") ? flag : flag + ".binning.gz";
}

inline void write_header(tsv_out::Out& out, const std::string& sample_id) {
  out.write("# This is the bioboxes.org binning output format at\n");
  out.write("# https://github.com/bioboxes/rfc/tree/master/data-format\n");
  out.write("@Version:0.10.0\n");
  out.write("@SampleID:" + sample_id + "\n");
  out.write("@@SEQUENCEID\tTAXID\n");
}

inline void write_line(tsv_out::Out& out, const char* query, size_t n, uint32_t taxid) {
  char num[16];
  const int m = snprintf(num, sizeof num, "\t%u\n", taxid);
  out.write(query, n);
  out.write(num, (size_t)m);
}

}  // namespace binning_format
