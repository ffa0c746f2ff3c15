"""A plain Python restatement of the binning pass of `kmcp profile -B` (kmcp/cmd/profile.go:2591-2784) for the tests: a map of
target -> rows per query, the three row cuts, and an LCA fold over the targets' TaxIds — NOT the min / max over a pre-order numbering of
kmcp_amd/csrc/bin_rule.hpp, so that the two can be held against each other.

What is ours and not the reference's ("Taxonomic binning"): TaxIds go through merged.dmp before anything else, so a
merged TaxId is printed resolved; the LCA of a TaxId that is deleted or absent from nodes.dmp with any OTHER TaxId is 0, as is the LCA of
TaxIds under different roots (the reference asks a third-party module); a whitelisted reference without a TaxId is refused up front.
Lines are written in the order the queries end (the reference's)."""
from tests import profile_contract as PC

HEADER = ("# This is the bioboxes.org binning output format at\n# https://github.com/bioboxes/rfc/tree/master/data-format\n@Version:0.10.0\n"
          "@SampleID:{}\n@@SEQUENCEID\tTAXID\n")


class BinningError(Exception):
    """what the reference reports through checkError (exit status 255)"""


def file_name(flag):
    """profile.go:505-507"""
    return flag if flag.endswith(".binning") or flag.endswith(".binning.gz") else flag + ".binning.gz"


def lca(tax, a, b):
    a, b = tax.resolve(a), tax.resolve(b)
    if a == b:
        return a
    return tax.lca(a, b)  # 0 with 0, with an unknown TaxId, and under different roots


def binning(texts, whitelist, taxid_map, tax, sample_id="", max_fpr=0.01, min_qcov=0.55, top_n=0, keep_perfect=False, keep_main=False, max_gap=0.4):
    """texts: one search result per input file; whitelist: the names of the references the EM ended with -> the binning file's text"""
    whitelist = set(whitelist)
    for name in sorted(whitelist):
        if name not in taxid_map:
            raise BinningError(f"unknown taxid for {name}, please check taxid mapping file(s)")
    out = [HEADER.format(sample_id)]

    def finish(query, matches):
        if len(matches) > 1:
            taxids = [taxid_map[ms[0]["target"]] for ms in matches.values()]
            t = tax.resolve(taxids[0])
            for t2 in taxids[1:]:
                t = lca(tax, t, t2)
            out.append(f"{query}\t{t}\n")
        else:
            for ms in matches.values():
                out.append(f"{query}\t{tax.resolve(taxid_map[ms[0]['target']])}\n")

    for text in texts:
        rows, _, _ = PC.read_search_result(text, max_fpr, min_qcov)
        matches, prev_query, p_score, n_score, process = {}, "", 1024, 0, True
        for match in rows:
            if match["target"] not in whitelist:  # skip matches of unwanted targets
                continue
            if prev_query != match["query"]:
                finish(prev_query, matches)
                matches, p_score, n_score, process = {}, 1024, 0, True
            elif keep_perfect:
                if not process:
                    prev_query = match["query"]
                    continue
                if p_score == 1 and match["qcov"] < 1:
                    process = False
                    prev_query = match["query"]
                    continue
            elif keep_main and p_score <= 1:
                if not process:
                    prev_query = match["query"]
                    continue
                if p_score - match["qcov"] > max_gap:
                    process = False
                    prev_query = match["query"]
                    continue
            if top_n > 0:
                if not process:
                    prev_query = match["query"]
                    continue
                if match["qcov"] < p_score:
                    n_score += 1
                    if n_score > top_n:
                        process = False
                        prev_query = match["query"]
                        continue
            matches.setdefault(match["target"], []).append(match)
            prev_query = match["query"]
            p_score = match["qcov"]
        finish(prev_query, matches)
    return "".join(out)


def whitelist_of_profile(text):
    """the reference names of a profile table: the first tab-separated column of every line that does not start with '#'"""
    return [l.split("\t", 1)[0] for l in text.splitlines() if l and not l.startswith("#")]
