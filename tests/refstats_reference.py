"""A plain Python restatement of stage 1/4 of `kmcp profile` (kmcp/cmd/profile.go:741-1099) for the tests: the same loop with its
`continue` paths, a dict of lists per query, float counters as the reference keeps them (Match gets 1/m per row), the LITERAL species
rule (the LCA of the query's TaxIds, then "at or below rank species"; tests/filter_reference.py) and the reference's stale
`theSameSpecies` replaced by the intended rule at --level strain (False).  Rows are read with tests/profile_contract.py.

The reference prints nothing after stage 1; `render` writes kmcp-refstats' format from the reference's own per-target state."""
from tests import filter_reference as FR
from tests import profile_contract as PC

HEADER = "#ref\tchunks\ttLen\treads\tureads\thicUreads\tchunksFrac\tverdict\tchunkReads\tchunkFirsts\tchunkUreads\tchunkHicUreads\n"

# profile.go:243-313: mode -> (hicUreadsMinQcov, minFragsProp, keepMainMatch)
PRESETS = {0: (0.7, 0.2, True), 1: (0.7, 0.6, False), 2: (0.7, 0.7, False), 3: (0.75, 0.8, False), 4: (0.8, 1.0, False), 5: (0.8, 1.0, False)}


class RefstatsError(Exception):
    """what the reference reports through checkError (exit status 255)"""


def params(mode=3, min_hic_ureads_qcov=None, min_chunks_fraction=None, keep_main_matches=False, min_qcov=0.55):
    """profile.go:315-421: the preset, overridden by a flag only when it was given; the FLAG's value (its default when absent) is what
    the range test sees"""
    if not 0 <= mode <= 5:
        raise RefstatsError(f"invalid profiling mode: {mode}")
    flag_h = 0.75 if min_hic_ureads_qcov is None else min_hic_ureads_qcov
    flag_p = 0.8 if min_chunks_fraction is None else min_chunks_fraction
    if flag_p < 0 or flag_p > 1:
        raise RefstatsError("min-chunks-fraction out of range")
    if flag_h <= 0 or flag_h > 1 or flag_h < min_qcov:
        raise RefstatsError("min-hic-ureads-qcov out of range")
    h, p, main = PRESETS[mode]
    if min_hic_ureads_qcov is not None:
        h = min_hic_ureads_qcov
    if min_chunks_fraction is not None:
        p = min_chunks_fraction
    return h, p, main or keep_main_matches


class Target:
    def __init__(self, m):
        self.name, self.gsize, n = m["target"], m["gsize"], m["chunks"]
        self.match, self.uniq, self.uniq_hic = [0.0] * n, [0.0] * n, [0.0] * n
        # what the reference does not keep but the output shows: rows and first rows per chunk, in integers
        self.rows, self.firsts = [0] * n, [0] * n


def stage1(texts, max_fpr=0.01, min_qcov=0.55, top_n=0, keep_perfect=False, keep_main=False, max_gap=0.4, hic_min_qcov=0.75,
           level="species", taxid_map=None, tax=None):
    """texts: one search result per input file -> (profile: name -> Target, matched reads, unique reads)"""
    level_species = level.lower() == "species"
    profile, n_reads, n_unique = {}, 0, 0

    def finish(matches):
        nonlocal n_reads, n_unique
        n_reads += 1
        same_species = False
        if level_species:
            taxids = []
            for ms in matches.values():
                if ms[0]["target"] not in (taxid_map or {}):
                    raise RefstatsError(f"unknown taxid for {ms[0]['target']}, please check taxid mapping file(s)")
                taxids.append(taxid_map[ms[0]["target"]])
            node = tax.resolve(taxids[0]) if tax.known(taxids[0]) else 0
            for t in taxids[1:]:
                node = tax.lca(node, t)
            same_species = tax.at_or_below_species(node)
        unique = len(matches) == 1 or same_species
        n_unique += unique
        for h, ms in matches.items():
            first = True
            for m in ms:
                t = profile.get(h)
                if t is None:
                    t = profile[h] = Target(m)
                if first:
                    if unique:
                        t.uniq[m["chunk_idx"]] += 1
                        if m["qcov"] >= hic_min_qcov:
                            t.uniq_hic[m["chunk_idx"]] += 1
                    t.firsts[m["chunk_idx"]] += 1
                    first = False
                t.match[m["chunk_idx"]] += 1.0 / float(len(ms))
                t.rows[m["chunk_idx"]] += 1

    for text in texts:
        rows, _, _ = PC.read_search_result(text, max_fpr, min_qcov)
        matches, prev_query, p_score, n_score, process = {}, "", 1024, 0, True
        for match in rows:
            if prev_query != match["query"]:  # new query
                if matches:
                    finish(matches)
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
        if matches:
            finish(matches)
    return profile, n_reads, n_unique


def verdict(t, min_chunks_fraction):
    """profile.go:1018-1095 in its order -> (verdict, SumMatch, SumUniqMatch, SumUniqMatchHic, FragsProp)"""
    sum_uniq = sum(t.uniq)
    sum_hic = sum(t.uniq_hic)
    frags = sum(1.0 for c in t.match if c > 0) / float(len(t.match))
    reads = sum(t.firsts)
    assert abs(sum(t.match) - reads) < 1e-6 * max(1, reads), "SumMatch is the number of reads"
    assert [c > 0 for c in t.match] == [c > 0 for c in t.rows]
    if sum_uniq < 1:
        v = "no-unique"
    elif sum_hic < 1:
        v = "no-hic-unique"
    elif frags < min_chunks_fraction:
        v = "low-chunks-fraction"
    else:
        v = "ok"
    return v, reads, int(sum_uniq), int(sum_hic), frags


def render(profile, n_reads, n_unique, min_chunks_fraction):
    out = [f"# matched reads: {n_reads}\n# unique reads: {n_unique}\n", HEADER]
    for name in sorted(profile, key=lambda s: s.encode()):
        t = profile[name]
        v, reads, ureads, hic, frags = verdict(t, min_chunks_fraction)
        lists = [",".join(str(int(x)) for x in l) for l in (t.rows, t.firsts, t.uniq, t.uniq_hic)]
        out.append("\t".join([name, str(len(t.match)), str(t.gsize), str(reads), str(ureads), str(hic), "%.4f" % frags, v] + lists) + "\n")
    return "".join(out)


def refstats(texts, mode=3, min_hic_ureads_qcov=None, min_chunks_fraction=None, keep_main_matches=False, min_qcov=0.55, **kw):
    h, p, main = params(mode, min_hic_ureads_qcov, min_chunks_fraction, keep_main_matches, min_qcov)
    prof, n, u = stage1(texts, min_qcov=min_qcov, keep_main=main, hic_min_qcov=h, **kw)
    return render(prof, n, u, p)


def verdicts_of(text):
    """the verdict column of a statistics file -> {ref: verdict}"""
    return {l.split("\t")[0]: l.split("\t")[7] for l in text.splitlines() if l and l[0] != "#"}
