"""A plain Python restatement of stage 2/4 of `kmcp profile` (kmcp/cmd/profile.go:1117-1279) for the tests: the same loop with its
`continue` paths — the one that skips the rows of targets stage 1 dropped comes BEFORE the query test —, ambMatch as a dict of dicts,
pScore = 1024, and the flush at the end of every file.  The kept set (the reference's `profile` map after stage 1) comes from
tests/refstats_reference.py; rows are read with tests/profile_contract.py.

The reference orients a pair by the targets' hashes and prints nothing after stage 2; `render` writes kmcp-refstats --cooccur's format,
the pair oriented by name."""
from tests import profile_contract as PC
from tests import refstats_reference as RR

HEADER = "#refA\trefB\treads\n"


def kept_set(texts, mode=3, min_hic_ureads_qcov=None, min_chunks_fraction=None, keep_main_matches=False, min_qcov=0.55, **kw):
    """stage 1 with kmcp-refstats' arguments -> (the targets with the verdict ok, the keep-main switch after the preset)"""
    h, p, main = RR.params(mode, min_hic_ureads_qcov, min_chunks_fraction, keep_main_matches, min_qcov)
    prof, _, _ = RR.stage1(texts, min_qcov=min_qcov, keep_main=main, hic_min_qcov=h, **kw)
    return {name for name, t in prof.items() if RR.verdict(t, p)[0] == "ok"}, main


def stage2(texts, profile, max_fpr=0.01, min_qcov=0.55, top_n=0, keep_perfect=False, keep_main=False, max_gap=0.4):
    """texts: one search result per input file; profile: the targets stage 1 kept -> ambMatch: a -> b -> count, a < b"""
    amb = {}

    def count(matches):
        if len(matches) > 1:  # skip uniq match
            hs = sorted(matches)
            for i in range(len(hs) - 1):
                for j in range(i + 1, len(hs)):
                    h1, h2 = hs[i], hs[j]
                    if h1 not in amb:
                        amb[h1] = {h2: 1}
                    else:
                        amb[h1][h2] = amb[h1].get(h2, 0) + 1

    for text in texts:
        rows, _, _ = PC.read_search_result(text, max_fpr, min_qcov)
        matches, prev_query, p_score, n_score, process = {}, "", 1024, 0, True
        for match in rows:
            if match["target"] not in profile:  # skip matches of unwanted targets
                continue
            if prev_query != match["query"]:  # new query
                count(matches)
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
                if match["qcov"] < p_score:  # match with a smaller score
                    n_score += 1
                    if n_score > top_n:
                        process = False
                        prev_query = match["query"]
                        continue
            matches[match["target"]] = None  # just need to collect keys
            prev_query = match["query"]
            p_score = match["qcov"]
        count(matches)
    return amb


def render(amb):
    rows = sorted((min(a, b, key=str.encode), max(a, b, key=str.encode), n) for a, bs in amb.items() for b, n in bs.items())
    rows.sort(key=lambda r: (r[0].encode(), r[1].encode()))
    return f"# pairs: {len(rows)}\n" + HEADER + "".join(f"{a}\t{b}\t{n}\n" for a, b, n in rows)


def cooccur(texts, max_fpr=0.01, top_n=0, keep_perfect=False, max_gap=0.4, level="species", taxid_map=None, tax=None, **stage1_args):
    """what `kmcp-refstats ... --cooccur FILE` writes into FILE"""
    min_qcov = stage1_args.get("min_qcov", 0.55)
    profile, main = kept_set(texts, max_fpr=max_fpr, top_n=top_n, keep_perfect=keep_perfect, max_gap=max_gap, level=level, taxid_map=taxid_map, tax=tax,
                             **stage1_args)
    return render(stage2(texts, profile, max_fpr=max_fpr, min_qcov=min_qcov, top_n=top_n, keep_perfect=keep_perfect, keep_main=main, max_gap=max_gap))


def pairs_of(text):
    """a pairs file -> {(refA, refB): reads}"""
    return {tuple(l.split("\t")[:2]): int(l.split("\t")[2]) for l in text.splitlines() if l and l[0] != "#"}
