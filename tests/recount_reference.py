"""A plain Python restatement of stage 3/4 of `kmcp profile` (kmcp/cmd/profile.go:1282-1888) for the tests: the same loop with its
`continue` paths, a dict of lists per query, float64 `+= 1/m`, `prop`, the LITERAL species rule (the LCA of the survivors' TaxIds), the
elimination as the double loop the reference writes — the j loop goes on after i was deleted — and MeanStdev (util.go:381).  Its one
departure: the reference sorts a read's targets unstably over a randomly ordered map; here the sort is stable over the order of the
targets' first rows (the tie rule of kmcp_amd/csrc/recount_rule.hpp).  Stages 1 and 2 come from tests/refstats_reference.py and
tests/cooccur_reference.py; rows are read with tests/profile_contract.py.

The reference prints nothing after stage 3; `render` writes kmcp-refstats --recount's format from the reference's own per-target state
(every shown figure is computed for every reference, also where the reference leaves the loop at an earlier test)."""
import math

from tests import cooccur_reference as CR
from tests import profile_contract as PC
from tests import refstats_reference as RR

HEADER = "#ref\tchunks\ttLen\treads\tureads\thicUreads\tchunksFrac\tdepthStdev\tcoverage\tverdict\tchunkReads\tchunkUreads\tchunkHicUreads\tchunkBases\n"

# profile.go:243-313 (mode 3: the flag defaults, :3173-3179): mode -> (r minReads, u minUReads, U minHicUreads, P HicUreadsMinProp, d maxFragsDepthStdev)
PRESETS = {0: (1, 1, 1, 0.01, 10), 1: (5, 2, 1, 0.1, 2), 2: (10, 5, 2, 0.2, 2), 3: (50, 20, 5, 0.1, 2), 4: (100, 50, 10, 0.1, 2), 5: (100, 50, 10, 0.15, 1.5)}


class Target:
    def __init__(self, m):
        self.name, self.gsize, n = m["target"], m["gsize"], m["chunks"]
        self.match, self.uniq, self.uniq_hic, self.qlen = [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n


def mean_stdev(values):
    n = len(values)
    if n == 0:
        return 0.0, 0.0
    if n == 1:
        return values[0], 0.0
    mean = sum(values) / float(n)
    variance = 0.0
    for v in values:
        variance += (v - mean) * (v - mean)
    return mean, math.sqrt(variance / float(n))


def stage3(texts, profile, amb, max_fpr=0.01, min_qcov=0.55, top_n=0, keep_perfect=False, keep_main=False, max_gap=0.4, hic_min_qcov=0.75,
           level="species", taxid_map=None, tax=None, no_amb_corr=False, min_dreads_prop=0.05, max_mismatch_err=0.05):
    """profile: name -> (SumMatch, SumUniqMatch) of the targets stage 1 kept; amb: stage 2's a -> b -> count, a < b.
    -> (profile2: name -> Target, recounted reads, reads that ended with one target, reads that lost a target)"""
    level_species = level.lower() == "species"
    profile2, counts = {}, [0, 0, 0]
    one_minus = 1 - min_dreads_prop

    def target(h, m):
        t = profile2.get(h)
        if t is None:
            t = profile2[h] = Target(m)
        return t

    def finish(matches):
        if not matches:
            return
        counts[0] += 1
        uniq_match = False
        if len(matches) > 1:
            if not no_amb_corr:
                hss = sorted(matches, key=lambda h: -matches[h][0]["qcov"])  # stable: ties keep the order of the first rows
                hsm = [False] * len(hss)
                n = len(hss)
                for i in range(n - 1):
                    if hsm[i]:
                        continue
                    for j in range(i + 1, n):
                        if hsm[j]:
                            continue
                        hi, hj = hss[i], hss[j]
                        h1, h2 = sorted((hi, hj))
                        n_shared = float(amb.get(h1, {}).get(h2, 0))
                        if profile[hi][0] * one_minus >= n_shared and profile[hj][1] < profile[hi][1] * max_mismatch_err:
                            hsm[j] = True
                        elif profile[hj][0] * one_minus >= n_shared and profile[hi][1] < profile[hj][1] * max_mismatch_err:
                            hsm[i] = True
                if any(hsm):
                    counts[2] += 1
                for i, h in enumerate(hss):
                    if hsm[i]:
                        del matches[h]
            if len(matches) > 1:  # redistribute matches
                same_species = False
                if level_species:
                    taxids = []
                    for ms in matches.values():
                        if ms[0]["target"] not in (taxid_map or {}):
                            raise RR.RefstatsError(f"unknown taxid for {ms[0]['target']}, please check taxid mapping file(s)")
                        taxids.append(taxid_map[ms[0]["target"]])
                    node = tax.resolve(taxids[0]) if tax.known(taxids[0]) else 0
                    for t2 in taxids[1:]:
                        node = tax.lca(node, t2)
                    same_species = tax.at_or_below_species(node)
                prop = 1.0 / float(len(matches))
                for h, ms in matches.items():
                    size = float(len(ms))
                    first = True
                    for m in ms:
                        t = target(h, m)
                        if first:
                            if level_species and same_species:
                                t.uniq[m["chunk_idx"]] += 1.0 / size
                                if m["qcov"] >= hic_min_qcov:
                                    t.uniq_hic[m["chunk_idx"]] += 1.0 / size
                            first = False
                        t.qlen[m["chunk_idx"]] += float(m["qlen"]) * prop / size
                        t.match[m["chunk_idx"]] += 1.0 / size
            else:
                uniq_match = True
        elif len(matches) == 1:
            uniq_match = True
        if uniq_match:
            counts[1] += 1
            for h, ms in matches.items():
                size = float(len(ms))
                first = True
                for m in ms:
                    t = target(h, m)
                    if first:
                        t.uniq[m["chunk_idx"]] += 1
                        if m["qcov"] >= hic_min_qcov:
                            t.uniq_hic[m["chunk_idx"]] += 1
                        first = False
                    t.qlen[m["chunk_idx"]] += float(m["qlen"]) / size
                    t.match[m["chunk_idx"]] += 1.0 / size

    for text in texts:
        rows, _, _ = PC.read_search_result(text, max_fpr, min_qcov)
        matches, prev_query, p_score, n_score, process = {}, "", 1024, 0, True
        for match in rows:
            if match["target"] not in profile:  # skip matches of unwanted targets
                continue
            if prev_query != match["query"]:
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
        finish(matches)
    return profile2, counts[0], counts[1], counts[2]


def judge(t, r, u, U, P, p, d, norm="mean"):
    """profile.go:1743-1888, the tests in its order -> dict of what the file shows"""
    sum_uniq, sum_hic, sum_match = sum(t.uniq), sum(t.uniq_hic), sum(t.match)
    frags = sum(1.0 for c in t.match if c >= r) / float(len(t.match))
    qlens = sum(t.qlen)
    rel = [c2 / qlens * float(len(t.qlen)) for c2 in t.qlen] if qlens else [0.0] * len(t.qlen)
    _, std = mean_stdev(rel)
    if norm == "mean":
        cov = qlens / float(t.gsize)
    else:
        nz = [c for c in t.qlen if c != 0]
        cov = (min(nz) if norm == "min" else max(nz)) * float(len(t.qlen)) / float(t.gsize)
    if sum_uniq < u:
        v = "few-unique"
    elif sum_hic < U:
        v = "few-hic-unique"
    elif sum_hic < P * sum_uniq:
        v = "low-hic-unique-prop"
    elif frags < p:
        v = "low-chunks-fraction"
    elif std > d:
        v = "high-depth-stdev"
    else:
        v = "ok"
    return dict(reads=sum_match, ureads=sum_uniq, hic=sum_hic, frags=frags, stdev=std, coverage=cov, verdict=v)


def render(profile2, n, n_unique, n_corrected, thresholds, norm="mean"):
    out = [f"# recounted reads: {n}\n# unique reads: {n_unique}\n# corrected reads: {n_corrected}\n", HEADER]
    for name in sorted(profile2, key=lambda s: s.encode()):
        t = profile2[name]
        j = judge(t, *thresholds, norm=norm)
        lists = [",".join("%.6f" % x for x in l) for l in (t.match, t.uniq, t.uniq_hic)] + [",".join("%.4f" % x for x in t.qlen)]
        out.append("\t".join([name, str(len(t.match)), str(t.gsize), "%.6f" % j["reads"], "%.6f" % j["ureads"], "%.6f" % j["hic"], "%.4f" % j["frags"],
                              "%.6f" % j["stdev"], "%.6f" % j["coverage"], j["verdict"]] + lists) + "\n")
    return "".join(out)


def recount(texts, mode=3, min_hic_ureads_qcov=None, min_chunks_fraction=None, keep_main_matches=False, min_qcov=0.55, max_fpr=0.01, top_n=0,
            keep_perfect=False, max_gap=0.4, level="species", taxid_map=None, tax=None, r=None, u=None, U=None, P=None, d=None,
            min_dreads_prop=0.05, max_mismatch_err=0.05, no_amb_corr=False, norm="mean"):
    """what `kmcp-refstats ... --recount FILE` writes into FILE"""
    h, p, main = RR.params(mode, min_hic_ureads_qcov, min_chunks_fraction, keep_main_matches, min_qcov)
    cuts = dict(max_fpr=max_fpr, min_qcov=min_qcov, top_n=top_n, keep_perfect=keep_perfect, keep_main=main, max_gap=max_gap)
    prof, _, _ = RR.stage1(texts, hic_min_qcov=h, level=level, taxid_map=taxid_map, tax=tax, **cuts)
    kept = {}
    for name, t in prof.items():
        v, reads, ureads, _, _ = RR.verdict(t, p)
        if v == "ok":
            kept[name] = (float(reads), float(ureads))
    amb = CR.stage2(texts, set(kept), **cuts)
    prof2, n, nu, nc = stage3(texts, kept, amb, hic_min_qcov=h, level=level, taxid_map=taxid_map, tax=tax, no_amb_corr=no_amb_corr,
                              min_dreads_prop=min_dreads_prop, max_mismatch_err=max_mismatch_err, **cuts)
    pr = PRESETS[mode]
    th = (pr[0] if r is None else r, pr[1] if u is None else u, pr[2] if U is None else U, pr[3] if P is None else P, p, pr[4] if d is None else d)
    return render(prof2, n, nu, nc, th, norm=norm)


def parse(text):
    """a recount file -> (the three '#' counts, {ref: dict(verdict, numbers: the scalar figures, lists: the four per-chunk lists)})"""
    lines = text.splitlines()
    heads = [int(l.split(": ")[1]) for l in lines[:3]]
    assert lines[3] + "\n" == HEADER
    refs = {}
    for l in lines[4:]:
        f = l.split("\t")
        refs[f[0]] = dict(chunks=int(f[1]), tlen=int(f[2]), numbers=[float(x) for x in f[3:9]], verdict=f[9],
                          lists=[[float(x) for x in c.split(",")] for c in f[10:14]])
    return heads, refs
