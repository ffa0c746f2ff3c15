"""Stage 4/4 of `kmcp profile` — abundance estimation by EM — restated for the tests.

OUR rule (kmcp_amd/csrc/em_rule.hpp) in Python integers: `read_adds` (one read in one pass), `pass_cols` (a pass over reads), `em_cols`
(what kmcpg_em_read returns), `rollup`, `run`, `finish` and `table`.  Everything the project computes is compared with it for EXACT
equality.  Python's float is the IEEE double of the C++ code and `/`, `*`, `+` round the same way, so the quotas and the roll-up's doubles
have the same bits.  This is restatement (a).  Restatement (b), the reference's own float64 arithmetic, is at the end of the file.

A read is (nk, qlen, rows), rows = [(column, count)] as K3 left them; the tables: target[column], species[column] (0 = none)."""
import math

UNIT = 720720
EM_UNIT = UNIT << 12
BASE = 65536
MATCH, UNIQ, HIC, BASES_LO, BASES_HI = range(5)
VERDICTS = ("ok", "few-unique", "few-hic-unique", "low-hic-unique-prop", "low-chunks-fraction", "high-depth-stdev")


def qcov(count, nk):
    return float("%.4f" % (float(count) / float(nk)))  # printed_qcov (k3_set_order.hpp): the digits %.4f prints, parsed back


def quota(cov, s):
    x = cov / s * float(EM_UNIT)
    return int(x) if x < float(EM_UNIT) else EM_UNIT


def single_share(m, first):
    return (UNIT - (m - 1) * (UNIT // m) if first else UNIT // m) << 12


def row_share(p, m, first):
    return p - (m - 1) * (p // m) if first else p // m


def kept_rows(nk, rows, target, est, cut=None):
    """a read's rows after the skip of the rows outside the whitelist and THEN the row cuts (refstats_rule.hpp: RefstatsCut; cut =
    dict(top_n, keep_perfect, keep_main, max_gap) or None), as the TSV tool applies them in every pass"""
    kept = [(int(c), int(n)) for c, n in rows if est[int(target[int(c)])]]
    if not cut:
        return kept
    out, prev, n_score, on = [], 1024.0, 0, True
    for i, (c, n) in enumerate(kept):
        q = qcov(n, nk)
        if i == 0:
            prev, n_score, on = 1024.0, 0, True
        elif cut.get("keep_perfect"):
            if not on:
                continue
            if prev == 1 and q < 1:
                on = False
                continue
        elif cut.get("keep_main") and prev <= 1:
            if not on:
                continue
            if prev - q > cut.get("max_gap", 0.4):
                on = False
                continue
        if cut.get("top_n", 0) > 0:
            if not on:
                continue
            if q < prev:
                n_score += 1
                if n_score > cut["top_n"]:
                    on = False
                    continue
        prev = q
        out.append((c, n))
    return out


def read_adds(nk, qlen, rows, target, species, est, cov, H, level_species, cut=None):
    """-> (nt, [(column, [match, uniq, hic, bases_lo, bases_hi])] for every kept row)"""
    kept = kept_rows(nk, rows, target, est, cut)
    by_target = {}
    for i, (c, _) in enumerate(kept):
        by_target.setdefault(int(target[c]), []).append(i)  # (dicts keep insertion order: first-row order)
    nt = len(by_target)
    if nt == 0:
        return 0, []
    p, uniq_first = {}, True
    if nt > 1:
        s = 0.0
        for t in by_target:
            s += float(cov[t])
        room = EM_UNIT
        for t in by_target:
            p[t] = min(quota(float(cov[t]), s), room)
            room -= p[t]
        p[next(iter(by_target))] += room
        sp = {int(species[kept[ix[0]][0]]) if species is not None else 0 for ix in by_target.values()}
        uniq_first = bool(level_species) and len(sp) == 1 and 0 not in sp
    ql = min(max(int(qlen), 0), 0xffffffff)
    out = []
    for t, ix in by_target.items():
        m = len(ix)
        for k, i in enumerate(ix):
            c, n = kept[i]
            share = single_share(m, k == 0) if nt == 1 else row_share(p[t], m, k == 0)
            prod = ql * share
            w = [share, 0, 0, prod & 0xffffffff, prod >> 32]
            if k == 0 and uniq_first:
                w[UNIQ] = EM_UNIT if nt == 1 else share
                if qcov(n, nk) >= H:
                    w[HIC] = w[UNIQ]
            out.append((c, w))
    return nt, out


def pass_cols(reads, n_cols, target, species, est, cov, H, level_species, cut=None):
    """a pass over `reads` -> ([n_cols][5] Python integers, dict of totals)"""
    cnt = [[0] * 5 for _ in range(n_cols)]
    tot = dict(assigned_reads=0, unique_reads=0, split_reads=0)
    for nk, qlen, rows in reads:
        nt, adds = read_adds(nk, qlen, rows, target, species, est, cov, H, level_species, cut)
        for c, w in adds:
            for j in range(5):
                cnt[c][j] += w[j]
        tot["assigned_reads"] += nt >= 1
        tot["unique_reads"] += nt == 1
        tot["split_reads"] += nt > 1
    return cnt, tot


def em_cols(reads, n_cols, target, species, est, cov, H, level_species, cut=None):
    """what kmcpg_em_read returns for `reads` searched with the recount stage on: [n_cols][6] = match, uniq, hic, single_bases, bases_lo,
    bases_hi — reads with ONE target in the whole table are K8's single-target reads (their bases in units of 2^-16 base, apart)"""
    single = [(nk, ql, rows) for nk, ql, rows in reads if len({int(target[int(c)]) for c, _ in rows}) == 1]
    multi = [(nk, ql, rows) for nk, ql, rows in reads if len({int(target[int(c)]) for c, _ in rows}) > 1]
    cnt, tot = pass_cols(multi, n_cols, target, species, est, cov, H, level_species, cut)
    out = [[w[MATCH], w[UNIQ], w[HIC], 0, w[BASES_LO], w[BASES_HI]] for w in cnt]
    for nk, ql, rows in single:
        if not est[int(target[int(rows[0][0])])]:
            continue
        rows = kept_rows(nk, rows, target, est, cut)  # (the cuts can drop later rows of the one target)
        m = len(rows)
        for k, (c, n) in enumerate(rows):
            share = single_share(m, k == 0)
            out[int(c)][0] += share
            out[int(c)][3] += max(int(ql), 0) * BASE // m
            if k == 0:
                out[int(c)][1] += EM_UNIT
                if qcov(n, nk) >= H:
                    out[int(c)][2] += EM_UNIT
        tot["assigned_reads"] += 1
        tot["unique_reads"] += 1
    return out, tot


# ---- the roll-up, the loop and the end -----------------------------------------------------------------------------
def chunk_bases(w):
    """w = [match, uniq, hic, single_bases, bases_lo, bases_hi] -> bases, as em_chunk_bases"""
    return float(w[3]) / float(BASE) + (float(w[5]) * 4294967296.0 + float(w[4])) / float(EM_UNIT)


def stdev(v):
    n = len(v)
    if n < 2:
        return 0.0
    s = 0.0
    for x in v:
        s += x
    mean = s / float(n)
    var = 0.0
    for x in v:
        var += (x - mean) * (x - mean)
    return math.sqrt(var / float(n))


def rollup(chunks, tlen, th, judge):
    """chunks: [[6 words]] of a reference; th: dict(r, u, U, P, p, d, norm) -> dict"""
    o = dict(match=sum(w[0] for w in chunks), uniq=sum(w[1] for w in chunks), hic=sum(w[2] for w in chunks), verdict="ok")
    n = len(chunks)
    covered = sum(1 for w in chunks if w[0] >= th["r"] * EM_UNIT)
    b = [chunk_bases(w) for w in chunks]
    qlens = 0.0
    for x in b:
        qlens += x
    nz = [x for x in b if x != 0]
    o["listed"] = o["match"] > 0
    o["chunks_frac"] = float(covered) / float(n) if n else 0.0
    o["rel_depth"], o["depth_stdev"], o["coverage"] = [0.0] * n, 0.0, 0.0
    if nz:
        o["rel_depth"] = [x / qlens * float(n) for x in b]
        o["depth_stdev"] = stdev(o["rel_depth"])
        top = qlens if th["norm"] == "mean" else (min(nz) if th["norm"] == "min" else max(nz)) * float(n)
        o["coverage"] = top / float(tlen)
    if judge:
        if o["uniq"] < th["u"] * EM_UNIT:
            o["verdict"] = VERDICTS[1]
        elif o["hic"] < th["U"] * EM_UNIT:
            o["verdict"] = VERDICTS[2]
        elif float(o["hic"]) < th["P"] * float(o["uniq"]):
            o["verdict"] = VERDICTS[3]
        elif o["chunks_frac"] < th["p"]:
            o["verdict"] = VERDICTS[4]
        elif o["depth_stdev"] > th["d"]:
            o["verdict"] = VERDICTS[5]
    return o


def run(classes, est, cov, th, do_pass, max_iters=10, pct_threshold=0.01):
    """classes: [dict(columns=[...], tlen=, name=)]; do_pass(est, cov) -> ([n_cols][6], assigned reads).
    -> dict(refs, est, assigned, passes, converged, verdicts0: the verdicts of pass 0)"""
    est, cov = list(est), list(cov)
    n = len(classes)
    res = dict(refs=[None] * n, passes=0, converged=False, assigned=0, verdicts0={})
    before = 0.0
    by_name = sorted(range(n), key=lambda c: (classes[c]["name"], c))  # the order the coverages are added in
    for it in range(max_iters + 1):
        if not any(est):
            break
        cols, res["assigned"] = do_pass(list(est), list(cov))
        res["passes"] += 1
        s = 0.0
        for c in by_name:
            if not est[c]:
                continue
            r = rollup([cols[k] for k in classes[c]["columns"]], classes[c]["tlen"], th, it == 0)
            if it == 0:
                res["verdicts0"][c] = r["verdict"] if r["listed"] else "unlisted"
            if not r["listed"] or r["verdict"] != "ok":
                est[c] = 0
            res["refs"][c] = r
            if est[c]:
                cov[c] = r["coverage"]
                s += r["coverage"]
        left = [c for c in by_name if est[c]]
        top_cov, top_pct = -1.0, 0.0
        for c in left:
            res["refs"][c]["percentage"] = cov[c] / s * 100
            if cov[c] > top_cov:
                top_cov, top_pct = cov[c], res["refs"][c]["percentage"]
        if not left:
            break
        if it > 0 and abs(top_pct - before) < pct_threshold:
            res["converged"] = True
            break
        before = top_pct
    res["est"] = est
    return res


def finish(classes, res, filter_low_pct=0.0):
    """-> the class indexes in table order (percentages renormalised in res where -F drops a tail)"""
    import functools
    refs = res["refs"]

    def less(a, b):
        x, y = refs[a], refs[b]
        if x["coverage"] != y["coverage"]:
            return -1 if x["coverage"] > y["coverage"] else 1
        if x["chunks_frac"] != y["chunks_frac"]:
            return -1 if x["chunks_frac"] > y["chunks_frac"] else 1
        return -1 if classes[a]["name"] < classes[b]["name"] else (1 if classes[a]["name"] > classes[b]["name"] else 0)
    order = sorted((c for c in range(len(classes)) if res["est"][c]), key=functools.cmp_to_key(less))
    if filter_low_pct > 0 and len(order) > 1:
        acc, keep = 0.0, len(order)
        while keep > 0:
            acc += refs[order[keep - 1]]["percentage"]
            if acc > filter_low_pct:
                break
            keep -= 1
        if keep < len(order):
            order = order[:keep]
            s = 0.0
            for c in order:
                s += refs[c]["coverage"]
            for c in order:
                refs[c]["percentage"] = refs[c]["coverage"] / s * 100
    return order


HEADER = "#ref\tpercentage\tcoverage\tchunksFrac\tchunksRelDepth\tchunksRelDepthStd\treads\tureads\thicureads\trefsize\n"


def table(classes, res, order):
    """cli/profile_format.hpp"""
    out = [f"# assigned reads: {res['assigned']}\n", f"# passes: {res['passes']}\n", f"# converged: {'yes' if res['converged'] else 'no'}\n", HEADER]
    for c in order:
        r = res["refs"][c]
        out.append("%s\t%.6f\t%.6f\t%.2f\t%s\t%.2f\t%.0f\t%.0f\t%.0f\t%d\n" % (
            classes[c]["name"], r["percentage"], r["coverage"], r["chunks_frac"], ";".join("%.2f" % x for x in r["rel_depth"]), r["depth_stdev"],
            float(r["match"]) / float(EM_UNIT), float(r["uniq"]) / float(EM_UNIT), float(r["hic"]) / float(EM_UNIT), classes[c]["tlen"]))
    return "".join(out)


# ---- (b) the reference's own arithmetic ---------------------------------------------------------------------------
# A literal float64 restatement of kmcp/cmd/profile.go:1907-2570 and :2786-2853: the same loop with its `continue` paths, dicts keyed by
# target, `prop / floatMsSize`, the LITERAL species rule (the LCA of the targets' TaxIds), the tests gated by `iter == 0`, the whitelist
# rebuilt from the targets that pass, the stop on the change of the predominant target.  Stage 3 (profile2, where the loop starts) comes
# from tests/recount_reference.py.  Go ranges over maps in random order; here dicts keep the order of first insertion.  Departures, both
# ours: the final ties go by name (the reference's quicksort is unstable), and mode 0's order and the score column are not restated.
class _Target:
    def __init__(self, m):
        self.name, self.gsize, n = m["target"], m["gsize"], m["chunks"]
        self.match, self.uniq, self.uniq_hic, self.qlen, self.rel_depth = [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n
        self.sum_uniq = self.sum_hic = self.sum_match = self.frags = self.qlens = self.rel_std = self.coverage = self.percentage = 0.0


def float_profile(texts, start, th, hic_min_qcov=0.75, level="species", taxid_map=None, tax=None, max_fpr=0.01, min_qcov=0.55, top_n=0, keep_perfect=False,
                  keep_main=False, max_gap=0.4, max_iters=10, pct_threshold=0.01, filter_low_pct=0.0):
    """start: name -> coverage of the references stage 3 judged ok (profile2); th: dict(r, u, U, P, p, d, norm).
    -> dict(verdicts0, passes, converged, order, coverage, percentage, assigned, margin: the smallest relative distance of a pass-0 test
    on a summed quantity from its threshold, conv_margin: the smallest distance of a pass's change of the top percentage from the threshold)"""
    from tests import profile_contract as PC
    from tests import recount_reference as R3
    level_species = level.lower() == "species"
    white, cover = set(start), dict(start)
    out = dict(verdicts0={}, passes=0, converged=False, margin=float("inf"), conv_margin=float("inf"))
    targets, dom_pre, assigned = [], 0.0, 0

    def near(a, b):
        out["margin"] = min(out["margin"], abs(a - b) / max(abs(a), abs(b), 1e-300))

    for it in range(max_iters + 1):
        profile3 = {}
        n_assigned = [0]

        def target(h, m):
            t = profile3.get(h)
            if t is None:
                t = profile3[h] = _Target(m)
            return t

        def finish(matches):
            uniq_match = False
            if len(matches) > 1:  # redistribute matches
                n_assigned[0] += 1
                sum_cov = 0.0
                taxids = []
                for h, ms in matches.items():
                    sum_cov += cover[h]
                    if level_species:
                        taxids.append(taxid_map[ms[0]["target"]])
                same_species = False
                if level_species:
                    node = tax.resolve(taxids[0]) if tax.known(taxids[0]) else 0
                    for t2 in taxids[1:]:
                        node = tax.lca(node, t2)
                    same_species = tax.at_or_below_species(node)
                for h, ms in matches.items():
                    size = float(len(ms))
                    first = True
                    prop = cover[h] / sum_cov
                    for m in ms:
                        t = target(h, m)
                        if first:
                            if level_species and same_species:
                                t.uniq[m["chunk_idx"]] += prop / size
                                if m["qcov"] >= hic_min_qcov:
                                    t.uniq_hic[m["chunk_idx"]] += prop / size
                            first = False
                        t.qlen[m["chunk_idx"]] += float(m["qlen"]) * prop / size
                        t.match[m["chunk_idx"]] += prop / size
            elif len(matches) == 1:
                n_assigned[0] += 1
                uniq_match = True
            if uniq_match:
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
                if match["target"] not in white:  # skip matches of unwanted targets
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
        assigned = n_assigned[0]
        out["passes"] += 1

        targets, white = [], set()
        for h, t in profile3.items():
            def fail(v):
                if it == 0:
                    out["verdicts0"][h] = v
            for c in t.uniq:
                t.sum_uniq += c
            if it == 0:
                near(t.sum_uniq, th["u"])
            if it == 0 and t.sum_uniq < th["u"]:
                fail("few-unique")
                continue
            for c in t.uniq_hic:
                t.sum_hic += c
            if it == 0:
                near(t.sum_hic, th["U"])
            if it == 0 and t.sum_hic < th["U"]:
                fail("few-hic-unique")
                continue
            if it == 0:
                near(t.sum_hic, th["P"] * t.sum_uniq)
            if it == 0 and t.sum_hic < th["P"] * t.sum_uniq:
                fail("low-hic-unique-prop")
                continue
            for c in t.match:
                if it == 0:
                    near(c, th["r"])
                if c >= th["r"]:
                    t.frags += 1
                t.sum_match += c
            t.frags = t.frags / float(len(t.match))
            if it == 0 and t.frags < th["p"]:
                fail("low-chunks-fraction")
                continue
            t.qlens = 0.0
            for c in t.qlen:
                t.qlens += c
            for i, c in enumerate(t.qlen):
                t.rel_depth[i] = c / t.qlens * float(len(t.qlen))
            _, t.rel_std = R3.mean_stdev(t.rel_depth)
            if it == 0:
                near(t.rel_std, th["d"])
            if it == 0 and t.rel_std > th["d"]:
                fail("high-depth-stdev")
                continue
            if th["norm"] == "mean":
                t.coverage = t.qlens / float(t.gsize)
            else:
                nz = [c for c in t.qlen if c != 0]
                t.coverage = (min(nz) if th["norm"] == "min" else max(nz)) * float(len(t.qlen)) / float(t.gsize)
            if it == 0:
                out["verdicts0"][h] = "ok"
            targets.append(t)
            cover[h] = t.coverage
            white.add(h)
        sum_cov = 0.0
        for t in targets:
            sum_cov += t.coverage
        for t in targets:
            t.percentage = t.coverage / sum_cov * 100
        targets.sort(key=lambda t: -t.coverage)
        if it > 0 and targets:
            change = abs(targets[0].percentage - dom_pre)
            out["conv_margin"] = min(out["conv_margin"], abs(change - pct_threshold))
            if change < pct_threshold:
                out["converged"] = True
                break
        if not targets:
            break
        dom_pre = targets[0].percentage

    import functools

    def less(a, b):  # Targets.Less, then the name
        if a.coverage != b.coverage:
            return -1 if a.coverage > b.coverage else 1
        if a.frags != b.frags:
            return -1 if a.frags > b.frags else 1
        return -1 if a.name < b.name else (1 if a.name > b.name else 0)
    targets.sort(key=functools.cmp_to_key(less))
    if filter_low_pct > 0 and len(targets) > 1:
        acc, n = 0.0, 0
        for t in reversed(targets):
            acc += t.percentage
            if acc > filter_low_pct:
                break
            n += 1
        if n > 0:
            targets = targets[:len(targets) - n]
            total = 0.0
            for t in targets:
                total += t.coverage
            for t in targets:
                t.percentage = t.coverage / total * 100
    out.update(order=[t.name for t in targets], coverage={t.name: t.coverage for t in targets}, percentage={t.name: t.percentage for t in targets}, assigned=assigned,
               reads={t.name: (t.sum_match, t.sum_uniq, t.sum_hic) for t in targets})
    return out


def float_start(texts, th, hic_min_qcov, level="species", taxid_map=None, tax=None, no_amb_corr=False, min_dreads_prop=0.05, max_mismatch_err=0.05, **cuts):
    """profile2 of tests/recount_reference.py judged with th -> name -> coverage of the references stage 3 says ok"""
    from tests import cooccur_reference as CR
    from tests import recount_reference as R3
    from tests import refstats_reference as RR
    prof, _, _ = RR.stage1(texts, hic_min_qcov=hic_min_qcov, level=level, taxid_map=taxid_map, tax=tax, **cuts)
    kept = {}
    for name, t in prof.items():
        v, reads, ureads, _, _ = RR.verdict(t, th["p"])
        if v == "ok":
            kept[name] = (float(reads), float(ureads))
    amb = CR.stage2(texts, set(kept), **cuts)
    prof2, _, _, _ = R3.stage3(texts, kept, amb, hic_min_qcov=hic_min_qcov, level=level, taxid_map=taxid_map, tax=tax, no_amb_corr=no_amb_corr,
                               min_dreads_prop=min_dreads_prop, max_mismatch_err=max_mismatch_err, **cuts)
    start = {}
    for name, t in prof2.items():
        j = R3.judge(t, th["r"], th["u"], th["U"], th["P"], th["p"], th["d"], norm=th["norm"])
        if j["verdict"] == "ok" and j["coverage"] > 0:
            start[name] = j["coverage"]
    return start
