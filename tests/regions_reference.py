"""A plain restatement of `kmcp utils merge-regions` (kmcp/cmd/merge-regions.go, row parser util-regions.go), written from reading them:
the yardstick of kmcp-regions (cli/kmcp_regions.cpp) and of the window summaries of K5.  It is literal — one loop over rows, a dict of
the current query's targets, the `begin0 > 0` test, the separate code for the last query — and carries the reference's three quirks
behind switches, each defaulting to what the reference does:

  map_order        the reference adds the targets' qCov in Go map order (random).  None = order of first appearance (a dict keeps it), one
                   of the orders the reference can take; a callable reorders the list of targets (tests show the sum's dependence on it).
  garbage_line     a file with exactly one passing query prints a line of the empty initial region before the real one.
  begin0_is_flag   False = the reference's `begin0 > 0` as "there is a pending region"; True = a proper flag.
"""
import re

DEFAULT_PATTERN = r"^(.+)_sliding:(\d+)\-(\d+)$"


class Fatal(Exception):
    """checkError: the message goes to stderr and the status is 255"""


def go_float(s):
    try:
        if s != s.strip() or s == "":
            raise ValueError
        return float(s)
    except ValueError:
        raise ValueError(s)


def go_atoi(s):
    try:
        return int(s) if re.fullmatch(r"[+-]?[0-9]+", s) else 0
    except ValueError:
        return 0


def parse_row(line, max_fpr, min_qcov, pattern):
    """util-regions.go parseMatchResult3: None for a dropped row, else (query, target, qcov, ref, begin, end)"""
    items = line.split("\t", 12)
    if len(items) < 13:
        raise Fatal("invalid kmcp search result format")
    try:
        fpr = go_float(items[3])
    except ValueError:
        raise Fatal("failed to parse FPR: %s" % items[3])
    if fpr > max_fpr:
        return None
    try:
        qcov = go_float(items[11])
    except ValueError:
        raise Fatal("failed to parse qCov: %s" % items[11])
    if qcov < min_qcov:
        return None
    m = pattern.search(items[0])
    if not m:
        raise Fatal("no reference and location found in the query name")
    return items[0], items[5], qcov, m.group(1), go_atoi(m.group(2)), go_atoi(m.group(3))


def window_summary(rows, map_order=None):
    """rows: (target, qcov) of one query in print order -> (n, score): the first row of every distinct target, added, divided by n if n > 1"""
    matches = {}
    for target, qcov in rows:
        matches.setdefault(target, []).append(qcov)
    targets = list(matches)
    if map_order:
        targets = map_order(targets)
    score = 0.0
    first = True
    for t in targets:
        if first:
            score = matches[t][0]
            first = False
        else:
            score += matches[t][0]
    if len(matches) > 1:
        score /= float(len(matches))
    return len(matches), score


def bed_line(ref, begin, end, name, score):
    return "%s\t%d\t%d\t%s\t%.0f\t.\n" % (ref, begin - 1, end, name, score * 1000)


def merge_file(lines, max_fpr=0.05, min_qcov=0.55, max_gap=0, min_overlap=1, ignore_type=False, regexp=DEFAULT_PATTERN,
               name_species="species-specific", name_assembly="assembly-specific", map_order=None, garbage_line=True, begin0_is_flag=False):
    """one input file's lines (without or with their end of line) -> its BED text"""
    pattern = re.compile(regexp)
    out = []
    matches = []  # the current query's kept rows: (target, qcov); its location is in cur
    cur = None
    prev_query = ""
    ref0, begin0, end0, name0, score0 = "", 0, 0, "", 0.0
    begin1 = end1 = 0
    pending = False
    n_queries = 0

    def summary():
        n, score = window_summary(matches, map_order)
        return cur[0], cur[1], cur[2], (name_assembly if n == 1 else name_species), score

    def extends(ref, begin, name):
        if ref == ref0 and begin + min_overlap - 1 <= end1 and (ignore_type or name == name0):
            return begin - begin1 <= max_gap if max_gap > 0 else True
        return False

    for line in lines:
        line = line.rstrip("\n")
        if line.endswith("\r"):
            line = line[:-1]
        if line == "" or line[0] == "#":
            continue
        m = parse_row(line, max_fpr, min_qcov, pattern)
        if m is None:
            continue
        query, target, qcov, mref, mbegin, mend = m
        if prev_query != query:
            if matches:
                n_queries += 1
                ref, begin, end, name, score = summary()
                if (pending if begin0_is_flag else begin0 > 0):
                    if extends(ref, begin, name):
                        end0 = end
                        if name0 != name:
                            name0 = name_species
                        if name0 == name_species:
                            score0 = (score0 + score) / 2
                    else:
                        out.append(bed_line(ref0, begin0, end0, name0, score0))
                        ref0, begin0, end0, name0, score0 = ref, begin, end, name, score
                else:
                    ref0, begin0, end0, name0, score0 = ref, begin, end, name, score
                    pending = True
                begin1, end1 = begin, end
            matches = []
        if not matches:
            cur = (mref, mbegin, mend)
        matches.append((target, qcov))
        prev_query = query

    if matches:
        n_queries += 1
        ref, begin, end, name, score = summary()
        if extends(ref, begin, name) and (pending or not begin0_is_flag):
            end0 = end
            if name0 != name:
                name0 = name_species
            if name0 == name_species:
                score0 = (score0 + score) / 2
            out.append(bed_line(ref0, begin0, end0, name0, score0))
        else:
            if n_queries > 1 or garbage_line:
                if pending or not begin0_is_flag:
                    out.append(bed_line(ref0, begin0, end0, name0, score0))
            out.append(bed_line(ref, begin, end, name, score))
    return "".join(out)


def merge(files, **kw):
    """several inputs (each a list of lines): the state is reset per file, the outputs are concatenated"""
    return "".join(merge_file(f, **kw) for f in files)
