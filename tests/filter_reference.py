"""A plain Python restatement of `kmcp utils filter` (kmcp/cmd/filter.go:253-392, row parser util-filter.go:46-82) for the tests.

It follows the LITERAL rule — the LCA of a query's TaxIds found by walking parents, then "is the LCA at or below rank species" —
and not the class shortcut of kmcp_amd/csrc/specific_rule.hpp, so that the two can be held against each other.  Kept rows are
emitted in input order (the reference walks a Go map: its order among targets is random).  A TaxId that is deleted or absent
has no LCA with anything (0) and is under no species."""
import gzip
import os

HEADER = "#query\tqLen\tqKmers\tFPR\thits\ttarget\tchunkIdx\tchunks\ttLen\tkSize\tmKmers\tqCov\ttCov\tjacc\tqueryIdx\n"


class FilterError(Exception):
    """what the reference reports through checkError (exit status 255)"""


class Taxonomy:
    def __init__(self, taxdump):
        self.parent, self.rank, self.merged, self.deleted = {}, {}, {}, set()
        for line in open(os.path.join(taxdump, "nodes.dmp")):
            f = [x.strip() for x in line.split("|")]
            if len(f) >= 3 and f[0]:
                self.parent[int(f[0])] = int(f[1])
                self.rank[int(f[0])] = f[2]
        p = os.path.join(taxdump, "merged.dmp")
        if os.path.exists(p):
            for line in open(p):
                f = [x.strip() for x in line.split("|")]
                if len(f) >= 2 and f[0]:
                    self.merged[int(f[0])] = int(f[1])
        p = os.path.join(taxdump, "delnodes.dmp")
        if os.path.exists(p):
            for line in open(p):
                f = [x.strip() for x in line.split("|")]
                if f and f[0]:
                    self.deleted.add(int(f[0]))

    def resolve(self, t):
        hops = 0
        while t in self.merged and self.merged[t] != t and hops < 64:
            t = self.merged[t]
            hops += 1
        return t

    def known(self, t):
        t = self.resolve(t)
        return t in self.parent and t not in self.deleted

    def lineage(self, t):
        """t, its parent, ... the root; [] for an unknown TaxId"""
        t = self.resolve(t)
        if not self.known(t):
            return []
        out = [t]
        while self.parent[t] != t and self.parent[t] in self.parent and len(out) <= len(self.parent):
            t = self.parent[t]
            out.append(t)
        return out

    def lca(self, a, b):
        if a == 0 or b == 0:
            return 0
        la, lb = self.lineage(a), self.lineage(b)
        if not la or not lb:
            return 0
        sa = set(la)
        for t in lb:
            if t in sa:
                return t
        return 0

    def at_or_below_species(self, t):
        return any(self.rank[x] == "species" for x in self.lineage(t)) if t else False


def read_taxid_maps(paths):
    m = {}
    for p in paths:
        for line in open(p):
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 2 or not line.strip():
                continue
            if not f[1].isdigit() or not f[1].isascii() or int(f[1]) > 0xFFFFFFFF:
                raise FilterError(f"invalid TaxId: {f[1]}")
            m[f[0]] = int(f[1])
    return m


def lines_of(path):
    """the lines of a plain or gzip file with their line ends"""
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    return data.decode().splitlines(keepends=True)


def judge(targets, level_species, taxid_map, tax):
    """targets: the distinct targets of a query in first-seen order -> keep?"""
    specific = False
    if level_species:
        taxids = []
        for t in targets:
            if t not in taxid_map:
                raise FilterError(f"unknown taxid for {t}, please check taxid mapping file(s)")
            taxids.append(taxid_map[t])
        node = tax.resolve(taxids[0]) if tax.known(taxids[0]) else 0
        for t in taxids[1:]:
            node = tax.lca(node, t)
        specific = tax.at_or_below_species(node)
    return len(targets) == 1 or specific


def filter_files(files_lines, max_fpr=0.05, min_qcov=0.55, level="species", taxid_map=None, tax=None, header=True, verdicts=None):
    """files_lines: per input file its lines (with line ends) -> the output text.  verdicts (a list) receives (query, n distinct targets,
    kept) per judged query."""
    level_species = level.lower() == "species"
    out = [HEADER] if header else []
    for lines in files_lines:
        prev, rows, targets = None, [], []

        def flush():
            if rows:
                keep = judge(targets, level_species, taxid_map, tax)
                if verdicts is not None:
                    verdicts.append((prev, len(targets), keep))
                if keep:
                    out.extend(rows)

        for line in lines:
            body = line.rstrip("\r\n")
            if body == "" or body[0] == "#":
                continue
            f = body.split("\t", 12)
            if len(f) < 13:
                raise FilterError("invalid kmcp search result format")
            try:
                fpr = float(f[3])
            except ValueError:
                raise FilterError(f"failed to parse FPR: {f[3]}")
            if fpr > max_fpr:
                continue
            try:
                qcov = float(f[11])
            except ValueError:
                raise FilterError(f"failed to parse qCov: {f[11]}")
            if qcov < min_qcov:
                continue
            if not rows or f[0] != prev:
                flush()
                prev, rows, targets = f[0], [], []
            if f[5] not in targets:
                targets.append(f[5])
            rows.append(line)
        flush()
    return "".join(out)
