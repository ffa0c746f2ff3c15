"""The crafted taxonomy and result rows of the filter tests (tests/test_filter_cpu.py; tests/specific_rule_check.cpp carries the same
tree).  25 nodes: two genera with species, strains and sub-strain nodes, a species group, a genus whose only child has no species
above it, a second family; one merged TaxId, one deleted one, and 777, which no file knows."""
import os

# taxid, parent, rank
NODES = [
    (1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "phylum"), (20, 10, "class"), (30, 20, "order"), (40, 30, "family"),
    (100, 40, "genus"), (110, 100, "species"), (111, 110, "strain"), (112, 110, "strain"), (113, 111, "no rank"),
    (120, 100, "species"), (121, 120, "strain"),
    (500, 100, "species group"), (510, 500, "species"), (511, 510, "strain"),
    (200, 40, "genus"), (210, 200, "species"), (211, 210, "subspecies"), (212, 211, "strain"),
    (300, 40, "genus"), (301, 300, "no rank"),
    (50, 30, "family"), (400, 50, "genus"), (410, 400, "species"),
]
MERGED = [(999, 111)]
DELETED = [888]
ABSENT = 777

# reference ID -> TaxId
TAXIDS = {
    "a1": 111, "a2": 112, "a3": 113, "aS": 110,       # strains of species 110, a node below a strain, the species itself
    "b1": 121,                                       # species 120, same genus
    "g1": 511,                                       # species 510 under a species group of the genus
    "c1": 212, "c2": 211,                            # species 210, another genus
    "x1": 100, "x2": 100, "x3": 301,                 # above species: the genus itself (twice), a no-rank node with no species above
    "m1": 999,                                       # merged into 111
    "d1": 888, "d2": 888,                            # deleted
    "n1": 777,                                       # in no file
    "f1": 410,                                       # another family
}


def write_taxdump(d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as fh:
        for t, p, r in NODES:
            fh.write(f"{t}\t|\t{p}\t|\t{r}\t|\tXX\t|\t0\t|\t1\t|\t11\t|\t1\t|\t0\t|\t1\t|\t1\t|\t0\t|\t\t|\n")
    with open(os.path.join(d, "merged.dmp"), "w") as fh:
        for a, b in MERGED:
            fh.write(f"{a}\t|\t{b}\t|\n")
    with open(os.path.join(d, "delnodes.dmp"), "w") as fh:
        for a in DELETED:
            fh.write(f"{a}\t|\n")
    return str(d)


def write_map(path, ids=None):
    with open(path, "w") as fh:
        for k, v in (TAXIDS if ids is None else ids).items():
            fh.write(f"{k}\t{v}\n")
    return str(path)


def row(query, target, fpr="1.0000e-03", qcov="0.8000", chunk=0, chunks=1, qidx=0, end="\n"):
    return "\t".join([query, "150", "130", fpr, "1", target, str(chunk), str(chunks), "30000", "21", "104", qcov, "0.0100", "0.0100", str(qidx)]) + end
