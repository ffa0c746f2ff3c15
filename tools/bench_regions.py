#!/usr/bin/env python3
"""Specific regions of a genome: the three-command pipeline against the one-pass command.

On the real-genome family database of tools/family_db.py and one base genome as the query, cut into windows with -s 10 -W 100, this tool
alternates, in one call,

    three   kmcp-search --sliding-step 10 --sliding-window 100 -o w.tsv ; kmcp-filter -f 1 -t 0 --level species -T .. -X .. w.tsv -o f.tsv ;
            kmcp-regions -f 1 -t 0 -l 20 f.tsv -o three.bed
    one     kmcp-search --sliding-step 10 --sliding-window 100 --specific-level species --taxid-map .. --taxdump .. --regions-bed one.bed
            --regions-min-overlap 20

(taxonomy: one species per base genome, its strains alternately in two species of one genus, as tests/test_gpu_specific.py writes it),
both warmed once, REPS times each, wall time from exec to exit.  It checks that the two BED files are equal, and prints both medians with
their spread and — from one in-process run of the library's summary entry on the same windows — kmcpg_last_summary's counters.

To compare against a parent commit, point --search / --filter at that commit's binaries: the pipeline then is the parent's kmcp-search
and kmcp-filter plus this tree's kmcp-regions.

    python tools/bench_regions.py OUT.json [--ecoli-strains 60] [--small-strains 10] [--genome 1] [--reps 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import family_db  # noqa: E402
from kmcp_amd import Database, lib  # noqa: E402

STEP, WINDOW, OVERLAP = 10, 100, 20


def write_taxonomy(d, names, accs):
    os.makedirs(d, exist_ok=True)
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "family")]
    ids = {}
    for gi in range(len(accs)):
        nodes.append((1000 + gi, 10, "genus"))
        nodes += [(2000 + 2 * gi + half, 1000 + gi, "species") for half in range(2)]
    for n in sorted(set(names)):
        acc, s = n.rsplit(".s", 1)
        gi, si = accs.index(acc), int(s)
        ids[n] = 100000 + 100 * gi + si
        nodes.append((ids[n], 2000 + 2 * gi + si % 2, "strain"))
    with open(os.path.join(d, "nodes.dmp"), "w") as fh:
        fh.writelines(f"{t}\t|\t{p}\t|\t{r}\t|\t\t|\n" for t, p, r in nodes)
    with open(os.path.join(d, "map.tsv"), "w") as fh:
        fh.writelines(f"{n}\t{t}\n" for n, t in ids.items())
    return d, os.path.join(d, "map.tsv"), ids


def timed(cmds):
    t0 = time.time()
    for c in cmds:
        r = subprocess.run(c, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("%s\n%s" % (" ".join(c), r.stderr))
    return time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--ecoli-strains", type=int, default=60)
    ap.add_argument("--small-strains", type=int, default=10)
    ap.add_argument("--genome", type=int, default=1, help="index of the base genome used as the query")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--search", default=os.path.join(ROOT, "kmcp_amd", "kmcp-search"), help="kmcp-search of the three-command pipeline")
    ap.add_argument("--filter", default=os.path.join(ROOT, "kmcp_amd", "kmcp-filter"), help="kmcp-filter of the three-command pipeline")
    a = ap.parse_args()
    search_here = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
    regions = os.path.join(ROOT, "kmcp_amd", "kmcp-regions")
    cols, _, info = family_db.generate(a.ecoli_strains, a.small_strains, 1000, log=lambda m: print(m, file=sys.stderr))
    accs = [x for x, _ in family_db.base_genomes()]
    acc, genome = family_db.base_genomes()[a.genome]
    with tempfile.TemporaryDirectory() as d:
        db_dir = lib.build_db(os.path.join(d, "db"), cols, k=family_db.K, threads=16, alias="family-db")
        names = [c[0] for c in cols]
        del cols
        dump, tmap, ids = write_taxonomy(os.path.join(d, "tax"), names, accs)
        fa = os.path.join(d, "q.fa")
        with open(fa, "w") as fh:
            fh.write(">%s\n%s\n" % (acc, bytes(genome).decode()))
        sliding = ["--sliding-step", str(STEP), "--sliding-window", str(WINDOW)]
        root = os.path.dirname(db_dir)
        w, f, three_bed, one_bed = (os.path.join(d, x) for x in ("w.tsv", "f.tsv", "three.bed", "one.bed"))
        three = [[a.search, "-d", root, fa, "-q", "-o", w] + sliding,
                 [a.filter, "-f", "1", "-t", "0", "--level", "species", "-T", tmap, "-X", dump, "-o", f, w],
                 [regions, "-f", "1", "-t", "0", "-l", str(OVERLAP), "-o", three_bed, f]]
        one = [[search_here, "-d", root, fa, "-q", "--specific-level", "species", "--taxid-map", tmap, "--taxdump", dump, "--regions-bed", one_bed,
                "--regions-min-overlap", str(OVERLAP)] + sliding]
        timed(three), timed(one)  # warm: the page cache, the code objects
        runs = {"three": [], "one": []}
        for _ in range(a.reps):
            runs["three"].append(timed(three))
            runs["one"].append(timed(one))
        equal = open(three_bed).read() == open(one_bed).read()
        n_regions = open(one_bed).read().count("\n")
        tsv_bytes = os.path.getsize(w)
        # the library's counters for the same windows, in process
        with Database.open(db_dir, device=0) as db:
            n = int(db.info.n_cols)
            cn = [db.col_info(c)[0] for c in range(n)]
            t_ids = {}
            target = np.array([t_ids.setdefault(x, len(t_ids)) for x in cn], dtype=np.uint32)
            species = np.array([2000 + 2 * accs.index(x.rsplit(".s", 1)[0]) + int(x.rsplit(".s", 1)[1]) % 2 for x in cn], dtype=np.uint32)
            db.set_specific(target, species)
            seqs, offs = lib.pack_reads([bytes(genome)])
            s, _, _ = db.wait_summaries(db.submit_windows_summary(seqs, offs, STEP, WINDOW))
            witness, _ = db.last_summary()

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)
    out = dict(database=info, query=acc, query_bases=len(genome), windows=len(s), step=STEP, window=WINDOW, reps=a.reps, bed_equal=equal,
               regions=n_regions, tsv_bytes=tsv_bytes,
               seconds={m: summary(v) for m, v in runs.items()}, one_over_three=statistics.median(runs["one"]) / statistics.median(runs["three"]),
               last_summary=witness)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit("the two BED files differ")


if __name__ == "__main__":
    main()
