#!/usr/bin/env python3
"""Does the species-specific stage (K4, kmcpg_set_specific) make the pipelined search of a hit-heavy database faster?

On the real-genome family database of tools/family_db.py a batch returns ~200 matches per read, and the pipelined submit / wait_pairs
path is bound by what crosses PCIe and is expanded on the host, not by the kernels.  With the stage on, only the surviving reads' matches
leave the GPU.  This tool alternates, in one session on one handle, the plain pipelined pairs path and the same path with the stage on
(taxonomy: one species per base genome, the strains alternately in two species of one genus — as tests/test_gpu_specific.py), REPS
times each, and reports the median and the spread of reads/s, K4's HIP-event milliseconds and the pairs that came down.

    python tools/bench_specific.py OUT.json [--ecoli-strains 600] [--small-strains 100] [--batch 131072] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import family_db  # noqa: E402
from kmcp_amd import Database, default_params, lib  # noqa: E402

NB = 8  # batches per timed run, from two host threads with two tickets each (what kmcp-search does)


def pipelined(db, h_reads, h_offs, params):
    pairs = [0] * NB

    def pump(t_):
        tk = []
        for i in range(t_, NB, 2):
            if len(tk) == 2:
                j, t = tk.pop(0)
                pairs[j] = db.wait_pairs(t, count_only=True)
            tk.append((i, db.submit(h_reads, h_offs, params=params)))
        while tk:
            j, t = tk.pop(0)
            pairs[j] = db.wait_pairs(t, count_only=True)
    th = [threading.Thread(target=pump, args=(t_,)) for t_ in range(2)]
    t0 = time.time()
    [x.start() for x in th]
    [x.join() for x in th]
    return (time.time() - t0) / NB, pairs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--ecoli-strains", type=int, default=600)
    ap.add_argument("--small-strains", type=int, default=100)
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    B = a.batch
    cols, reads, info = family_db.generate(a.ecoli_strains, a.small_strains, B, log=lambda m: print(m, file=sys.stderr))
    accs = [x for x, _ in family_db.base_genomes()]
    with tempfile.TemporaryDirectory() as d:
        db_dir = lib.build_db(d, cols, k=family_db.K, threads=32, alias="family-db")
        del cols
        h_reads = np.ascontiguousarray(reads[:B]).reshape(-1)
        h_offs = np.arange(B + 1, dtype=np.uint64) * family_db.READ_LEN
        params = default_params()
        with Database.open(db_dir, device=0) as db:
            n = int(db.info.n_cols)
            names = [db.col_info(c)[0] for c in range(n)]
            ids = {}
            target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
            species = np.array([2000 + 2 * accs.index(x.rsplit(".s", 1)[0]) + int(x.rsplit(".s", 1)[1]) % 2 for x in names], dtype=np.uint32)
            db.set_profiling(1)
            pipelined(db, h_reads, h_offs, params)  # sizes staging and hit buffers
            runs = {"plain": [], "specific": []}
            k4_ms, down = [], {}
            for rep in range(a.reps):
                for mode in ("plain", "specific"):
                    if mode == "specific":
                        db.set_specific(target, species)
                    else:
                        db.set_specific()
                    s_per_batch, pairs = pipelined(db, h_reads, h_offs, params)
                    runs[mode].append(B / s_per_batch)
                    down[mode] = pairs
                    if mode == "specific":
                        st, _ = db.last_specific()
                        k4_ms.append(db.last_k4_ms)
                        witness = st
            db.set_specific()

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)
    out = dict(database=info, batch_reads=B, batches_per_run=NB, reps=a.reps, reads_per_s={m: summary(v) for m, v in runs.items()},
               k4_ms=summary(k4_ms), pairs_down_per_batch=down, witness_last_batch=witness,
               specific_over_plain=statistics.median(runs["specific"]) / statistics.median(runs["plain"]))
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
