#!/usr/bin/env python3
"""The same reads against several databases: (a) one kmcp-search run per database, then kmcp-merge — the reference's documented profiling
workflow — against (b) one kmcp-search run with --also-db (kmcpg_open_set: every database resident, the reads parsed once, one hit list
ordered on the GPU in kmcp-merge's order).

Three synthetic databases of BASELINE configs[1]'s shape (bench.py WORKLOADS["config1"], different seeds) are written to a work
directory with kmcpg_save_db; 90 % of the reads are mutated fragments planted into a random column of EACH database (bench.py make_batch), so
a matched read has a row per database and the printed scores tie across members.  Both routes read the same FASTQ and write a TSV; the
two TSVs are compared once (they must be identical).  Per route: wall time (processes started to last process gone, best of --repeats
after one untimed run) and search-phase time (kmcp-search's own "elapsed - before the search started", summed over the runs of (a), plus
kmcp-merge's wall time).  --search-bin / --merge-bin name other binaries for route (a), e.g. a build of the parent commit.

  python tools/bench_multidb.py --reads 2000000 --out profiles/multidb.json
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_search(cli, args, env):
    t0 = time.perf_counter()
    r = subprocess.run([cli] + args, capture_output=True, text=True, env=env, timeout=1800)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(" ".join([cli] + args) + " failed: " + r.stderr[-2000:])
    before = re.search(r"([\d.]+) s before the search started", r.stderr)
    elapsed = re.search(r"elapsed time: ([\d.]+)s", r.stderr)
    phase = float(elapsed.group(1)) - float(before.group(1)) if before and elapsed else None
    return wall, phase


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--search-bin", default=os.path.join(ROOT, "kmcp_amd", "kmcp-search"), help="kmcp-search of route (a)")
    ap.add_argument("--merge-bin", default=os.path.join(ROOT, "kmcp_amd", "kmcp-merge"), help="kmcp-merge of route (a)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    from kmcp_amd import Database, lib

    cli = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
    wl = dict(bench.WORKLOADS["config1"])
    L = bench.READ_LEN
    work = bench._pick_workdir(args.reads * (16 + 2 * L + 140) * 3 + 8.0e9)
    if work is None:
        raise SystemExit("no work directory with enough room")
    dev = torch.device("cuda:0")
    rec = {"reads": args.reads, "databases": 3, "route_a_search_bin": args.search_bin, "route_a_merge_bin": args.merge_bin}
    try:
        dbs = []
        for m in range(3):
            spec = lib.SynthSpec(k=wl["k"], num_hashes=wl["num_hashes"], fpr=wl["fpr"], n_blocks=wl["n_blocks"], cols_per_block=wl["cols_per_block"],
                                 num_sigs=wl["num_sigs"], kmers_per_col=wl["kmers_per_col"], seed=42 + m, sigs_step=wl.get("sigs_step", 0))
            dbs.append(Database.open_synthetic(spec, device=0))
        n_cols = int(dbs[0].info.n_cols)

        def plant(frag, offs, n, total, maxlen, cols):  # the fragment into the same column number of every database
            for db in dbs:
                db.plant_reads_device(frag.data_ptr(), offs.data_ptr(), n, total, maxlen, cols.data_ptr())

        fq = os.path.join(work, "reads.fq")
        done = 0
        while done < args.reads:
            nb = min(1 << 20, args.reads - done)
            bt = bench.make_batch(dev, wl, nb, n_cols, 9000 + done // (1 << 20), plant)
            bench._write_fastq(fq, bt.reads.cpu().numpy().reshape(nb, L), done)
            done += nb
            del bt
        torch.cuda.synchronize()
        roots = []
        for m, db in enumerate(dbs):
            roots.append(os.path.join(work, f"db{m}"))
            db.save(roots[-1])
            db.close()
        torch.cuda.empty_cache()

        env = dict(os.environ)
        singles = [os.path.join(work, f"single{m}.tsv") for m in range(3)]
        merged, together = os.path.join(work, "merged.tsv"), os.path.join(work, "together.tsv")

        def route_a():
            for f in singles + [merged]:
                if os.path.exists(f):
                    os.unlink(f)
            t0 = time.perf_counter()
            phase = 0.0
            for m in range(3):
                _, ph = run_search(args.search_bin, ["-d", roots[m], fq, "-o", singles[m]], env)
                phase = phase + ph if ph is not None and phase is not None else None
            t1 = time.perf_counter()
            r = subprocess.run([args.merge_bin, "-o", merged] + singles, capture_output=True, text=True, timeout=1800)
            if r.returncode != 0:
                raise RuntimeError("kmcp-merge failed: " + r.stderr[-2000:])
            t2 = time.perf_counter()
            return dict(wall_s=t2 - t0, search_phase_s=(phase + (t2 - t1)) if phase is not None else None, merge_s=t2 - t1)

        def route_b():
            if os.path.exists(together):
                os.unlink(together)
            wall, phase = run_search(cli, ["-d", roots[0], "--also-db", roots[1], "--also-db", roots[2], fq, "-o", together], env)
            return dict(wall_s=wall, search_phase_s=phase)

        route_a(), route_b()  # untimed: first touch of the binaries, the files and the driver
        with open(merged, "rb") as f1, open(together, "rb") as f2:
            same = f1.read() == f2.read()
        rec["outputs_identical"] = same
        rec["rows"] = sum(1 for line in open(together, "rb") if not line.startswith(b"#"))
        a_runs, b_runs = [], []
        for _ in range(args.repeats):  # alternating
            a_runs.append(route_a())
            b_runs.append(route_b())
        a, b = min(a_runs, key=lambda x: x["wall_s"]), min(b_runs, key=lambda x: x["wall_s"])
        rec.update({"a_three_runs_plus_merge": a, "b_one_run_also_db": b, "a_wall_all": [x["wall_s"] for x in a_runs], "b_wall_all": [x["wall_s"] for x in b_runs],
                    "wall_ratio_a_over_b": a["wall_s"] / b["wall_s"],
                    "search_phase_ratio_a_over_b": (a["search_phase_s"] / b["search_phase_s"]) if a["search_phase_s"] and b["search_phase_s"] else None})
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if not rec.get("outputs_identical", False):
        raise SystemExit("the two routes wrote different TSVs")


if __name__ == "__main__":
    main()
