#!/usr/bin/env python3
"""Sliding windows of long queries: the window entry (kmcpg_submit_windows — the reads' bases uploaded once, windows read in place on the
device) against the same windows cut into text on the host and sent through kmcpg_submit, on the three shapes the reference's own
documentation and benchmarks use:
  contigs  -s 100  -W 300       over 4-Mbp contigs        (kmcp search --help, "Attentions" 3)
  hifi     -s 1000 -W 212 -g    over ~10-kb reads         (benchmarks/mock-hifi-zymo)
  genome   -s 4    -W 150       over one genome           (benchmarks/searching)
Per shape: windows/s of both library routes (submit + wait_pairs; the host cut of the text route is timed apart), K1 / K2 ms of the last
kernel call of each route, and the wall time of kmcp-search on the records (--sliding-*) against kmcp-search on a FASTA of the windows.

usage: bench_sliding.py OUT.json [--reps 3]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from kmcp_amd import Database, default_params, lib  # noqa: E402
from tests import synth  # noqa: E402

CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")


def windows_text(reads, S, W, g):
    out = []
    for r in reads:
        L = len(r)
        i = 0
        while True:
            e = i + W
            if e > L:
                if not g or i >= L:
                    break
                e = L
            out.append(r[i:e])
            i += S
    return out


def contigs_from(genomes, n, length, seed):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):  # half from the database's genomes (hits), half random sequence
        parts, have = [], 0
        while have < length:
            if rng.random() < 0.5:
                g = genomes[int(rng.integers(0, len(genomes)))]
                p = int(rng.integers(0, len(g) - 20000))
                parts.append(g[p:p + 20000])
            else:
                parts.append(bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20000)]))
            have += 20000
        out.append(b"".join(parts)[:length])
    return out


def timed(fn, reps):
    fn()  # warm-up: workspaces, lanes, pinned buffers
    t0 = time.perf_counter()
    for _ in range(reps):
        m = fn()
    return (time.perf_counter() - t0) / reps, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="one shape by name (counter runs)")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--level", type=int, default=1, help="2: also the bytes the COBS kernels requested (kmcpg_last_gathered_bytes)")
    a = ap.parse_args()
    genomes = synth.random_genomes(16, 250000, seed=3)
    tmp = tempfile.mkdtemp(prefix="bench_sliding_")
    db_dir = synth.make_db(os.path.join(tmp, "db"), genomes, k=21, n_chunks=4, overlap=150, threads=4)
    shapes = {
        "contigs_s100_W300": (contigs_from(genomes, 4, 4_000_000, 1), 100, 300, False),
        "hifi_s1000_W212_g": (synth.sample_reads(genomes, 2000, 10000, sub_rate=0.002, seed=2, frac_random=0.1), 1000, 212, True),
        "genome_s4_W150": (contigs_from(genomes, 1, 1_000_000, 4), 4, 150, False),
    }
    if a.only:
        shapes = {a.only: shapes[a.only]}
    params = default_params()
    out = {"database": {"genomes": len(genomes), "genome_len": len(genomes[0]), "k": 21, "chunks": 4}, "shapes": {}}
    with Database.open(db_dir) as db:
        db.set_profiling(a.level)
        for name, (reads, S, W, g) in shapes.items():
            seqs, offs = lib.pack_reads(reads)
            n_win, win_bases = lib.window_count(offs, S, W, g)
            t0 = time.perf_counter()
            wins = windows_text(reads, S, W, g)
            ws, wo = lib.pack_reads(wins)
            cut_s = time.perf_counter() - t0
            assert len(wins) == n_win
            dt_w, m_w = timed(lambda: db.wait_pairs(db.submit_windows(seqs, offs, S, W, g, params), count_only=True), a.reps)
            k1_w, k2_w = db.last_timing()
            req_w = (db.last_gathered_bytes() + db.last_hash_bytes()) if a.level >= 2 else None
            dt_t, m_t = timed(lambda: db.wait_pairs(db.submit(ws, wo, params=params), count_only=True), a.reps)
            k1_t, k2_t = db.last_timing()
            req_t = (db.last_gathered_bytes() + db.last_hash_bytes()) if a.level >= 2 else None
            assert m_w == m_t, (name, m_w, m_t)
            out["shapes"][name] = dict(
                reads=len(reads), read_bases=int(offs[-1]), windows=n_win, window_bases=win_bases, matches=m_w,
                window_entry=dict(s=dt_w, windows_per_s=n_win / dt_w, last_k1_ms=k1_w, last_k2_ms=k2_w),
                materialized=dict(s=dt_t, windows_per_s=n_win / dt_t, upload_bytes=int(wo[-1]), host_cut_s=cut_s, last_k1_ms=k1_t, last_k2_ms=k2_t),
                speedup=dt_t / dt_w, last_k2_requested_bytes=dict(window_entry=req_w, materialized=req_t))
            print(name, json.dumps(out["shapes"][name]), file=sys.stderr)
    # the CLI, both routes (records + --sliding-*, and a FASTA of the windows), output to /dev/null
    for name, (reads, S, W, g) in ({} if a.no_cli else shapes).items():
        rec = os.path.join(tmp, "rec.fa")
        win = os.path.join(tmp, "win.fa")
        with open(rec, "w") as fh:
            for i, r in enumerate(reads):
                fh.write(f">r{i}\n{r.decode()}\n")
        with open(win, "w") as fh:
            for i, r in enumerate(reads):
                L, j = len(r), 0
                while True:
                    e = j + W
                    if e > L:
                        if not g or j >= L:
                            break
                        e = L
                    fh.write(f">r{i}_sliding:{j + 1}-{e}\n{r[j:e].decode()}\n")
                    j += S
        flags = ["--sliding-step", str(S), "--sliding-window", str(W)] + (["--sliding-greedy"] if g else [])
        walls = {}
        for route, args in (("sliding", flags + [rec]), ("window_fasta", [win])):
            t0 = time.perf_counter()
            r = subprocess.run([CLI, "-d", os.path.dirname(db_dir), "-o", "/dev/null"] + args, check=True, timeout=600, capture_output=True, text=True)
            walls[route] = time.perf_counter() - t0
            # the CLI's own per-stage account (reader, library, formatter, time before the search started)
            walls[route + "_stages"] = [ln.split("] ", 1)[-1] for ln in r.stderr.splitlines()
                                        if any(x in ln for x in ("done searching", "writer loop", "elapsed time", "processed queries:"))]
        out["shapes"][name]["cli_wall_s"] = walls
        out["shapes"][name]["cli_window_fasta_bytes"] = os.path.getsize(win)
        print(name, "cli", walls, file=sys.stderr)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
