#!/usr/bin/env python
"""Rate of index inspection (kmcpg_col_ones, kmcpg_block_density) against a read-only streaming pass over the same rows.

    python tools/bench_density.py [--workload gtdb|config1_ungrouped|small] [--reps 5] [--out FILE.json]

gtdb: the GTDB-scale synthetic index of bench.py (32 blocks x 14 976 columns x ~968 700 rows, 58 GB).  config1_ungrouped: the
39-byte-row layout of BASELINE configs[1] with every block on its own (KMCPG_FUSE=0) — bound by request rate, as the COBS kernel is
there.  For each it reports, after a warm-up, the HIP-event time of the device work of
  * col_ones over the whole index,
  * block_density with 1024 bins per block, block by block (summed),
  * kmcpg_stream_probe: every resident group's rows read once, 16 B per lane, one XOR per load — the yardstick,
each as milliseconds and as bytes of resident rows / time, and the ratio of the density rates to the yardstick's with the
yardstick's own run-to-run spread beside it.  The CPU figure is numpy (np.unpackbits + sum on a row range of one block), labelled as
such: it is not the reference, whose Go binary this project cannot build.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kmcp_amd import lib  # noqa: E402

WORKLOADS = {
    # bench.py's "gtdb" index
    "gtdb": dict(k=21, num_hashes=1, fpr=0.3, n_blocks=32, cols_per_block=14976, num_sigs=967708, sigs_step=64, kmers_per_col=345510, seed=1),
    # BASELINE configs[1]: 10 k chunks in blocks of 312 columns (39-byte rows)
    "config1_ungrouped": dict(k=21, num_hashes=1, fpr=0.3, n_blocks=32, cols_per_block=312, num_sigs=1100000, sigs_step=0, kmers_per_col=392000, seed=2),
    "small": dict(k=21, num_hashes=1, fpr=0.3, n_blocks=4, cols_per_block=14976, num_sigs=120000, sigs_step=64, kmers_per_col=42000, seed=3),
}


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gtdb", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    w = dict(WORKLOADS[args.workload])
    if args.workload == "config1_ungrouped":
        os.environ["KMCPG_FUSE"] = "0"
    spec = lib.SynthSpec(k=w["k"], num_hashes=w["num_hashes"], fpr=w["fpr"], n_blocks=w["n_blocks"], cols_per_block=w["cols_per_block"],
                         num_sigs=w["num_sigs"], kmers_per_col=w["kmers_per_col"], seed=w["seed"], scale=0, syncmer_s=0, minimizer_w=0,
                         sigs_step=w["sigs_step"])
    out = dict(workload=args.workload, spec=w, bins=args.bins)
    with lib.Database.open_synthetic(spec, device=args.device) as db:
        nb = db.info.n_blocks
        infos = [db.block_info(b) for b in range(nb)]
        # yardstick first and last: its spread brackets the density runs
        db.stream_probe()
        probe = []
        for _ in range(args.reps):
            ms, nbytes = db.stream_probe()
            probe.append(ms)
        out["resident_row_bytes"] = nbytes
        db.col_ones()
        ones_ms = []
        for _ in range(args.reps):
            db.col_ones()
            ones_ms.append(db.last_density_ms())
        out["col_ones_launch"] = db.last_density_launch()
        dens_ms = []
        for rep in range(args.reps + 1):
            t = 0.0
            for b in range(nb):
                db.block_density(b, max(1, infos[b]["num_sigs"] // args.bins))
                t += db.last_density_ms()
            if rep:
                dens_ms.append(t)
        out["block_density_launch"] = db.last_density_launch()
        for _ in range(args.reps):
            ms, _ = db.stream_probe()
            probe.append(ms)
        # numpy on the host: rows of one block, read back first (not timed)
        n_rows = min(infos[0]["num_sigs"], max(1024, (256 << 20) // infos[0]["row_bytes"]))
        rows = np.zeros((n_rows, infos[0]["row_bytes"]), dtype=np.uint8)
        db.read_row_range(0, 0, rows)
        t0 = time.perf_counter()
        cpu = np.unpackbits(rows, axis=1)[:, :infos[0]["n_cols"]].sum(axis=0, dtype=np.uint64)
        cpu_s = time.perf_counter() - t0
        gpu = db.block_density(0, n_rows, 0, n_rows)[:, 0]
        out["numpy_matches_gpu"] = bool(np.array_equal(cpu, gpu))
        out["numpy_unpackbits_sum"] = dict(rows=n_rows, bytes=int(rows.nbytes), seconds=cpu_s, GBps=rows.nbytes / cpu_s / 1e9,
                                           note="numpy on one host thread, not the reference")

    def rate(ms):
        return nbytes / (ms * 1e-3) / 1e12

    ps, os_, ds = stats(probe), stats(ones_ms), stats(dens_ms)
    out["stream_probe"] = dict(ms=ps, TBps=rate(ps["median"]), spread=(ps["max"] - ps["min"]) / ps["median"])
    out["col_ones"] = dict(ms=os_, TBps=rate(os_["median"]), over_stream=ps["median"] / os_["median"])
    out["block_density_1024"] = dict(ms=ds, TBps=rate(ds["median"]), over_stream=ps["median"] / ds["median"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
