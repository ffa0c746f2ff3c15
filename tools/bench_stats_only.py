#!/usr/bin/env python3
"""What does a statistics-only search (kmcpg_submit_stats / kmcpg_wait_stats, K10) save against the route that brings every pair to the
host (kmcpg_submit / kmcpg_wait_pairs), at the library's boundary?

One handle per shape with K6 + K7 + K8 on (every column a reference of its own), the config1-shaped index of bench.py and two shapes of
tools/bench_cooccur.py's batch: one hit per read ("config1": every fragment planted into one column) and the family shape ("even": every
fragment in F = 57 neighbouring columns, the families anywhere in the index).  Batches of 32 768 reads from host buffers, two threads
with two tickets in flight each — what kmcp-search's searchers do.  The two routes alternate in one process, `--reps` repetitions of
`--batches` batches each; the stages are reset before every repetition (so that K8's log never fills and both routes count the same).
Reported: reads/s (median and range over the repetitions — the range of a route is the noise floor), the bytes that came from the device
per batch (pairs route: 8 per pair and the offsets, qlen, qkmers; statistics route: kmcpg_result_stats.bytes_d2h), the LEFT reads, and
k10_ms: the HIP-event time of K10's kernels for one batch, from a pass of its own at profiling level 1 after the timed window.

    python tools/bench_stats_only.py [--batch 32768] [--relatives 57] [--batches 16] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_cooccur import READ_LEN, SPEC, make_batch  # noqa: E402
from kmcp_amd import Database, default_params, lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--relatives", type=int, default=57)
    ap.add_argument("--batches", type=int, default=16, help="batches per repetition and route, shared by the two threads")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stats_only.py needs a GPU")
    B, dev = a.batch, torch.device("cuda", 0)
    params = default_params()

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v))

    out = dict(workload="config1-shaped: 32 blocks x 312 columns, every column a reference, 150-bp reads, k = 21, -t 0.55; K6 + K7 + K8 on", batch_reads=B,
               batches=a.batches, reps=a.reps, threads=2, tickets_per_thread=2, shapes={})
    for shape, F in (("config1", 1), ("even", a.relatives)):
        db = Database.open_synthetic(lib.SynthSpec(seed=42, **SPEC), device=0)
        n_cols = int(db.info.n_cols)
        target = np.arange(n_cols, dtype=np.uint32)
        reads, offs = make_batch(db, dev, B, n_cols, 3000 + F, F, 0)
        h_reads, h_offs = reads.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)
        db.set_refstats(target, None)
        db.set_cooccur(target)
        db.set_recount(target, None)

        def reset():
            db.refstats_reset()
            db.cooccur_reset()
            db.recount_reset()

        def run(route, n_batches):
            """n_batches batches over two threads with two tickets each; returns (seconds, [per-batch result])"""
            todo, got, lock = [n_batches], [], threading.Lock()

            def take():
                with lock:
                    if todo[0] == 0:
                        return False
                    todo[0] -= 1
                    return True

            def finish(t):
                if route == "stats":
                    r = db.wait_stats(t)
                else:
                    pairs = db.wait_pairs(t, count_only=True)
                    r = dict(bytes_d2h=8 * pairs + B * 16 + 32, kept_pairs=pairs)  # pairs, offsets, qlen, qkmers, the four counter words
                with lock:
                    got.append(r)

            def worker():
                fl = []
                while take():
                    fl.append(db.submit_stats(h_reads, h_offs, params=params) if route == "stats" else db.submit(h_reads, h_offs, params=params))
                    if len(fl) == 2:
                        finish(fl.pop(0))
                for t in fl:
                    finish(t)

            th = [threading.Thread(target=worker) for _ in range(2)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            return time.perf_counter() - t0, got

        routes = ("pairs", "stats")
        state = {}
        for r in routes:  # warm-up (lanes, pinned buffers, the hit-buffer hint), and the counts of one batch: both routes count the same
            reset()
            run(r, 4)
            reset()
            _, one = run(r, 1)
            state[r] = (db.refstats_read(n_cols)[0].tobytes(), db.cooccur_read()[0].tobytes(), one[0])
        assert state["pairs"][:2] == state["stats"][:2], "the two routes counted different things"
        rate, nbytes = {r: [] for r in routes}, {r: [] for r in routes}
        for rep in range(a.reps):  # the routes alternate: a drift of the machine hits both alike
            for r in routes:
                reset()
                sec, got = run(r, a.batches)
                rate[r].append(B * a.batches / sec)
                nbytes[r].append(statistics.median(g["bytes_d2h"] for g in got))
        # K10's own time: one batch in flight at profiling level 1, outside the timed window
        db.set_profiling(1)
        k10 = []
        for _ in range(5):
            reset()
            db.wait_stats(db.submit_stats(h_reads, h_offs, params=params))
            db.last_stats()
            k10.append(db.last_k10_ms)
        db.set_profiling(0)
        st = state["stats"][2]
        d = dict(hits_per_read=st["kept_pairs"] / B, matched_reads=st["matched_reads"], left_reads=st["left_reads"], left_pairs=st["left_pairs"],
                 reads_per_s={r: summary(rate[r]) for r in routes}, bytes_from_device_per_batch={r: summary(nbytes[r]) for r in routes}, k10_ms=summary(k10))
        p, s = d["reads_per_s"]["pairs"], d["reads_per_s"]["stats"]
        d["stats_over_pairs"] = s["median"] / p["median"]
        d["spread_of_pairs"] = (p["max"] - p["min"]) / p["median"]
        d["spread_of_stats"] = (s["max"] - s["min"]) / s["median"]
        out["shapes"][shape] = d
        print(f"{shape}: {d['hits_per_read']:.1f} hits per read, {d['left_reads']} reads ({d['left_pairs']} pairs) left to the host per batch; reads/s pairs route "
              f"{p['median']:.4g} (spread {d['spread_of_pairs']:.3f}), statistics-only {s['median']:.4g} (spread {d['spread_of_stats']:.3f}): {d['stats_over_pairs']:.4f} of the pairs route; "
              f"bytes from the device per batch {d['bytes_from_device_per_batch']['pairs']['median']:.0f} -> {d['bytes_from_device_per_batch']['stats']['median']:.0f}; "
              f"K10 {d['k10_ms']['median']:.3f} ms", flush=True)
        db.close()
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
