#!/usr/bin/env python3
"""What does the recount with ambiguity correction (K8, kmcpg_set_recount) cost on a hit-heavy batch — the log kernel behind K3 during the
search, the replay after it — and does the workgroups' LDS table do its job?

The workload of tools/bench_cooccur.py: the config1-shaped index of bench.py (10 k columns, 150-bp reads, k = 21), every column a
reference of its own, every planted fragment in F = 57 neighbouring columns, so a read names ~57 targets: the replay's elimination has
up to 56 live rows and ~1 600 pair lookups per read.  Two samples:
    even    the reads' families lie anywhere in the index
    sample  the reads come from 24 families only, as a metagenome's do: the adds fall on a few hundred columns
Stage 1's sums are taken from the batch itself (reads per target; unique reads drawn with a heavy tail, so that the correction bites), the
pair list from K7 on the same batch.  Measured from HBM, the forms alternated in one process: reads resident on the device, K1 + K2
(kmcpg_query_device), K3 (kmcpg_group_device) and, with the stage on, k8_log (kmcpg_recount_log_device) behind it on one stream — stage
off, on, on with KMCPG_RECOUNT_SLOTS=0 (no LDS table).  Reads/s of whole steps (host clock around a synchronised step; a repetition is the
median of its steps; median and range over the repetitions — the range of "off" is the noise floor), HIP-event milliseconds of K3 and
k8_log for the same batch, and of k8_replay over that batch's log (kmcpg_recount_run, with and without the LDS table), with the witness
of both kernels.  The replay is checked before anything is timed: two runs give the same bytes, and every logged read is replayed.

    python tools/bench_recount.py [--batch 32768] [--relatives 57] [--steps 5] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_cooccur import FAMILIES, READ_LEN, SPEC, make_batch  # noqa: E402
from kmcp_amd import Database, default_params, lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--relatives", type=int, default=57)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recount.py needs a GPU")
    B, F, dev = a.batch, a.relatives, torch.device("cuda", 0)
    params = default_params()
    cap = (F + 8) * B + 4096
    d_hits = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    d_qk, d_ql = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    d_pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    d_roffs = torch.zeros(B + 2, dtype=torch.int64, device=dev)
    d_left = torch.zeros(B, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v))

    out = dict(workload=f"config1-shaped: 32 blocks x 312 columns, every column a reference, 150-bp reads, k = 21, -t 0.55; every fragment in {F} neighbouring columns",
               batch_reads=B, relatives=F, steps=a.steps, reps=a.reps, samples={})
    for sample in ("even", "sample"):
        db = Database.open_synthetic(lib.SynthSpec(seed=42, **SPEC), device=0)  # (a fresh index: the plantings of the other sample are gone)
        n_cols = int(db.info.n_cols)
        target = np.arange(n_cols, dtype=np.uint32)
        db.set_profiling(1)
        reads, offs = make_batch(db, dev, B, n_cols, 2000 + (sample == "sample"), F, FAMILIES if sample == "sample" else 0)

        def set_stage(form):
            os.environ.pop("KMCPG_RECOUNT_SLOTS", None)
            if form == "off":
                db.set_recount()
                return
            if form == "on, no LDS table":
                os.environ["KMCPG_RECOUNT_SLOTS"] = "0"
            db.set_recount(target, None, hic_min_qcov=0.75, log_bytes=1 << 30)  # (set anew for every form: an empty log)
            os.environ.pop("KMCPG_RECOUNT_SLOTS", None)

        def step(on, cooccur=False):
            """one batch from HBM; returns (seconds, K3 ms, k8_log ms)"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            db.query_device(reads.data_ptr(), offs.data_ptr(), B, B * READ_LEN, READ_LEN, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_qk.data_ptr(), d_ql.data_ptr(),
                            params=params, stream=st.cuda_stream)
            ev[0].record(st)
            db.group_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_qk.data_ptr(), B, d_pairs.data_ptr(), d_roffs.data_ptr(), params=params, stream=st.cuda_stream)
            ev[1].record(st)
            if cooccur:
                db.cooccur_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), B, 512, d_left.data_ptr(), d_n_hits=d_cnt.data_ptr(), hit_cap=cap, stream=st.cuda_stream)
            if on:
                db.recount_log_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), d_ql.data_ptr(), B, 512, d_left.data_ptr(), d_n_hits=d_cnt.data_ptr(),
                                      hit_cap=cap, stream=st.cuda_stream)
            ev[2].record(st)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]) if on else 0.0

        # stages 1 and 2 of this batch: K7's pair list, the reads per target, unique reads with a heavy tail
        db.set_cooccur(target)
        step(False, cooccur=True)
        pairs_tab, _ = db.cooccur_read()
        db.set_cooccur()
        roffs = d_roffs.cpu().numpy()
        cols = d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2)[:int(roffs[B]), 0]
        rng = np.random.default_rng(7)
        classes = np.zeros(n_cols, dtype=lib.RECOUNT_CLASS_DTYPE)
        classes["reads"] = np.bincount(cols, minlength=n_cols)
        classes["ureads"] = (classes["reads"] * rng.choice([0.0, 0.001, 0.01, 0.1, 0.9], size=n_cols)).astype(np.uint64)
        classes["kept"] = (classes["reads"] > 0) & (rng.random(n_cols) < 0.9)
        forms = ("off", "on", "on, no LDS table")
        for f in forms:  # warm-up: every shape the timed window uses
            set_stage(f)
            step(f != "off")
        # the replay itself, before anything is timed: every logged read is replayed, and a second run gives the same bytes
        set_stage("on")
        step(True)
        db.recount_run(classes, pairs_tab)
        first, tot = db.recount_read()
        db.recount_run(classes, pairs_tab)
        again, tot2 = db.recount_read()
        wit, _ = db.last_recount()
        assert wit["skipped"] == 0 and wit["bad_segments"] == 0 and wit["left_full"] == 0, wit
        assert first.tobytes() == again.tobytes() and tot == tot2 and wit["replay_reads"] == tot["logged_reads"] == wit["logged"] > 0, (tot, wit)
        rate, k3, k8, replay, witness = {f: [] for f in forms}, {f: [] for f in forms}, {f: [] for f in forms}, {f: [] for f in forms[1:]}, {}
        for rep in range(a.reps):  # the forms alternate: a drift of the machine hits all of them alike
            for f in forms:
                set_stage(f)
                got = [step(f != "off") for _ in range(a.steps)]
                rate[f].append(B / statistics.median(g_[0] for g_ in got))
                k3[f].append(statistics.median(g_[1] for g_ in got))
                k8[f].append(statistics.median(g_[2] for g_ in got))
                if f == "off":
                    continue
                set_stage(f)  # the replay of ONE batch's log
                step(True)
                ms = []
                for _ in range(a.steps):
                    db.recount_run(classes, pairs_tab)
                    witness[f] = db.last_recount()[0]
                    ms.append(db.last_k8_replay_ms)
                replay[f].append(statistics.median(ms))
        set_stage("off")
        d = dict(pairs_per_batch=int(roffs[B]), hits_per_read=float(roffs[B]) / B, stage2_pairs=int(len(pairs_tab)), totals=tot,
                 device_reads_per_s={f: summary(rate[f]) for f in forms}, k3_ms={f: summary(k3[f]) for f in forms},
                 k8_log_ms={f: summary(k8[f]) for f in forms[1:]}, k8_replay_ms={f: summary(replay[f]) for f in forms[1:]}, witness=witness)
        off, on = d["device_reads_per_s"]["off"], d["device_reads_per_s"]["on"]
        d["device_on_over_off"] = on["median"] / off["median"]
        d["device_spread_of_off"] = (off["max"] - off["min"]) / off["median"]
        out["samples"][sample] = d
        w = witness["on"]
        print(f"{sample}: {d['hits_per_read']:.1f} hits per read, {tot['logged_reads']} reads logged ({tot['log_bytes_used']} bytes), {tot['single_reads']} single, "
              f"{tot['corrected_reads']} corrected, {tot['unique_reads']} end unique; from HBM reads/s off {off['median']:.4g} (spread {d['device_spread_of_off']:.3f}), "
              f"on {on['median']:.4g} ({d['device_on_over_off']:.4f} of off), no LDS table {d['device_reads_per_s']['on, no LDS table']['median']:.4g}; "
              f"K3 {d['k3_ms']['on']['median']:.3f} ms, k8_log {d['k8_log_ms']['on']['median']:.3f} ms (no LDS table {d['k8_log_ms']['on, no LDS table']['median']:.3f}), "
              f"k8_replay {d['k8_replay_ms']['on']['median']:.3f} ms (no LDS table {d['k8_replay_ms']['on, no LDS table']['median']:.3f}): {w['replay_lookups']} lookups, "
              f"adds {w['replay_lds_adds']} LDS, {w['replay_global_adds']} global ({w['replay_spilled_adds']} past a full LDS table), grid {w['replay_grid']}", flush=True)
        db.close()
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
