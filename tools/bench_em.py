#!/usr/bin/env python3
"""What does one EM pass (K9, kmcpg_em_pass) cost over a resident read log, does the workgroups' LDS table help, and what do the default
11 passes of the loop cost?  The measurement behind the default of KMCPG_EM_SLOTS.

The workload of tools/bench_recount.py: the config1-shaped index of bench.py (10 k columns, 150-bp reads, k = 21), every column a
reference of its own, every planted fragment in F = 57 neighbouring columns, so a read names ~57 targets and a pass shares it out over
up to 57 of them.  Two samples:
    even    the reads' families lie anywhere in the index
    sample  the reads come from 24 families only, as a metagenome's do: the adds fall on a few hundred columns
One batch is searched and logged (K1 + K2, K3, k8_log on device pointers); nine references in ten are on the whitelist, their coverages
drawn over four orders of magnitude.  The forms alternate in one process, three runs each (a run is the median of its passes):
    LDS table      KMCPG_EM_SLOTS=1024       HIP-event time of k9_em (the witness, profiling level 1)
    no LDS table   KMCPG_EM_SLOTS=0          the same
    host half      every read in the host log (the batch searched through the library with KMCPG_RECOUNT_DEVICE=0): host clock around
                   kmcpg_em_pass
and the whole loop of the default 11 passes — kmcpg_em_pass, kmcpg_em_read and a coverage per reference from the columns, in numpy — by the
host clock.  Before anything is timed the three forms must give the same bytes.

    python tools/bench_em.py [--batch 32768] [--relatives 57] [--passes 5] [--reps 3] [--out FILE]
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
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_em.py needs a GPU")
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

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v))

    out = dict(workload=f"config1-shaped: 32 blocks x 312 columns, every column a reference, 150-bp reads, k = 21, -t 0.55; every fragment in {F} neighbouring columns",
               batch_reads=B, relatives=F, passes=a.passes, reps=a.reps, samples={})
    for sample in ("even", "sample"):
        db = Database.open_synthetic(lib.SynthSpec(seed=42, **SPEC), device=0)
        n_cols = int(db.info.n_cols)
        target = np.arange(n_cols, dtype=np.uint32)
        db.set_profiling(1)
        reads, offs = make_batch(db, dev, B, n_cols, 2000 + (sample == "sample"), F, FAMILIES if sample == "sample" else 0)
        h_reads, h_offs = reads.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)
        rng = np.random.default_rng(7)
        classes = np.zeros(n_cols, dtype=lib.EM_CLASS_DTYPE)
        classes["est"] = rng.random(n_cols) < 0.9
        classes["coverage"] = rng.choice([0.01, 0.1, 1.0, 10.0, 100.0], size=n_cols) * rng.uniform(0.5, 2.0, size=n_cols)

        def log_on_device():
            db.set_recount(target, None, hic_min_qcov=0.75, log_bytes=1 << 30)
            db.query_device(reads.data_ptr(), offs.data_ptr(), B, B * READ_LEN, READ_LEN, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_qk.data_ptr(), d_ql.data_ptr(),
                            params=params, stream=st.cuda_stream)
            db.group_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_qk.data_ptr(), B, d_pairs.data_ptr(), d_roffs.data_ptr(), params=params, stream=st.cuda_stream)
            db.recount_log_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), d_ql.data_ptr(), B, 512, d_left.data_ptr(), d_n_hits=d_cnt.data_ptr(), hit_cap=cap,
                                  stream=st.cuda_stream)
            torch.cuda.synchronize()

        def log_on_host():
            os.environ["KMCPG_RECOUNT_DEVICE"] = "0"
            try:
                db.set_recount(target, None, hic_min_qcov=0.75, log_bytes=1 << 30)
                db.search_packed_count(h_reads, h_offs, params=params)
            finally:
                os.environ.pop("KMCPG_RECOUNT_DEVICE")

        def one_pass(slots, cls=classes):
            """-> (HIP-event ms of k9_em or -1, host seconds of kmcpg_em_pass)"""
            os.environ["KMCPG_EM_SLOTS"] = str(slots)
            try:
                t0 = time.perf_counter()
                db.em_pass(cls, level_species=False)
                dt = time.perf_counter() - t0
            finally:
                os.environ.pop("KMCPG_EM_SLOTS")
            wit, _ = db.last_em()
            return db.last_k9_ms, dt, wit

        def loop(slots, n_passes=11):
            """the default 11 passes with a coverage per reference from the columns; host seconds"""
            cls = classes.copy()
            t0 = time.perf_counter()
            for _ in range(n_passes):
                one_pass(slots, cls)
                got, _ = db.em_read()
                b = got["single_bases"] / 65536.0 + (got["bases_hi"] * 4294967296.0 + got["bases_lo"]) / float(lib.EM_UNIT)
                cls["coverage"] = np.where(cls["est"] != 0, np.maximum(b / 1e3, 1e-12), cls["coverage"])
            return time.perf_counter() - t0

        # the three forms give the same bytes (the LEFT reads of the device route are not in the device pointers' log: compare what both hold)
        log_on_device()
        one_pass(1024)
        with_table, tot = db.em_read()
        one_pass(0)
        without, tot0 = db.em_read()
        assert with_table.tobytes() == without.tobytes() and tot == tot0 and tot["split_reads"] > 0, (tot, tot0)
        assert int(with_table["match"].sum()) == tot["assigned_reads"] * lib.EM_UNIT
        left = int(d_left.sum().item())
        ms = {f: [] for f in ("LDS table", "no LDS table")}
        host_s, loop_s, witness = [], {f: [] for f in ms}, {}
        for rep in range(a.reps):  # the forms alternate: a drift of the machine hits all of them alike
            log_on_device()
            for f, slots in (("LDS table", 1024), ("no LDS table", 0)):
                got = [one_pass(slots) for _ in range(a.passes)]
                ms[f].append(statistics.median(g[0] for g in got))
                witness[f] = got[-1][2]
                loop_s[f].append(loop(slots))
            log_on_host()
            got = [one_pass(0) for _ in range(a.passes)]
            host_s.append(statistics.median(g[1] for g in got))
            host_cols, host_tot = db.em_read()
            if left == 0:
                assert host_cols.tobytes() == with_table.tobytes(), "the host half counts what the device counts"
        db.set_recount()
        d = dict(totals=tot, left_by_k8_log=left, host_log_reads=host_tot["host_reads"], k9_ms={f: summary(ms[f]) for f in ms}, host_half_ms=summary([1e3 * s for s in host_s]),
                 loop_11_passes_ms={f: summary([1e3 * s for s in loop_s[f]]) for f in loop_s}, witness=witness)
        out["samples"][sample] = d
        w, w0 = witness["LDS table"], witness["no LDS table"]
        print(f"{sample}: {w['reads']} logged reads ({w['split']} split, {w['one']} with one estimated target, {w['none']} with none), grid {w['grid']}; k9_em "
              f"{d['k9_ms']['LDS table']['median']:.3f} ms with the LDS table ({w['lds_adds']} LDS adds, {w['global_adds']} global, {w['spilled_adds']} spilled), "
              f"{d['k9_ms']['no LDS table']['median']:.3f} ms without ({w0['global_adds']} global adds); host half {d['host_half_ms']['median']:.1f} ms; "
              f"11 passes {d['loop_11_passes_ms']['LDS table']['median']:.1f} ms / {d['loop_11_passes_ms']['no LDS table']['median']:.1f} ms", flush=True)
        db.close()
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
