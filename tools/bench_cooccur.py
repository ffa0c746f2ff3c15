#!/usr/bin/env python3
"""What do the shared reads of reference pairs (K7, kmcpg_set_cooccur) cost on a hit-heavy batch, and does the workgroups' LDS table do
its job?

The config1-shaped index of bench.py (10 k columns: 32 blocks x 312 columns, 150-bp reads, k = 21), every column a reference of its own,
and the family shape of tools/bench_families.py: every planted fragment sits in F = 57 neighbouring columns (a species of F close
relatives; profiles/r03_families.json has 57 hits per read), so a read names ~57 targets and K7 counts ~1 600 pairs for it — the
quadratic stage the reference warns about.  Two samples:
    even    the reads' families lie anywhere in the index: nearly every pair of a workgroup's reads is a new one
    sample  the reads come from 24 families only, as a metagenome's do: the same ~38 000 pairs over and over
Measured two ways, the forms alternated in one process:
  * from HBM: reads resident on the device, K1 + K2 (kmcpg_query_device), K3 (kmcpg_group_device) and, with the stage on, K7
    (kmcpg_cooccur_device) behind it on one stream — stage off, on, on with KMCPG_COOCCUR_SLOTS=0 (no LDS table).  Reads/s of whole steps
    (host clock around a synchronised step; a repetition is the median of its steps; median and range over the repetitions — the range of
    "off" is the noise floor) and HIP-event milliseconds of K3 and K7 for the same batch, with the witness of the last K7 launch;
  * at the library's boundary: kmcpg_search_batch of the same reads from host memory — stage off, on, and with every read left to the host
    half (KMCPG_COOCCUR_DEVICE=0: the host map takes every pair).
The counts are checked before anything is timed: device adds = the sum over the counted reads of m (m - 1) / 2 for their m targets.

    python tools/bench_cooccur.py [--batch 32768] [--relatives 57] [--steps 5] [--reps 5] [--host-steps 1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from kmcp_amd import Database, default_params, lib  # noqa: E402

SPEC = dict(k=21, num_hashes=1, fpr=0.3, n_blocks=32, cols_per_block=312, num_sigs=1121470, kmers_per_col=400000)  # bench.py WORKLOADS["config1"]
READ_LEN, FAMILIES = 150, 24


def make_batch(db, dev, n_reads, n_cols, seed, relatives, families):
    """random 150-bp fragments planted into `relatives` neighbouring columns each (10 % unrelated), queried with 1 % substitutions;
    families > 0: the first column of a read's family is one of that many"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    offs = (torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * READ_LEN).contiguous()
    code = torch.randint(0, 4, (n_reads * READ_LEN,), generator=g, device=dev, dtype=torch.uint8)
    cols = torch.randint(0, n_cols, (n_reads,), generator=g, device=dev).to(torch.int32)
    if families:
        first = torch.randint(0, n_cols, (families,), generator=g, device=dev).to(torch.int32)
        cols = first[torch.randint(0, families, (n_reads,), generator=g, device=dev)]
    cols[torch.rand(n_reads, generator=g, device=dev) < 0.10] = -1
    frag = acgt[code.long()].contiguous()
    for j in range(relatives):
        cj = torch.where(cols >= 0, (cols + j) % n_cols, cols).contiguous()
        db.plant_reads_device(frag.data_ptr(), offs.data_ptr(), n_reads, n_reads * READ_LEN, READ_LEN, cj.data_ptr())
    torch.cuda.synchronize()
    sub = torch.rand(code.numel(), generator=g, device=dev) < 0.01
    code[sub] = torch.randint(0, 4, (int(sub.sum().item()),), generator=g, device=dev, dtype=torch.uint8)
    return acgt[code.long()].contiguous(), offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--relatives", type=int, default=57)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=1, help="steps per repetition of the form that leaves every read to the host half")
    ap.add_argument("--table-slots", type=int, default=0, help="slots of the pair table (default: the library's)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cooccur.py needs a GPU")
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
               batch_reads=B, relatives=F, steps=a.steps, reps=a.reps, host_steps=a.host_steps, samples={})
    for sample in ("even", "sample"):
        db = Database.open_synthetic(lib.SynthSpec(seed=42, **SPEC), device=0)  # (a fresh index: the plantings of the other sample are gone)
        n_cols = int(db.info.n_cols)
        target = np.arange(n_cols, dtype=np.uint32)
        db.set_profiling(1)
        reads, offs = make_batch(db, dev, B, n_cols, 2000 + (sample == "sample"), F, FAMILIES if sample == "sample" else 0)
        h_reads, h_offs = reads.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)

        def set_stage(form):
            for k in ("KMCPG_COOCCUR_SLOTS", "KMCPG_COOCCUR_DEVICE"):
                os.environ.pop(k, None)
            if form == "off":
                db.set_cooccur()
                return
            if form == "on, no LDS table":
                os.environ["KMCPG_COOCCUR_SLOTS"] = "0"
            db.set_cooccur(target, table_slots=a.table_slots)
            os.environ.pop("KMCPG_COOCCUR_SLOTS", None)
            if form == "host only":
                os.environ["KMCPG_COOCCUR_DEVICE"] = "0"

        def step(on):
            """one batch from HBM; returns (seconds, K3 ms, K7 ms)"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            db.query_device(reads.data_ptr(), offs.data_ptr(), B, B * READ_LEN, READ_LEN, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_qk.data_ptr(), d_ql.data_ptr(),
                            params=params, stream=st.cuda_stream)
            ev[0].record(st)
            db.group_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_qk.data_ptr(), B, d_pairs.data_ptr(), d_roffs.data_ptr(), params=params, stream=st.cuda_stream)
            ev[1].record(st)
            if on:
                db.cooccur_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), B, 512, d_left.data_ptr(), d_n_hits=d_cnt.data_ptr(), hit_cap=cap,
                                  stream=st.cuda_stream)
            ev[2].record(st)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]) if on else 0.0

        def boundary():
            """one batch from host memory through kmcpg_search_batch; returns seconds"""
            t0 = time.perf_counter()
            db.search_packed_count(h_reads, h_offs, params=params)
            return time.perf_counter() - t0

        device_forms, boundary_forms = ("off", "on", "on, no LDS table"), ("off", "on", "host only")
        for f in device_forms:  # warm-up: every shape the timed window uses
            set_stage(f)
            step(f != "off")
        for f in boundary_forms[:2]:
            set_stage(f)
            boundary()
        # the counts themselves, before anything is timed: a counted read of m targets adds m (m - 1) / 2
        set_stage("on")
        step(True)
        wit, _ = db.last_cooccur()
        pairs_tab, tot = db.cooccur_read()
        roffs = d_roffs.cpu().numpy()
        left = d_left.cpu().numpy().astype(bool)
        lens = np.diff(roffs[:B + 1]).astype(np.int64)  # (every column is a reference: a read's pairs are its targets)
        assert wit["skipped"] == 0 and wit["bad_segments"] == 0, wit
        want = int((lens[~left] * (lens[~left] - 1) // 2).sum())
        assert tot["device_adds"] == want == int(pairs_tab["reads"].sum()) == wit["pairs"], (tot, want, wit)
        rate, k3, k7, witness = {f: [] for f in device_forms}, {f: [] for f in device_forms}, {f: [] for f in device_forms}, {}
        brate = {f: [] for f in boundary_forms}
        for rep in range(a.reps):  # the forms alternate: a drift of the machine hits all of them alike
            for f in device_forms:
                set_stage(f)
                got = [step(f != "off") for _ in range(a.steps)]
                rate[f].append(B / statistics.median(g_[0] for g_ in got))
                k3[f].append(statistics.median(g_[1] for g_ in got))
                k7[f].append(statistics.median(g_[2] for g_ in got))
                if f != "off":
                    witness[f] = db.last_cooccur()[0]
            for f in boundary_forms:
                set_stage(f)
                got = [boundary() for _ in range(a.host_steps if f == "host only" else a.steps)]
                brate[f].append(B / statistics.median(got))
                if f == "host only":
                    _, t2 = db.cooccur_read()
                    assert t2["device_adds"] == 0 and t2["host_adds"] > 0, t2
        set_stage("off")
        d = dict(pairs_per_batch=int(roffs[B]), hits_per_read=float(roffs[B]) / B, pair_adds_per_batch=want, distinct_pairs=int(len(pairs_tab)),
                 left_reads=int(left.sum()), left_for_a_full_table=tot["left_full"], table_slots=tot["table_slots"], table_keys=tot["keys"],
                 device_reads_per_s={f: summary(rate[f]) for f in device_forms}, k3_ms={f: summary(k3[f]) for f in device_forms},
                 k7_ms={f: summary(k7[f]) for f in device_forms if f != "off"}, boundary_reads_per_s={f: summary(brate[f]) for f in boundary_forms}, witness=witness)
        off, on = d["device_reads_per_s"]["off"], d["device_reads_per_s"]["on"]
        boff, bon, bhost = (d["boundary_reads_per_s"][f] for f in boundary_forms)
        d["device_on_over_off"] = on["median"] / off["median"]
        d["device_spread_of_off"] = (off["max"] - off["min"]) / off["median"]
        d["boundary_on_over_off"] = bon["median"] / boff["median"]
        d["boundary_host_only_over_off"] = bhost["median"] / boff["median"]
        d["boundary_spread_of_off"] = (boff["max"] - boff["min"]) / boff["median"]
        out["samples"][sample] = d
        w = witness["on"]
        print(f"{sample}: {d['hits_per_read']:.1f} hits per read, {want} pair adds on {d['distinct_pairs']} pairs, {d['left_reads']} reads left ({tot['left_full']} for a full table); "
              f"from HBM reads/s off {off['median']:.4g} (spread {d['device_spread_of_off']:.3f}), on {on['median']:.4g} ({d['device_on_over_off']:.4f} of off), "
              f"no LDS table {d['device_reads_per_s']['on, no LDS table']['median']:.4g}; K3 {d['k3_ms']['on']['median']:.3f} ms, K7 {d['k7_ms']['on']['median']:.3f} ms, "
              f"K7 without LDS table {d['k7_ms']['on, no LDS table']['median']:.3f} ms; K7 adds: {w['lds_adds']} LDS, {w['global_adds']} global ({w['spilled_adds']} past a full "
              f"LDS table), grid {w['grid']}; at the boundary reads/s off {boff['median']:.4g} (spread {d['boundary_spread_of_off']:.3f}), on {bon['median']:.4g} "
              f"({d['boundary_on_over_off']:.4f} of off), host only {bhost['median']:.4g} ({d['boundary_host_only_over_off']:.4f} of off)", flush=True)
        db.close()
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
