#!/usr/bin/env python3
"""What do the reference statistics (K6, kmcpg_set_refstats) cost, and does the workgroups' LDS table do its job?

The config1-shaped search of bench.py (10 k chunks: 32 blocks x 312 columns, 150-bp reads, k = 21) from HBM: reads resident on the device,
K1 + K2 (kmcpg_query_device), K3 (kmcpg_group_device) and, with the stage on, K6 (kmcpg_refstats_device) behind it on the same stream.
Ten columns are one reference (its chunks).  Two hit distributions:
    even     every planted read has a column of its own choosing, uniformly over the index
    skewed   half of the planted reads lie on ONE reference (10 columns): the case that would serialise plain global atomics
and three forms of a step, alternated in one process: stage off, stage on, stage on with KMCPG_REFSTATS_SLOTS=0 (no LDS table: every add a
global atomic — the plain-atomics baseline).  Per form: reads/s of whole steps (host clock around a synchronised step; a repetition is
the median of its steps; median and range over the repetitions — the range of "off" is the noise floor), and HIP-event milliseconds of K3
and of K6 for the same batch, with the witness of the last K6 launch.

The yardstick needs no constant: K6 reads the pairs once, K3 reads, sorts and writes them — K6 slower than K3 on the skewed distribution
means it is bound by contention, not by the pairs.

    python tools/bench_refstats.py [--batch 1048576] [--steps 5] [--reps 5] [--out FILE]
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
READ_LEN, CHUNKS, POOL = 150, 10, 20000


def make_batch(db, dev, n_reads, n_cols, seed, skewed):
    """random 150-bp fragments planted into their columns (10 % unrelated), queried with 1 % substitutions"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    offs = (torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * READ_LEN).contiguous()
    code = torch.randint(0, 4, (n_reads * READ_LEN,), generator=g, device=dev, dtype=torch.uint8)
    cols = torch.randint(0, n_cols, (n_reads,), generator=g, device=dev).to(torch.int32)
    if skewed:
        # the hot reference holds POOL distinct fragments (what its columns have room for); half of the reads are copies of them
        hot = torch.rand(n_reads, generator=g, device=dev) < 0.5
        pick = torch.randint(0, POOL, (n_reads,), generator=g, device=dev)
        pool = torch.randint(0, 4, (POOL, READ_LEN), generator=g, device=dev, dtype=torch.uint8)
        code = torch.where(hot[:, None], pool[pick], code.view(n_reads, READ_LEN)).contiguous().view(-1)
        cols = torch.where(hot, (CHUNKS * 333 + pick % CHUNKS).to(torch.int32), cols)
    cols[torch.rand(n_reads, generator=g, device=dev) < 0.10] = -1
    cols = cols.contiguous()
    frag = acgt[code.long()].contiguous()
    db.plant_reads_device(frag.data_ptr(), offs.data_ptr(), n_reads, n_reads * READ_LEN, READ_LEN, cols.data_ptr())
    torch.cuda.synchronize()
    sub = torch.rand(code.numel(), generator=g, device=dev) < 0.01
    code[sub] = torch.randint(0, 4, (int(sub.sum().item()),), generator=g, device=dev, dtype=torch.uint8)
    return acgt[code.long()].contiguous(), offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1048576)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--wgs", type=int, default=0, help="KMCPG_REFSTATS_WGS for the stage: K6's grid (default: the library's)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refstats.py needs a GPU")
    B, dev = a.batch, torch.device("cuda", 0)
    db = Database.open_synthetic(lib.SynthSpec(seed=42, **SPEC), device=0)
    n_cols = int(db.info.n_cols)
    target = (np.arange(n_cols) // CHUNKS).astype(np.uint32)
    params = default_params()
    db.set_profiling(1)
    cap = 8 * B + 4096
    d_hits = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    d_qk, d_ql = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    d_pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    d_roffs = torch.zeros(B + 2, dtype=torch.int64, device=dev)
    d_left = torch.zeros(B, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def set_stage(form):
        os.environ.pop("KMCPG_REFSTATS_SLOTS", None)
        if form == "off":
            db.set_refstats()
            return
        if form == "on, no table":
            os.environ["KMCPG_REFSTATS_SLOTS"] = "0"
        if a.wgs:
            os.environ["KMCPG_REFSTATS_WGS"] = str(a.wgs)
        db.set_refstats(target, None, hic_min_qcov=0.75)
        os.environ.pop("KMCPG_REFSTATS_SLOTS", None)

    def step(reads, offs, on):
        """one batch; returns (seconds, K3 ms, K6 ms)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db.query_device(reads.data_ptr(), offs.data_ptr(), B, B * READ_LEN, READ_LEN, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_qk.data_ptr(), d_ql.data_ptr(),
                        params=params, stream=st.cuda_stream)
        ev[0].record(st)
        db.group_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_qk.data_ptr(), B, d_pairs.data_ptr(), d_roffs.data_ptr(), params=params, stream=st.cuda_stream)
        ev[1].record(st)
        if on:
            db.refstats_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), B, 512, d_left.data_ptr(), d_n_hits=d_cnt.data_ptr(), hit_cap=cap,
                               stream=st.cuda_stream)
        ev[2].record(st)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]) if on else 0.0

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v))

    out = dict(workload="config1-shaped: 32 blocks x 312 columns, 150-bp reads, k = 21, -t 0.55; 10 columns = one reference", batch_reads=B, steps=a.steps, reps=a.reps,
               distributions={})
    forms = ("off", "on", "on, no table")
    for dist in ("even", "skewed"):
        reads, offs = make_batch(db, dev, B, n_cols, 1000 + (dist == "skewed"), dist == "skewed")
        for f in forms:  # warm-up: every shape the timed window uses
            set_stage(f)
            step(reads, offs, f != "off")
        # the counts themselves: every pair of a counted read is one row
        set_stage("on")
        step(reads, offs, True)
        cols, tot = db.refstats_read(n_cols)
        wit, _ = db.last_refstats()
        roffs = d_roffs.cpu().numpy()
        left = d_left.cpu().numpy().astype(bool)
        lens = np.diff(roffs[:B + 1])
        assert wit["skipped"] == 0 and wit["bad_segments"] == 0, wit
        assert int(cols["rows"].sum()) == int(lens[~left].sum()), ("rows", int(cols["rows"].sum()), int(lens[~left].sum()))
        assert tot["matched_reads"] == int((lens[~left] > 0).sum()), ("matched reads", tot, int((lens[~left] > 0).sum()))
        hot_share = float(np.bincount(target, weights=cols["rows"].astype(np.float64)).max() / max(1, cols["rows"].sum()))
        rate = {f: [] for f in forms}  # per repetition: the median of its steps
        k3 = {f: [] for f in forms}
        k6 = {f: [] for f in forms}
        witness = {}
        for rep in range(a.reps):  # the forms alternate: a drift of the machine hits all of them alike
            for f in forms:
                set_stage(f)
                got = [step(reads, offs, f != "off") for _ in range(a.steps)]
                rate[f].append(B / statistics.median(g_[0] for g_ in got))
                k3[f].append(statistics.median(g_[1] for g_ in got))
                k6[f].append(statistics.median(g_[2] for g_ in got))
                if f != "off":
                    witness[f] = db.last_refstats()[0]
        set_stage("off")
        d = dict(pairs_per_batch=int(roffs[B]), matched_reads=tot["matched_reads"], rows_on_the_fullest_reference=hot_share, left_reads=int(left.sum()),
                 reads_per_s={f: summary(rate[f]) for f in forms}, k3_ms={f: summary(k3[f]) for f in forms}, k6_ms={f: summary(k6[f]) for f in forms if f != "off"},
                 witness=witness)
        off, on = d["reads_per_s"]["off"], d["reads_per_s"]["on"]
        d["on_over_off"] = on["median"] / off["median"]
        d["spread_of_off"] = (off["max"] - off["min"]) / off["median"]
        out["distributions"][dist] = d
        print(f"{dist}: {d['pairs_per_batch']} pairs, fullest reference {hot_share:.3f} of the rows; reads/s off {off['median']:.4g} (spread {d['spread_of_off']:.3f}), "
              f"on {on['median']:.4g} ({d['on_over_off']:.4f} of off), no table {d['reads_per_s']['on, no table']['median']:.4g}; "
              f"K3 {d['k3_ms']['on']['median']:.3f} ms, K6 {d['k6_ms']['on']['median']:.3f} ms, K6 without table {d['k6_ms']['on, no table']['median']:.3f} ms; "
              f"K6 adds: {witness['on']['lds_adds']} LDS, {witness['on']['global_adds']} global ({witness['on']['spilled_adds']} spilled), grid {witness['on']['grid']}", flush=True)
    db.close()
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
