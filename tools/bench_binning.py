#!/usr/bin/env python3
"""What does taxonomic binning on the GPU (kmcpg_submit_bins / kmcpg_wait_bins, K11) cost, and what does it bring off the device?

(a) At the library's boundary, on the config1-shaped index of bench.py and the two batch shapes of tools/bench_cooccur.py (one hit per
    read; the family shape, F = 57 neighbouring columns): one handle with the species-specific stage (K4) on, every column a class, and
    the binning stage with two plans in turn — "all": every column a whitelisted reference, a leaf under one of 64 genera under one
    root (about 10 000 nodes: the climb reads global memory); "sample": every 48th column whitelisted (208 references, 274 nodes: the
    tables sit in LDS, the shape of a real sample).  Reported per shape and plan: the HIP-event time of K11 for one batch beside K4's on
    the SAME K3 output (kmcpg_bin_device and kmcpg_specific_device on the pairs of kmcpg_group_device, profiling level 1, median and
    range of --reps), and the bytes a bins ticket brings from the device beside those of a pairs ticket.
(b) The wall time of `kmcp-search --binning` beside the same command with `-o` (median and range of --reps runs each, the two
    alternating; the `-o` side exists without this feature and is the yardstick), on --db DIR --reads FILE --refs P --taxid-map M
    --taxdump X, or with --family N on the family database of tools/family_db.py (16 base genomes, 51 references) with N of its reads,
    every reference listed, under a taxonomy written here.

    python tools/bench_binning.py [--batch 32768] [--relatives 57] [--reps 5] [--family N | --db DIR --reads FILE --refs P --taxid-map M --taxdump X] [--out FILE]
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


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def plan_for(n_cols, genera=64, every=1):
    """root 1 -> `genera` genera -> one leaf per whitelisted column (every `every`-th), in pre-order under the virtual root:
    (node_of_column, parent, last, taxid); a column off the whitelist has node 0xffffffff"""
    parent, last, taxid, node = [0, 0], [0, 0], [0, 1], np.full(n_cols, 0xFFFFFFFF, dtype=np.uint32)
    per = -(-n_cols // genera)
    for g in range(genera):
        cols = [c for c in range(g * per, min(n_cols, (g + 1) * per)) if c % every == 0]
        if not len(cols):
            continue
        gnode = len(parent)
        parent.append(1), last.append(gnode + len(cols)), taxid.append(100 + g)
        for c in cols:
            node[c] = len(parent)
            parent.append(gnode), last.append(len(parent) - 1), taxid.append(100000 + c)
    last[0] = last[1] = len(parent) - 1
    return node, np.array(parent, dtype=np.uint32), np.array(last, dtype=np.uint32), np.array(taxid, dtype=np.uint32)


def library_side(a, out):
    import torch
    from bench_cooccur import READ_LEN, SPEC, make_batch
    from kmcp_amd import Database, default_params, lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_binning.py needs a GPU")
    B, dev = a.batch, torch.device("cuda", 0)
    params = default_params()
    for shape, F in (("config1", 1), ("even", a.relatives)):
        db = Database.open_synthetic(lib.SynthSpec(seed=42, **SPEC), device=0)
        n_cols = int(db.info.n_cols)
        reads, offs = make_batch(db, dev, B, n_cols, 3000 + F, F, 0)
        h_reads, h_offs = reads.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)
        pairs = db.wait_pairs(db.submit(h_reads, h_offs, params=params), count_only=True)
        # K11 beside K4 on the same K3 output
        cap = max(int(pairs) * 2, 1024)
        d_hits = torch.empty(cap * 3, dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        d_qk, d_ql = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        db.query_device(reads.data_ptr(), offs.data_ptr(), B, B * READ_LEN, READ_LEN, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_qk.data_ptr(), d_ql.data_ptr(), params=params)
        d_pairs, d_roffs = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(B + 2, dtype=torch.int64, device=dev)
        db.group_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_qk.data_ptr(), B, d_pairs.data_ptr(), d_roffs.data_ptr(), params=params)
        torch.cuda.synchronize()
        d_bins = torch.empty(B, dtype=torch.int32, device=dev)
        d_out, d_ooffs, d_verd = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(B + 1, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
        out["shapes"][shape] = {}
        for plan, every in (("all", 1), ("sample", 48)):
            node, parent, last, taxid = plan_for(n_cols, every=every)
            db.set_profiling(0)
            db.set_specific()  # (a bins ticket refuses a handle with K4 on)
            db.set_binning(node, parent, last, taxid)
            # the tickets: bytes from the device, and that both routes say the same about the batch
            for _ in range(3):
                bins, st = db.wait_bins(db.submit_bins(h_reads, h_offs, params=params))
            assert st["kept_pairs"] == pairs, (st, pairs)
            db.set_specific(np.arange(n_cols, dtype=np.uint32), None)
            db.set_profiling(1)
            k11, k4 = [], []
            for _ in range(a.reps + 1):  # the two kernels alternate; the first pair is dropped
                db.bin_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), B, 1 << 30, d_bins.data_ptr())
                w, _ = db.last_bins()
                k11.append(db.last_k11_ms)
                db.specific_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), B, 1 << 30, d_out.data_ptr(), cap, d_ooffs.data_ptr(), d_verd.data_ptr())
                db.last_specific()
                k4.append(db.last_k4_ms)
            d = dict(hits_per_read=pairs / B, references=int((node != 0xFFFFFFFF).sum()), plan_nodes=len(parent), in_lds=w["in_lds"], binned_reads=st["binned_reads"],
                     host_reads=st["host_reads"], several=w["several"], climb_steps=w["climb_steps"], k11_ms=summary(k11[1:]), k4_ms=summary(k4[1:]),
                     bytes_per_ticket=dict(bins=st["bytes_d2h"], pairs=8 * int(pairs) + B * 16 + 32))
            out["shapes"][shape][plan] = d
            print(f"{shape} / {plan}: {d['hits_per_read']:.1f} hits per read, {d['references']} references, plan of {len(parent)} nodes (in LDS: {w['in_lds']}), "
                  f"{d['binned_reads']} of {B} reads binned ({d['several']} by a climb of {d['climb_steps']} steps in all); K11 {d['k11_ms']['median']:.4f} ms "
                  f"({d['k11_ms']['min']:.4f} - {d['k11_ms']['max']:.4f}) beside K4 {d['k4_ms']['median']:.4f} ms ({d['k4_ms']['min']:.4f} - {d['k4_ms']['max']:.4f}) per batch; "
                  f"bytes per ticket {d['bytes_per_ticket']['pairs']} -> {d['bytes_per_ticket']['bins']}", flush=True)
        db.close()


def family_inputs(a, tmp):
    """the family database with a.family of its reads as FASTQ, every reference listed, a genus per accession with its strains by turns
    in two species: fills a.db, a.reads, a.refs, a.taxid_map, a.taxdump"""
    import family_db
    from kmcp_amd import lib
    cols, reads, _ = family_db.generate(ecoli_strains=6, small_strains=3, n_reads=a.family)
    whole = lib.build_db(os.path.join(tmp, "db"), cols, k=family_db.K, threads=8, alias="family-db")
    names = sorted({c[0] for c in cols})
    accs = sorted({n.rsplit(".s", 1)[0] for n in names})
    nodes, tmap = ["1\t|\t1\t|\tno rank\t|\n"], []
    for gi in range(len(accs)):
        nodes.append(f"{100 + gi}\t|\t1\t|\tgenus\t|\n")
        nodes += [f"{1000 + 2 * gi + h}\t|\t{100 + gi}\t|\tspecies\t|\n" for h in range(2)]
    for n in names:
        acc, si = n.rsplit(".s", 1)
        gi = accs.index(acc)
        nodes.append(f"{50000 + 100 * gi + int(si)}\t|\t{1000 + 2 * gi + int(si) % 2}\t|\tstrain\t|\n")
        tmap.append(f"{n}\t{50000 + 100 * gi + int(si)}\n")
    os.makedirs(os.path.join(tmp, "tax"))
    open(os.path.join(tmp, "tax", "nodes.dmp"), "w").writelines(nodes)
    open(os.path.join(tmp, "map.tsv"), "w").writelines(tmap)
    open(os.path.join(tmp, "refs.txt"), "w").write("".join(n + "\n" for n in names))
    family_db.write_fastq(os.path.join(tmp, "r.fq"), reads)
    a.db, a.reads, a.refs, a.taxid_map, a.taxdump = os.path.dirname(whole), os.path.join(tmp, "r.fq"), os.path.join(tmp, "refs.txt"), os.path.join(tmp, "map.tsv"), os.path.join(tmp, "tax")
    return f"family database: {len(names)} references, {reads.shape[0]} reads of {reads.shape[1]} bp, every reference listed"


def cli_side(a, out):
    cli = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
    wall = dict(tsv=[], binning=[])
    with tempfile.TemporaryDirectory() as tmp:
        what = family_inputs(a, tmp) if a.family else f"{a.db}, {a.reads}, {a.refs}"
        base = [cli, "-d", a.db, a.reads, "-q"]
        for rep in range(a.reps + 1):  # (the first pair warms the page cache and is dropped)
            for route, extra in (("tsv", ["-o", os.path.join(tmp, "o.tsv")]),
                                 ("binning", ["--binning", os.path.join(tmp, "b.binning"), "--binning-refs", a.refs, "--taxid-map", a.taxid_map, "--taxdump", a.taxdump])):
                t0 = time.perf_counter()
                subprocess.run(base + extra, check=True, capture_output=True)
                if rep:
                    wall[route].append(time.perf_counter() - t0)
        sizes = dict(tsv=os.path.getsize(os.path.join(tmp, "o.tsv")), binning=os.path.getsize(os.path.join(tmp, "b.binning")))
    out["cli"] = dict(input=what, wall_s={r: summary(v) for r, v in wall.items()}, file_bytes=sizes)
    w = out["cli"]["wall_s"]
    print(f"kmcp-search on {what}: -o {w['tsv']['median']:.3f} s ({w['tsv']['min']:.3f} - {w['tsv']['max']:.3f}; {sizes['tsv']} bytes written), "
          f"--binning {w['binning']['median']:.3f} s ({w['binning']['min']:.3f} - {w['binning']['max']:.3f}; {sizes['binning']} bytes written)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--relatives", type=int, default=57)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--family", type=int, default=0, help="reads of the family database for the command-line side (0: none, unless --db is given)")
    ap.add_argument("--db", default="")
    ap.add_argument("--reads", default="")
    ap.add_argument("--refs", default="")
    ap.add_argument("--taxid-map", default="")
    ap.add_argument("--taxdump", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = dict(workload="config1-shaped: 32 blocks x 312 columns, two plans (every column / every 48th column whitelisted), 150-bp reads, k = 21, -t 0.55", batch_reads=a.batch, reps=a.reps, shapes={})
    library_side(a, out)
    if a.db or a.family:
        cli_side(a, out)
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
