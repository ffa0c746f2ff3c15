#!/usr/bin/env python3
"""Sketching a batch of genomes for a database build: kmcpg_sketch_genomes (chunks read in place, K1, ONE segmented sort + unique
for the batch: sort_segments.hip) against the only route the library had before it — kmcpg_kmers_device with dedup_threshold = 0 on a
throw-away synthetic handle, one call per genome over its chunks laid out as reads, every list copied to the host, as
tools/family_db.py drives K1 (per-workgroup sorts up to 65 536 k-mers, a device-wide sort per longer chunk: sort_huge.hip).

Shapes (ISSUE "Measurement"):  a  64 genomes x 4 Mbp x 10 chunks, plain k = 21
                               b  the same, FracMinHash scale 10
                               c  2 000 genomes x 100 kbp x 10 chunks (every chunk below 65 536 k-mers)
Both paths start from genomes in host memory and end with sorted-unique lists in host memory.  Runs alternate (new, old, new, old ...)
after one warm-up of each; per shape the script reports the median and the spread (max - min) of both, the launch witness, the
HIP-event split of the new path (k-mer kernels | segmented sort) and the sort's rate.  The lists of both paths are compared once.
--makedb times kmcp-makedb end to end on the shape's genomes written as .fa.gz to /dev/shm.
--makedb --two-pass times `kmcp-makedb --two-pass` against the one-pass default instead, on the same genomes as .fa and as .fa.gz: one
warm-up of each, then alternating runs (one-pass, two-pass, ...), wall time of the command plus the phases of its log lines; the
scatter kernel's keys/s (its HIP-event time) beside the one-pass index stage and beside kmcpg_stream_probe over the finished database,
the yardstick for what the memory system streams.  The two databases are compared file by file.

  python tools/bench_makedb.py --shape a --repeats 5 --out profiles/r09_makedb.json
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "a": dict(genomes=64, length=4000000, scale=1),
    "b": dict(genomes=64, length=4000000, scale=10),
    "c": dict(genomes=2000, length=100000, scale=1),
}
K, SPLIT, OVERLAP = 21, 10, 150
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_genomes(n, length, seed=1):
    """genome 0 .. : the reference's demo genomes (tests/golden) tiled to `length` where there are any, then uniform random ones"""
    out = []
    try:
        from tests.test_gpu_config0 import load_genomes
        for acc, recs in sorted(load_genomes().items())[:min(4, n)]:
            s = (b"N" * (K - 1)).join(r for name, r in recs if "plasmid" not in name)
            out.append((s * (length // len(s) + 1))[:length])
    except Exception:
        pass
    rng = np.random.default_rng(seed)
    while len(out) < n:
        out.append(_ACGT[rng.integers(0, 4, size=length)].tobytes())
    return out[:n]


class OldPath:
    """kmcpg_kmers_device, dedup_threshold 0, one call per genome (tools/family_db.py Builder.add_genome without torch.unique)"""

    def __init__(self, lib, scale, device=0):
        import torch
        from kmcp_amd import Database
        self.torch, self.lib = torch, lib
        self.dev = torch.device("cuda", device)
        spec = lib.SynthSpec(k=K, num_hashes=1, fpr=0.3, n_blocks=1, cols_per_block=8, num_sigs=1024, kmers_per_col=100, seed=1, scale=scale)
        self.db = Database.open_synthetic(spec, device=device)
        self.params = lib.default_params(dedup_threshold=0, min_qlen=0, min_matched=1)

    def close(self):
        self.db.close()

    def run(self, genomes, bounds):
        torch = self.torch
        lists = []
        for g, bd in zip(genomes, bounds):
            if not bd:
                continue
            seq = torch.frombuffer(bytearray(g), dtype=torch.uint8).to(self.dev)
            parts = [seq[a:b] for a, b in bd]
            lens = torch.tensor([p.numel() for p in parts], dtype=torch.int64)
            n = len(parts)
            offs = torch.zeros(n + 1, dtype=torch.int64)
            offs[1:] = torch.cumsum(lens, 0)
            total = int(offs[-1])
            d_seq = torch.cat(parts).contiguous()
            d_offs = offs.to(self.dev)
            d_h = torch.empty(total, dtype=torch.int64, device=self.dev)
            d_ko = torch.empty(n, dtype=torch.int64, device=self.dev)
            d_nk = torch.empty(n, dtype=torch.int32, device=self.dev)
            self.db.kmers_device(d_seq.data_ptr(), d_offs.data_ptr(), n, total, int(lens.max()), d_h.data_ptr(), total, d_ko.data_ptr(), d_nk.data_ptr(),
                                 params=self.params)
            torch.cuda.synchronize()
            nk = d_nk.cpu().tolist()
            for ci in range(n):
                lists.append(d_h[int(offs[ci]):int(offs[ci]) + nk[ci]].cpu().numpy().view(np.uint64))
        return lists


def run_shape(name, spec, args, lib):
    import torch
    n = args.genomes or spec["genomes"]
    genomes = make_genomes(n, spec["length"])
    bounds = [lib.split_bounds(len(g), SPLIT, OVERLAP, 1000, K) for g in genomes]
    res = dict(shape=name, genomes=n, length=spec["length"], chunks=sum(len(b) for b in bounds), k=K, scale=spec["scale"])
    old = None if args.no_yardstick else OldPath(lib, spec["scale"])
    new_t, old_t, dev_ms, witness = [], [], [], None
    with lib.Sketcher(k=K, scale=spec["scale"], device=0) as sk:
        for rep in range(-1, args.repeats):  # -1: warm-up (allocations, code objects)
            t0 = time.perf_counter()
            with sk.sketch(genomes, split_number=SPLIT, split_overlap=OVERLAP, split_min_ref=1000) as got:
                t1 = time.perf_counter()
                if rep == -1:
                    new_lists = [got.list(i).copy() for i in range(len(got))] if old else None
                    res["unique_kmers"] = int(got.koff[len(got)])
            if rep >= 0:
                new_t.append(t1 - t0)
                dev_ms.append(sk.last_sketch_ms())
            witness = sk.last_sketch_launches()
            if old:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lists = old.run(genomes, bounds)
                t1 = time.perf_counter()
                if rep >= 0:
                    old_t.append(t1 - t0)
                else:
                    assert len(lists) == len(new_lists), (len(lists), len(new_lists))
                    for i, (x, y) in enumerate(zip(lists, new_lists)):
                        assert np.array_equal(x, y), f"list {i} differs between the two paths"
                    res["lists_equal"] = True
                    new_lists = None
                lists = None
    if old:
        old.close()
    med = statistics.median
    res["new_s"] = dict(median=med(new_t), min=min(new_t), max=max(new_t), spread=max(new_t) - min(new_t), runs=new_t)
    if old_t:
        res["old_s"] = dict(median=med(old_t), min=min(old_t), max=max(old_t), spread=max(old_t) - min(old_t), runs=old_t)
        res["speedup"] = med(old_t) / med(new_t)
        # the old path's launches follow from its structure (query.cpp run_kmers): per genome K1 (3 kernels), launch_dedup (2-6), two
        # read-backs, and per chunk above 65 536 k-mers 8 x 5 + 7 launches of sort_huge.hip
    res["witness"] = witness
    km, so = med([d[0] for d in dev_ms]), med([d[1] for d in dev_ms])
    keys = sum(w["keys"] for w in witness)
    passes = witness[0]["passes"] if witness else 0
    res["device_ms"] = dict(kmers=km, sort_unique=so)
    if so > 0:
        # bytes the sort moves: per pass the keys are read twice (histogram, scatter) and written once; the unique pass reads twice, writes once
        moved = keys * 8 * 3 * (passes + 1)
        res["sort"] = dict(keys=keys, passes=passes, keys_per_s=keys / (so / 1e3), bytes_moved=moved, bytes_per_s=moved / (so / 1e3),
                           of_streaming_6_25_TBps=moved / (so / 1e3) / 6.25e12)
    if args.makedb:
        res["makedb"] = run_makedb(genomes, spec)
    return res


def run_two_pass(name, spec, args, lib):
    """kmcp-makedb --two-pass against one-pass, end to end"""
    import filecmp
    import re
    n = args.genomes or spec["genomes"]
    genomes = make_genomes(n, spec["length"])
    exe = os.path.join(ROOT, "kmcp_amd", "kmcp-makedb")
    tmp = tempfile.mkdtemp(prefix="bench_two_pass_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    res = dict(shape=name, genomes=n, length=spec["length"], k=K, scale=spec["scale"], inputs={})
    med = statistics.median
    try:
        for form in ("fa", "fa.gz"):
            files = []
            for i, g in enumerate(genomes):
                p = os.path.join(tmp, f"g{i:05d}.{form}")
                with (gzip.open(p, "wb", compresslevel=1) if form.endswith("gz") else open(p, "wb")) as fh:
                    fh.write(b">g%d chromosome\n" % i)
                    fh.write(b"\n".join(g[j:j + 80] for j in range(0, len(g), 80)) + b"\n")
                files.append(p)
            lst = os.path.join(tmp, f"files_{form}.txt")
            with open(lst, "w") as fh:
                fh.write("\n".join(files) + "\n")
            base = [exe, "-k", str(K), "-n", str(SPLIT), "-l", str(OVERLAP), "--num-hash", "1", "-f", "0.3", "-j", "16", "-i", lst, "--force"]
            if spec["scale"] > 1:
                base += ["-D", str(spec["scale"])]
            dirs = dict(one=os.path.join(tmp, "one.kmcp"), two=os.path.join(tmp, "two.kmcp"))
            cmds = dict(one=base + ["-O", dirs["one"]], two=base + ["--two-pass", "-O", dirs["two"]] + (["--matrix-budget", args.matrix_budget] if args.matrix_budget else []))
            runs = dict(one=[], two=[])
            for rep in range(-1, args.repeats):  # -1: warm-up (page cache, code objects)
                for mode in ("one", "two"):
                    t0 = time.perf_counter()
                    r = subprocess.run(cmds[mode], capture_output=True, text=True, timeout=900)
                    wall = time.perf_counter() - t0
                    assert r.returncode == 0, r.stderr
                    if rep >= 0:
                        runs[mode].append(dict(wall_s=wall, log=[x for x in r.stderr.splitlines() if "elapsed" in x or "two-pass:" in x]))
            out = dict(files=len(files), bytes=sum(os.path.getsize(f) for f in files))
            for mode in ("one", "two"):
                w = [x["wall_s"] for x in runs[mode]]
                out[mode] = dict(wall_s=dict(median=med(w), min=min(w), max=max(w), spread=max(w) - min(w)), runs=runs[mode])
            out["two_over_one"] = out["two"]["wall_s"]["median"] / out["one"]["wall_s"]["median"]
            # the scatter alone: HIP-event time of the kernels of all scatter calls, beside the index stage of one-pass (uploads, its
            # scatter launches, read-back and file writes together: what the lists cost after the sketch there)
            sc = [re.search(r"(\d+) keys scattered in ([0-9.]+) ms \((\d+) launch", "\n".join(x["log"])) for x in runs["two"]]
            ms = [float(m.group(2)) for m in sc]
            keys = int(sc[0].group(1))
            out["scatter"] = dict(keys=keys, launches=int(sc[0].group(3)), ms=dict(median=med(ms), min=min(ms), max=max(ms), spread=max(ms) - min(ms)),
                                  keys_per_s=keys / (med(ms) / 1e3), atomic_bytes_per_s=4 * keys / (med(ms) / 1e3))
            ix = [float(re.search(r"index ([0-9.]+) s", "\n".join(x["log"])).group(1)) for x in runs["one"]]
            out["one_pass_index_s"] = dict(median=med(ix), min=min(ix), max=max(ix), spread=max(ix) - min(ix), keys_per_s=keys / med(ix))
            one_r, two_r = os.path.join(dirs["one"], "R001"), os.path.join(dirs["two"], "R001")
            names = sorted(os.listdir(one_r))
            out["databases_equal"] = names == sorted(os.listdir(two_r)) and all(filecmp.cmp(os.path.join(one_r, f), os.path.join(two_r, f), shallow=False)
                                                                                for f in names if f != "__db.yml")
            res["inputs"][form] = out
        from kmcp_amd import Database
        with Database.open(os.path.join(dirs["two"], "R001"), device=0) as db:
            probes = [db.stream_probe() for _ in range(4)][1:]
        pm = med([p[0] for p in probes])
        res["stream_probe"] = dict(ms=pm, bytes=probes[0][1], bytes_per_s=probes[0][1] / (pm / 1e3))
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_makedb(genomes, spec):
    exe = os.path.join(ROOT, "kmcp_amd", "kmcp-makedb")
    tmp = tempfile.mkdtemp(prefix="bench_makedb_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        files = []
        for i, g in enumerate(genomes):
            p = os.path.join(tmp, f"g{i:05d}.fa.gz")
            with gzip.open(p, "wb", compresslevel=1) as fh:
                fh.write(b">g%d chromosome\n" % i)
                fh.write(b"\n".join(g[j:j + 80] for j in range(0, len(g), 80)) + b"\n")
            files.append(p)
        lst = os.path.join(tmp, "files.txt")
        with open(lst, "w") as fh:
            fh.write("\n".join(files) + "\n")
        cmd = [exe, "-k", str(K), "-n", str(SPLIT), "-l", str(OVERLAP), "--num-hash", "1", "-f", "0.3", "-j", "16", "-O", os.path.join(tmp, "db.kmcp"), "-i", lst]
        if spec["scale"] > 1:
            cmd += ["-D", str(spec["scale"])]
        runs = []
        for _ in range(2):  # the second run has the files and the binary in the page cache
            t0 = time.perf_counter()
            r = subprocess.run(cmd + ["--force"], capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr
            line = [x for x in r.stderr.splitlines() if "elapsed" in x]
            runs.append(dict(wall_s=wall, log=line[-1] if line else ""))
        return dict(files=len(files), gz_bytes=sum(os.path.getsize(f) for f in files), runs=runs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="a,b,c")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--genomes", type=int, default=0, help="fewer genomes than the shape's (quick look)")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--makedb", action="store_true")
    ap.add_argument("--two-pass", action="store_true", help="with --makedb: kmcp-makedb --two-pass against one-pass, nothing else")
    ap.add_argument("--matrix-budget", default="", help="passed to kmcp-makedb --two-pass (several rounds)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from kmcp_amd import lib
    out = []
    for name in args.shape.split(","):
        r = run_two_pass(name, SHAPES[name], args, lib) if (args.makedb and args.two_pass) else run_shape(name, SHAPES[name], args, lib)
        print(json.dumps(r), flush=True)
        out.append(r)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/bench_makedb.py", shapes=out), fh, indent=1)


if __name__ == "__main__":
    main()
