"""kmcp-makedb (genome files -> database: `kmcp compute` + `kmcp index` on the GPU) on the reference's 15 demo genomes
(tests/golden/demo_profiling_refs_300k.fa.gz, one .fa.gz per accession): the .uniki files are the oracle's byte for byte — O.build_db over
tests/test_gpu_config0.py compute_columns —, __db.yml carries the same values, __name_mapping.tsv is the same file, and kmcp-search over
the new database prints the oracle's TSV.  The same for a FracMinHash (-D 10) and a closed-syncmer (-S 11) sketch, for an -i list and
-I/-r, and --force / the refusal to overwrite as makeOutDir has them (kmcp/cmd/util.go:92-113)."""
import filecmp
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_build import _yml
from tests.test_gpu_cli import compare, oracle_tsv, run_cli, write_fastq
from tests.test_gpu_config0 import K, OVERLAP, SPLIT, compute_columns, load_genomes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEDB = os.path.join(ROOT, "kmcp_amd", "kmcp-makedb")
YML_KEYS = ("version", "unikiVersion", "k", "ks", "hashed", "canonical", "scaled", "scale", "minimizer", "minimizer-w", "syncmer", "syncmer-s",
            "hashes", "numNameGroups", "blocksize", "totalKmers")
FLAGS = ["-k", str(K), "-n", str(SPLIT), "-l", str(OVERLAP), "-B", "plasmid", "--num-hash", "1", "-f", "0.3", "-j", "16"]


@pytest.fixture(scope="module")
def demo(oracle_lib, tmp_path_factory):
    O = oracle_lib
    tmp = tmp_path_factory.mktemp("makedb")
    genomes = load_genomes()
    assert len(genomes) == 15
    refs = tmp / "refs"
    refs.mkdir()
    files = []
    for acc in sorted(genomes):
        path = str(refs / (acc + ".fa.gz"))
        with gzip.open(path, "wt") as fh:
            for name, s in genomes[acc]:
                fh.write(">%s\n" % name)
                s = s.decode()
                for i in range(0, len(s), 80):
                    fh.write(s[i:i + 80] + "\n")
        files.append(path)
    cols, big = compute_columns(O, genomes)
    rng = np.random.default_rng(9)
    accs = sorted(big)
    reads = []
    for _ in range(2000):
        g = big[accs[int(rng.integers(0, len(accs)))]]
        p = int(rng.integers(0, len(g) - 150))
        reads.append(g[p:p + 150])
    reads += synth.random_genomes(100, 150, seed=10)
    return dict(tmp=tmp, files=files, refs=str(refs), cols=cols, big=big, reads=reads)


def makedb(args, expect=0):
    r = subprocess.run([MAKEDB] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == expect, (r.returncode, r.stderr)
    return r


def assert_same_db(got, ref):
    yr, yg = _yml(os.path.join(ref, "__db.yml")), _yml(os.path.join(got, "__db.yml"))
    assert yr["files"] == yg["files"] and len(yr["files"]) >= 1
    for key in YML_KEYS:
        assert yr[key] == yg[key], key
    assert float(yr["fpr"]) == float(yg["fpr"])
    for f in yr["files"]:
        assert filecmp.cmp(os.path.join(ref, f), os.path.join(got, f), shallow=False), f
    assert open(os.path.join(ref, "__name_mapping.tsv")).read() == open(os.path.join(got, "__name_mapping.tsv")).read()
    assert sorted(os.listdir(got)) == sorted(os.listdir(ref))


def assert_same_search(O, demo, got, ref, out_name, min_rows=1500):
    ids = [f"r{i}" for i in range(len(demo["reads"]))]
    fq = str(demo["tmp"] / "reads.fq")
    if not os.path.exists(fq):
        write_fastq(fq, ids, demo["reads"])
    odb = O.OracleDB(ref)
    try:
        want, trailer = oracle_tsv(O, odb, ids, demo["reads"])
        assert len(want) > min_rows
        compare(run_cli(["-d", os.path.dirname(got), fq], str(demo["tmp"] / out_name)), want, trailer)
    finally:
        odb.close()


def test_makedb_writes_the_oracles_database(demo, oracle_lib):
    O = oracle_lib
    tmp = demo["tmp"]
    ref = O.build_db(str(tmp / "oracle.kmcp"), O.sketch_cfg(k=K), demo["cols"], num_hashes=1, fpr=0.3, threads=16)
    out = str(tmp / "gpu.kmcp")
    r = makedb(FLAGS + ["-O", out] + demo["files"])
    assert "150 column(s)" in r.stderr
    got = os.path.join(out, "R001")
    assert len([f for f in os.listdir(got) if f.endswith(".uniki")]) == 10
    assert_same_db(got, ref)
    assert_same_search(O, demo, got, ref, "plain.tsv")
    # the same database from an -i list and from -I / -r; small batches: several sketch calls, one fills while the other runs
    lst = tmp / "files.txt"
    lst.write_text("\n".join(demo["files"]) + "\n")
    out_i = str(tmp / "gpu_i.kmcp")
    makedb(FLAGS + ["-O", out_i, "-i", str(lst), "--batch-bases", "700000"])
    assert_same_db(os.path.join(out_i, "R001"), ref)
    out_d = str(tmp / "gpu_d.kmcp")
    (tmp / "refs" / "notes.txt").write_text("not a genome\n")
    makedb(FLAGS + ["-O", out_d, "-I", demo["refs"], "-r", r"\.fa\.gz$"])
    assert_same_db(os.path.join(out_d, "R001"), ref)
    # refusal to overwrite, and --force (makeOutDir)
    r = makedb(FLAGS + ["-O", out] + demo["files"][:2], expect=255)
    assert "out-dir not empty" in r.stderr and "--force" in r.stderr
    assert_same_db(got, ref)  # untouched
    makedb(FLAGS + ["-O", out, "--force"] + demo["files"][:2])
    assert len(_yml(os.path.join(got, "__db.yml"))["files"]) >= 1
    names = {line.split("\t")[0] for line in open(os.path.join(got, "__name_mapping.tsv"))}
    assert len(names) == 2


@pytest.mark.parametrize("flag, kw", [(["-D", "10"], dict(scale=10)), (["-S", "11"], dict(syncmer_s=11))])
def test_makedb_sketch_modes(demo, oracle_lib, flag, kw):
    O = oracle_lib
    tmp = demo["tmp"]
    tag = flag[0].strip("-")
    cfg = O.sketch_cfg(k=K, **kw)
    accs = sorted(demo["big"])
    cols = synth.make_columns([demo["big"][a] for a in accs], cfg, n_chunks=SPLIT, overlap=OVERLAP, names=accs)
    ref = O.build_db(str(tmp / f"oracle_{tag}.kmcp"), cfg, cols, num_hashes=1, fpr=0.3, threads=16)
    out = str(tmp / f"gpu_{tag}.kmcp")
    makedb(FLAGS + flag + ["-O", out] + demo["files"])
    assert_same_db(os.path.join(out, "R001"), ref)
    assert_same_search(O, demo, os.path.join(out, "R001"), ref, f"{tag}.tsv", min_rows=500)
