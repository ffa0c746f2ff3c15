"""kmcp-makedb --two-pass on the reference's 15 demo genomes (the fixtures and helpers of tests/test_gpu_makedb.py): the database is
the oracle's byte for byte and searches like it — in one round, in several sketch batches, in several rounds under a --matrix-budget
that holds three blocks (the log must show the files read again per round, later rounds only a subset), for a FracMinHash and a
closed-syncmer sketch; a budget below the largest block is refused with the block, its bytes and the budget; and a genome that changes
between the passes is caught by the library (the column and both counts named) with no __db.yml written."""
import os
import re

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_makedb import FLAGS, assert_same_db, assert_same_search, demo, makedb  # noqa: F401  (demo: the module's fixture)
from tests.test_gpu_config0 import K, OVERLAP, SPLIT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(demo, oracle_lib):  # noqa: F811
    O = oracle_lib
    ref = O.build_db(str(demo["tmp"] / "oracle2.kmcp"), O.sketch_cfg(k=K), demo["cols"], num_hashes=1, fpr=0.3, threads=16)
    odb = O.OracleDB(ref)
    try:
        matrix_bytes = [odb.block_info(b)[0] * odb.block_info(b)[2] for b in range(odb.nblocks)]
    finally:
        odb.close()
    assert len(matrix_bytes) == 10
    return ref, matrix_bytes


def rounds_log(stderr):
    """[(round, rounds, files read, files)] of the "round i of n: x of y file(s) read" lines"""
    return [tuple(int(v) for v in m) for m in re.findall(r"round (\d+) of (\d+): (\d+) of (\d+) file\(s\) read", stderr)]


def test_two_pass_writes_the_oracles_database(demo, oracle_lib, reference):  # noqa: F811
    ref, _ = reference
    out = str(demo["tmp"] / "two.kmcp")
    r = makedb(FLAGS + ["--two-pass", "-O", out] + demo["files"])
    assert "150 column(s)" in r.stderr and "no k-mer list was held in host memory" in r.stderr
    assert rounds_log(r.stderr) == [(1, 1, 15, 15)]
    assert "10 block(s) in 1 round(s); files read: pass 1 15, pass 2 15" in r.stderr
    keys = int(re.search(r"(\d+) keys scattered in [0-9.]+ ms \((\d+) launch", r.stderr).group(1))
    assert keys == sum(len(c[4]) for c in demo["cols"])
    got = os.path.join(out, "R001")
    assert_same_db(got, ref)
    assert_same_search(oracle_lib, demo, got, ref, "two_pass.tsv")


def test_two_pass_in_several_batches(demo, reference):  # noqa: F811
    ref, _ = reference
    out = str(demo["tmp"] / "two_batches.kmcp")
    r = makedb(FLAGS + ["--two-pass", "--batch-bases", "700000", "-O", out] + demo["files"])
    launches = int(re.search(r"keys scattered in [0-9.]+ ms \((\d+) launch", r.stderr).group(1))
    assert launches >= 5  # one per batch (one piece each): 4.5 Mbp in batches of at most 0.7 Mbp
    assert_same_db(os.path.join(out, "R001"), ref)


def test_two_pass_in_several_rounds(demo, oracle_lib, reference):  # noqa: F811
    ref, mb = reference
    # no four consecutive blocks fit, three of the larger ones do: at least four rounds
    budget = min(sum(m + 8 for m in mb[i:i + 4]) for i in range(len(mb) - 3)) - 1
    assert budget >= 3 * (max(mb) + 8)
    out = str(demo["tmp"] / "two_rounds.kmcp")
    r = makedb(FLAGS + ["--two-pass", "--matrix-budget", str(budget), "-O", out] + demo["files"])
    log = rounds_log(r.stderr)
    n_rounds = len(log)
    assert n_rounds >= 4 and [x[0] for x in log] == list(range(1, n_rounds + 1)) and all(x[1] == n_rounds and x[3] == 15 for x in log)
    assert sum(x[2] for x in log) > 15          # files were read again, round by round
    assert any(x[2] < 15 for x in log[1:])      # and a later round read only the files it has columns of
    assert "in %d round(s); files read: pass 1 15, pass 2 %d" % (n_rounds, sum(x[2] for x in log)) in r.stderr
    peak = int(re.search(r"peak matrix bytes (\d+)", r.stderr).group(1))
    assert max(mb) + 8 <= peak <= budget
    got = os.path.join(out, "R001")
    assert_same_db(got, ref)
    assert_same_search(oracle_lib, demo, got, ref, "two_rounds.tsv")
    # k/M/G suffixes as the other size flags parse them
    out_k = str(demo["tmp"] / "two_rounds_k.kmcp")
    r = makedb(FLAGS + ["--two-pass", "--matrix-budget", "%dK" % (budget // 1024), "-O", out_k] + demo["files"])
    assert len(rounds_log(r.stderr)) >= 4
    assert_same_db(os.path.join(out_k, "R001"), ref)


@pytest.mark.parametrize("flag, kw", [(["-D", "10"], dict(scale=10)), (["-S", "11"], dict(syncmer_s=11))])
def test_two_pass_sketch_modes(demo, oracle_lib, flag, kw):  # noqa: F811
    O = oracle_lib
    tmp = demo["tmp"]
    tag = flag[0].strip("-")
    cfg = O.sketch_cfg(k=K, **kw)
    accs = sorted(demo["big"])
    cols = synth.make_columns([demo["big"][a] for a in accs], cfg, n_chunks=SPLIT, overlap=OVERLAP, names=accs)
    ref = O.build_db(str(tmp / f"oracle2_{tag}.kmcp"), cfg, cols, num_hashes=1, fpr=0.3, threads=16)
    out = str(tmp / f"two_{tag}.kmcp")
    makedb(FLAGS + flag + ["--two-pass", "-O", out] + demo["files"])
    assert_same_db(os.path.join(out, "R001"), ref)
    assert_same_search(O, demo, os.path.join(out, "R001"), ref, f"two_{tag}.tsv", min_rows=500)


def test_budget_below_the_largest_block(demo, reference):  # noqa: F811
    _, mb = reference
    big = mb.index(max(mb))
    budget = max(mb) + 7
    out = str(demo["tmp"] / "two_small.kmcp")
    r = makedb(FLAGS + ["--two-pass", "--matrix-budget", str(budget), "-O", out] + demo["files"], expect=255)
    assert "block %d " % (big + 1) in r.stderr and str(max(mb) + 8) in r.stderr and str(budget) in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(out, "R001", "__db.yml"))


def test_a_genome_that_changes_between_the_passes(tmp_path):
    """the library, driven as the command drives it: pass 1 on one set of genomes, pass 2 with one genome one base shorter"""
    from kmcp_amd import lib
    genomes = synth.random_genomes(12, 5000, seed=601)
    changed = list(genomes)
    changed[7] = changed[7][:-1]
    out = str(tmp_path / "db")
    with lib.Sketcher(k=21, device=0) as sk, lib.Builder(device=0, block_size=8) as b:
        counts = []
        sk.sketch_to(genomes, lambda p: counts.extend(np.diff(p["koff"]).tolist()))
        assert len(counts) == 12
        b.add_cols([("g%02d" % i, len(g), 0, 1, int(n)) for i, (g, n) in enumerate(zip(genomes, counts))])
        assert b.plan(1 << 30) == (2, 1)
        b.begin_round(0)

        def scatter(p):
            b.scatter_device(p["d_hashes"], p["koff"], p["genome"], p["stream"])  # one chunk per genome: the genome is the column

        with pytest.raises(lib.KmcpGpuError) as e:
            sk.sketch_to(changed, scatter)
        assert e.value.code == -1 and "column 7 (g07)" in str(e.value), str(e.value)
        assert "%d k-mers now, %d in pass 1" % (counts[7] - 1, counts[7]) in str(e.value)
        assert b.info()["scatter_launches"] == 0
        with pytest.raises(lib.KmcpGpuError):
            b.end_round(out)  # nothing was scattered: no block file with a column missing
        assert not os.path.exists(out)
        # the handle and the sketcher are usable: the unchanged genomes build the database
        sk.sketch_to(genomes, scatter)
        b.end_round(out)
        got = b.finish(out)
        assert b.info()["scatter_launches"] == 1 and b.info()["keys_scattered"] == sum(counts)
    with lib.Sketcher(k=21, device=0) as sk, sk.sketch(genomes) as s:
        cols = [("g%02d" % i, len(g), 0, 1, s.list(i).copy()) for i, g in enumerate(genomes)]
    one = lib.build_db(str(tmp_path / "one"), cols, block_size=8)
    from tests.test_gpu_builder import assert_same_files
    assert_same_files(got, one, whole=True)
