"""Database sets on the GPU (kmcpg_open_set, kmcp-search --also-db): the result of every query is what kmcp-merge makes of the members'
separate results — the same columns, counts, order and `hits` (tests/dbset_merge.py restates the merge on records), the same Match bits
through kmcpg_expand_pairs, the same TSV bytes through the command line — for -s qcov / tcov / jacc, single and paired reads, with the
device ordering the segments and with the host doing it (KMCPG_DEVICE_FINALIZE=0), in every size class of the sort kernels and on the
sixteen members a set may have.  kmcpg_last_set_order shows which class ordered the segments and that the tie rule was at work."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import dbset_data, synth
from tests.dbset_merge import assert_equal, merge_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
MERGE = os.path.join(ROOT, "kmcp_amd", "kmcp-merge")
SORTS = ["qcov", "tcov", "jacc"]


@pytest.fixture(scope="module")
def data(oracle_lib, tmp_path_factory):
    return dbset_data.build(tmp_path_factory.mktemp("dbset_gpu"))


@pytest.fixture(scope="module")
def handles(data):
    """the three members on their own, the set, and the set with the host ordering every segment"""
    from kmcp_amd import Database
    members = [Database.open(d, device=0) for d in data["dirs"]]
    the_set = Database.open_set(data["dirs"], device=0)
    os.environ["KMCPG_DEVICE_FINALIZE"] = "0"  # (read when a handle's lanes are created, at its first search)
    try:
        host_set = Database.open_set(data["dirs"], device=0)
        host_set.search_pairs(data["reads"][:4])
    finally:
        del os.environ["KMCPG_DEVICE_FINALIZE"]
    yield dict(members=members, set=the_set, host_set=host_set)
    for h in members + [the_set, host_set]:
        h.close()


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("sort_by", [0, 1, 2], ids=SORTS)
def test_set_equals_the_merge_of_separate_searches(data, handles, sort_by, paired):
    from kmcp_amd import default_params
    p = default_params(sort_by=sort_by)
    reads, reads2 = data["reads"], data["reads2"] if paired else None
    n = len(reads)
    S = handles["set"]
    bases = S.set_info()
    separate = [M.search(reads, reads2, params=p) for M in handles["members"]]
    want, stats = merge_members(separate, bases, sort_by, n)
    # the data exercises what it is meant to (from the separate results alone)
    assert stats["rows"] >= 1500 and stats["multi"] >= 200 and stats["tied"] >= 50, stats
    got = S.search_pairs(reads, reads2, params=p)
    assert_equal(got, want, "set, pairs")
    assert (got.qkmers == separate[0].qkmers).all() and (got.qlen == separate[0].qlen).all()
    w = S.last_set_order()
    assert w["wave_segments"] > 0 and w["device_mixed_runs"] > 0 and w["host_segments"] == 0, w
    assert_equal(S.search(reads, reads2, params=p), want, "set, records")
    # the Match records of the pairs: the bits the members' own records have
    want_recs, _ = merge_members(separate, bases, sort_by, n, records=True)
    for i in range(n):
        if len(want_recs[i]):
            assert S.expand_pairs(int(got.qkmers[i]), got.read(i)).tobytes() == want_recs[i].tobytes(), i
    # the same with the host ordering every segment
    H = handles["host_set"]
    assert_equal(H.search_pairs(reads, reads2, params=p), want, "set, KMCPG_DEVICE_FINALIZE=0")
    wh = H.last_set_order()
    assert wh["host_segments"] > 0 and wh["host_mixed_runs"] > 0 and wh["wave_segments"] == wh["device_mixed_runs"] == 0, wh


def test_one_member_set_is_the_database(data, handles):
    from kmcp_amd import Database, default_params
    reads, reads2 = data["reads"], data["reads2"]
    with Database.open_set(data["dirs"][:1], device=0) as one:
        for p in (default_params(), default_params(sort_by=2, top_n_scores=1), default_params(do_not_sort=1)):
            for r2 in (None, reads2):
                a, b = handles["members"][0].search(reads, r2, params=p), one.search(reads, r2, params=p)
                assert a.matches.tobytes() == b.matches.tobytes() and (a.offs == b.offs).all() and (a.qkmers == b.qkmers).all()


def _against_merge(dirs, reads, p, sort_by=0):
    from kmcp_amd import Database
    separate = []
    for d in dirs:
        with Database.open(d, device=0) as M:
            separate.append(M.search(reads, params=p))
    with Database.open_set(dirs, device=0) as S:
        want, stats = merge_members(separate, S.set_info(), sort_by, len(reads))
        got = S.search_pairs(reads, params=p)
        assert_equal(got, want)
        assert_equal(S.search(reads, params=p), want)
        return S.last_set_order(), stats, [int(got.offs[i + 1] - got.offs[i]) for i in range(len(reads))]


def test_workgroup_class(oracle_lib, tmp_path):
    """300 columns of one 2 kb genome, the database twice in a set: 600 matches per read.  The columns end 0, 10 .. 40 bases early, so equal
    counts come with five column sizes: in the exact order the two members alternate inside a run of equal printed score"""
    from kmcp_amd import default_params
    g = synth.random_genomes(1, 2000, seed=310)[0]
    d = synth.make_db(tmp_path / "w", [g[:2000 - 10 * (i % 5)] for i in range(300)], k=21, n_chunks=1, threads=4, names=[f"w{i:03d}" for i in range(300)])
    reads = synth.sample_reads([g[:1900]], 64, 150, sub_rate=0.01, seed=311, frac_random=0.0)
    w, stats, per_read = _against_merge([d, d], reads, default_params())
    assert max(per_read) == 600 and stats["tied"] > 0
    assert w["wg_segments"] >= 1 and w["device_mixed_runs"] >= 1 and w["long_segments"] == 0 and w["host_segments"] == 0, w


def test_host_class(oracle_lib, tmp_path):
    """two members of 2 100 columns of one 1 kb sequence at -t 0.3: more than 4 096 matches per read, ordered by the host"""
    from kmcp_amd import default_params
    g = synth.random_genomes(1, 1000, seed=320)[0]
    cols = [g[:1000 - 10 * (i % 5)] for i in range(2100)]  # (five column sizes, as above)
    dirs = [synth.make_db(tmp_path / x, cols, k=21, n_chunks=1, threads=4, names=[f"{x}{i:04d}" for i in range(2100)]) for x in "hj"]
    reads = synth.sample_reads([g[:900]], 64, 150, sub_rate=0.01, seed=321, frac_random=0.0)
    w, stats, per_read = _against_merge(dirs, reads, default_params(min_qcov=0.3))
    assert max(per_read) == 4200 and stats["tied"] > 0
    assert w["long_segments"] >= 1 and w["host_segments"] >= 1 and w["host_mixed_runs"] >= 1, w


def test_sixteen_members(oracle_lib, tmp_path):
    """member i holds genomes i and i + 1 (mod 16): every genome lives in two members"""
    from kmcp_amd import default_params
    genomes = synth.random_genomes(16, 8000, seed=330)
    dirs = [synth.make_db(tmp_path / f"m{i:02d}", [genomes[i], genomes[(i + 1) % 16]], k=21, n_chunks=2, threads=4, names=[f"g{i:02d}", f"g{(i + 1) % 16:02d}"])
            for i in range(16)]
    reads = synth.sample_reads(genomes, 256, 150, sub_rate=0.01, seed=331, frac_random=0.1)
    for sort_by in (0, 2):
        w, stats, _ = _against_merge(dirs, reads, default_params(sort_by=sort_by), sort_by)
        assert stats["multi"] >= 100 and stats["tied"] >= 100, stats
        assert w["wave_segments"] >= 100 and w["device_mixed_runs"] >= 100, w


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (cmd, r.stderr)


def _text(path):
    if path.endswith(".gz"):
        with gzip.open(path, "rb") as fh:
            return fh.read()
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("extra,ext", [([], ".tsv"), (["-s", "tcov"], ".tsv"), (["-s", "jacc", "-H"], ".tsv"), ([], ".tsv.gz")], ids=["qcov", "tcov", "jacc-H", "gz"])
def test_cli_also_db_prints_what_kmcp_merge_prints(data, tmp_path, extra, ext):
    from tests.test_gpu_cli import write_fastq
    reads = data["reads"][:2000]
    fq = str(tmp_path / "reads.fq")
    write_fastq(fq, [f"read{i}" for i in range(len(reads))], reads)
    roots = [os.path.dirname(d) for d in data["dirs"]]
    singles = []
    for m, root in enumerate(roots):
        out = str(tmp_path / f"single{m}{ext}")
        _run([CLI, "-d", root, fq, "-o", out, "-q"] + extra)
        # (kmcp-merge counts an input without rows as one matched query, cli/kmcp_merge.cpp:13-14: not in play here)
        assert any(l and not l.startswith(b"#") for l in _text(out).split(b"\n")), out
        singles.append(out)
    merged, together = str(tmp_path / f"merged{ext}"), str(tmp_path / f"together{ext}")
    _run([MERGE, "-o", merged] + extra + singles)
    _run([CLI, "-d", roots[0], "--also-db", roots[1], "--also-db", roots[2], fq, "-o", together, "-q"] + extra)
    want, got = _text(merged), _text(together)
    assert got == want
    assert got.count(b"\n") > 1500


def test_cli_without_also_db_is_unchanged(oracle_lib, data, tmp_path):
    from tests.test_gpu_cli import compare, oracle_tsv, run_cli, write_fastq
    O = oracle_lib
    reads = data["reads"][:2000]
    ids = [f"read{i}" for i in range(len(reads))]
    fq = str(tmp_path / "reads.fq")
    write_fastq(fq, ids, reads)
    odb = O.OracleDB(data["dirs"][0])
    want, trailer = oracle_tsv(O, odb, ids, reads)
    odb.close()
    compare(run_cli(["-d", os.path.dirname(data["dirs"][0]), fq], str(tmp_path / "plain.tsv")), want, trailer)
