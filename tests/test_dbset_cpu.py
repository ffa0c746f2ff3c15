"""Database sets without a GPU: kmcpg_open_set on metadata-only handles (the union of the members' columns, kmcpg_set_info, the agreement
rule and its messages, the member limits), the host half's merge order on a set handle (kmcpg_finalize / kmcpg_finalize_grouped against
the merge of the members' own results, tests/dbset_merge.py), the parameters a set refuses, and the flags kmcp-search refuses next to
--also-db before it opens anything."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.dbset_merge import assert_equal, merge_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
EUNSUPPORTED, EINVAL = -6, -1


@pytest.fixture(scope="module")
def dbs(oracle_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dbset")
    genomes = synth.random_genomes(7, 6000, seed=90)
    a = synth.make_db(tmp / "a", genomes[:4], k=21, n_chunks=2, threads=4, names=[f"a{i}" for i in range(4)])
    b = synth.make_db(tmp / "b", genomes[4:], k=21, n_chunks=2, threads=4, names=[f"b{i}" for i in range(3)])
    return dict(tmp=tmp, genomes=genomes, a=a, b=b)


def test_union_of_the_members(dbs):
    from kmcp_amd import Database
    with Database.open(dbs["a"], device=-1) as A, Database.open(dbs["b"], device=-1) as B, Database.open_set([dbs["a"], dbs["b"]], device=-1) as S:
        na, nb = int(A.info.n_cols), int(B.info.n_cols)
        assert (na, nb) == (8, 6)
        assert int(S.info.n_cols) == na + nb and S.info.n_blocks == A.info.n_blocks + B.info.n_blocks
        assert S.info.matrix_bytes == A.info.matrix_bytes + B.info.matrix_bytes
        assert S.set_info() == [0, na] and A.set_info() == [0]
        assert [S.col_info(c) for c in range(na)] == [A.col_info(c) for c in range(na)]
        assert [S.col_info(na + c) for c in range(nb)] == [B.col_info(c) for c in range(nb)]
        # the blocks of B follow those of A, their column bases moved up by A's columns
        for blk in range(B.info.n_blocks):
            want = B.block_info(blk)
            got = S.block_info(A.info.n_blocks + blk)
            assert got["col_base"] == want["col_base"] + na and (got["num_sigs"], got["n_cols"], got["row_bytes"]) == (want["num_sigs"], want["n_cols"], want["row_bytes"])
        assert S.ks == [21]


def test_one_member_is_kmcpg_open(dbs):
    from kmcp_amd import Database, lib
    with Database.open(dbs["a"], device=-1) as A, Database.open_set([dbs["a"]], device=-1) as S:
        assert bytes(S.info) == bytes(A.info)
        assert S.set_info() == [0] and S.ks == A.ks
        with pytest.raises(lib.KmcpGpuError, match="not a database set"):
            S.last_set_order()


def test_member_limits(dbs):
    from kmcp_amd import Database, lib
    for dirs in ([], [dbs["a"]] * 17):
        with pytest.raises(lib.KmcpGpuError) as e:
            Database.open_set(dirs, device=-1)
        assert e.value.code == EINVAL and "1 to 16 members" in str(e.value)
    with Database.open_set([dbs["a"], dbs["b"]] * 8, device=-1) as S:  # sixteen is allowed
        assert len(S.set_info()) == 16 and int(S.info.n_cols) == 8 * 14


@pytest.mark.parametrize("field,kw", [("k ", dict(k=31)), ("scale", dict(scale=4)), ("numHashes", dict(num_hashes=2)), ("fpr", dict(fpr=0.2)),
                                      ("syncmer_s", dict(syncmer_s=9)), ("minimizer_w", dict(minimizer_w=5))])
def test_members_must_agree(dbs, field, kw):
    from kmcp_amd import Database, lib
    other = synth.make_db(dbs["tmp"] / ("other_" + field.strip()), dbs["genomes"][:2], n_chunks=1, threads=2, **dict(dict(k=21), **kw))
    for dirs in ([dbs["a"], other], [other, dbs["a"]], [dbs["a"], dbs["b"], other]):
        with pytest.raises(lib.KmcpGpuError) as e:
            Database.open_set(dirs, device=-1)
        assert e.value.code == EUNSUPPORTED
        msg = str(e.value)
        assert "disagree in " + field in msg and dirs[0] in msg and other in msg, msg


def test_a_member_with_two_k_mer_sizes_is_refused(dbs):
    from kmcp_amd import Database, lib
    two = str(dbs["tmp"] / "two_k")
    shutil.copytree(dbs["b"], two)
    yml = open(two + "/__db.yml").read()
    yml2 = re.sub(r"ks:\n- 21\n", "ks:\n- 11\n- 21\n", yml)  # (the headers carry the largest k, util-db-search.go:690: still 21)
    assert yml2 != yml
    open(two + "/__db.yml", "w").write(yml2)
    with Database.open(two, device=-1) as T:
        assert T.ks == [21, 11]
    for dirs in ([dbs["a"], two], [two, dbs["a"]]):
        with pytest.raises(lib.KmcpGpuError) as e:
            Database.open_set(dirs, device=-1)
        assert e.value.code == EUNSUPPORTED and "disagree in k " in str(e.value) and "11,21" in str(e.value) and two in str(e.value)
    with Database.open_set([two], device=-1) as T:  # one member: kmcpg_open, several k-mer sizes and all
        assert T.ks == [21, 11]


def _random_hits(rng, n_reads, n_cols, qk):
    from kmcp_amd import lib
    reads, cols, counts = [], [], []
    for r in range(n_reads):
        m = int(rng.integers(0, n_cols + 1))
        c = rng.permutation(n_cols)[:m]
        k = int(qk[r]) - rng.integers(0, 4, size=m)  # few distinct counts: printed scores tie within and across members
        reads.append(np.full(m, r, np.uint32)); cols.append(c.astype(np.uint32)); counts.append(k.astype(np.uint32))
    hits = np.empty(sum(len(x) for x in cols), dtype=lib.HIT_DTYPE)
    hits["read"], hits["col"], hits["count"] = np.concatenate(reads), np.concatenate(cols), np.concatenate(counts)
    return hits[rng.permutation(len(hits))]


@pytest.mark.parametrize("sort_by", [0, 1, 2], ids=["qcov", "tcov", "jacc"])
def test_host_half_orders_a_set_as_kmcp_merge(dbs, sort_by):
    """kmcpg_finalize and kmcpg_finalize_grouped on a set handle against the merge of the members' own kmcpg_finalize results"""
    from kmcp_amd import Database, default_params
    rng = np.random.default_rng(91 + sort_by)
    members = [dbs["a"], dbs["b"], dbs["a"]]  # the third repeats the first: every score of A ties with its twin across members
    n_reads = 120
    qk = rng.integers(11000, 13000, size=n_reads).astype(np.int32)  # > 10 000 k-mers: neighbouring counts print equal qCov
    ql = (qk + 20).astype(np.int32)
    p = default_params(min_qcov=0.0, min_matched=1, max_fpr=1.0, sort_by=sort_by)
    with Database.open_set(members, device=-1) as S:
        bases = S.set_info()
        n_cols = int(S.info.n_cols)
        hits = _random_hits(rng, n_reads, n_cols, qk)
        separate = []
        for m, d in enumerate(members):
            hi = bases[m + 1] if m + 1 < len(bases) else n_cols
            sel = hits[(hits["col"] >= bases[m]) & (hits["col"] < hi)].copy()
            sel["col"] -= bases[m]
            with Database.open(d, device=-1) as M:
                separate.append(M.finalize(sel, qk, ql, params=p))
        want, stats = merge_members(separate, bases, sort_by, n_reads)
        # (a read names half of the 22 columns on average, so most reads hold a column of A together with its twin: an exact tie across members)
        assert stats["rows"] == len(hits) and stats["tied"] >= n_reads // 2, stats
        assert_equal(S.finalize(hits, qk, ql, params=p), want, "kmcpg_finalize")
        # grouped by read but in no order inside a read: kmcpg_finalize_grouped finds that out and orders the segment itself
        order = np.argsort(hits["read"], kind="stable")
        pairs = np.ascontiguousarray(np.stack([hits["col"][order], hits["count"][order]], axis=1).astype(np.uint32))
        offs = np.zeros(n_reads + 2, dtype=np.uint64)
        offs[1:n_reads + 1] = np.cumsum(np.bincount(hits["read"], minlength=n_reads))
        assert_equal(S.finalize_grouped(pairs, offs, qk, ql, params=p), want, "kmcpg_finalize_grouped, unordered segments")
        # ... and takes a list that IS in the merge order as it stands
        in_order = np.concatenate([w for w in want if len(w)]).astype(np.uint32)
        assert_equal(S.finalize_grouped(np.ascontiguousarray(in_order), offs, qk, ql, params=p), want, "kmcpg_finalize_grouped, ordered segments")
        w = S.last_set_order()
        assert w["host_segments"] > 0 and w["host_mixed_runs"] > 0 and w["wave_segments"] == w["wg_segments"] == w["device_mixed_runs"] == 0, w


@pytest.mark.parametrize("kw,what", [(dict(try_se=1), "try_se"), (dict(do_not_sort=1), "do_not_sort"), (dict(top_n_scores=1), "top_n_scores"), (dict(k=21), "params->k")])
def test_a_set_refuses_what_acts_per_member(dbs, kw, what):
    from kmcp_amd import Database, default_params, lib
    hits = np.zeros(1, dtype=lib.HIT_DTYPE)
    hits["count"] = 100
    qk, ql = np.array([120], np.int32), np.array([140], np.int32)
    with Database.open_set([dbs["a"], dbs["b"]], device=-1) as S, Database.open_set([dbs["a"]], device=-1) as one:
        with pytest.raises(lib.KmcpGpuError) as e:
            S.finalize(hits, qk, ql, params=default_params(**kw))
        assert e.value.code == EUNSUPPORTED and what in str(e.value)
        with pytest.raises(lib.KmcpGpuError) as e:
            S.finalize_grouped(np.array([[0, 100]], np.uint32), np.array([0, 1, 0], np.uint64), qk, ql, params=default_params(**kw))
        assert e.value.code == EUNSUPPORTED and what in str(e.value)
        assert len(one.finalize(hits, qk, ql, params=default_params(**kw)).read(0)) == 1  # one member: an ordinary handle


REFUSED = [(["-K"], "-K"), (["--try-se"], "--try-se"), (["-S"], "-S"), (["-n", "1"], "-n"), (["--keep-top-scores", "3"], "--keep-top-scores"), (["-g"], "-g"),
           (["-G"], "-G"), (["--sliding-step", "50", "--sliding-window", "100"], "--sliding-"), (["--sliding-step", "50", "--sliding-window", "100", "--sliding-greedy"], "--sliding-"),
           (["--gpus", "2"], "--gpus"), (["--gpu-passes", "2"], "--gpu-passes")]


@pytest.mark.parametrize("flags,named", REFUSED, ids=[" ".join(f) for f, _ in REFUSED])
def test_cli_refuses_flags_next_to_also_db(dbs, tmp_path, flags, named):
    fq = str(tmp_path / "r.fq")
    with open(fq, "w") as fh:
        fh.write("@r0\n" + dbs["genomes"][0][:150].decode() + "\n+\n" + "I" * 150 + "\n")
    out = str(tmp_path / "out.tsv")
    r = subprocess.run([CLI, "-d", os.path.dirname(dbs["a"]), "--also-db", os.path.dirname(dbs["b"]), fq, "-o", out] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert named in r.stderr and "--also-db" in r.stderr, r.stderr
    assert not os.path.exists(out)
