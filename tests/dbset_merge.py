"""The oracle of database sets: what kmcp-merge (cli/kmcp_merge.cpp) makes of the members' separate results, restated on result records.
A query's rows from all members in member order, each member's in its own row order, stable-sorted by the PRINTED score ("%.4f", parsed
back) descending; `hits` is the number of rows.  Python's "%.4f" rounds the double's exact value half to even, as glibc's does."""
import numpy as np

SCORE = ("qcov", "tcov", "jacc")


def merge_members(results, bases, sort_by, n_reads, records=False):
    """results[m].read(i) = the MATCH_DTYPE records of read i on member m alone -> per read an int64 array [rows, 2] of (global column, mKmers)
    in merged order, and statistics: rows, reads with rows of two or more members, reads with a run of equal printed score that spans members.
    records=True: per read the merged records themselves (global columns) instead of the pairs."""
    out, rows, multi, tied = [], 0, 0, 0
    for i in range(n_reads):
        parts = []
        for m, res in enumerate(results):
            x = res.read(i).copy()
            x["col"] += np.uint32(bases[m])
            parts.append(x)
        recs = np.concatenate(parts)
        member = np.concatenate([np.full(len(x), m) for m, x in enumerate(parts)])
        printed = np.array([float("%.4f" % v) for v in recs[SCORE[sort_by]]])
        order = np.argsort(-printed, kind="stable")
        recs, member, printed = recs[order], member[order], printed[order]
        out.append(recs if records else np.stack([recs["col"].astype(np.int64), recs["mkmers"].astype(np.int64)], axis=1).reshape(-1, 2))
        rows += len(recs)
        multi += len(set(member.tolist())) > 1
        tied += bool(((printed[1:] == printed[:-1]) & (member[1:] != member[:-1])).any())
    return out, dict(rows=rows, multi=multi, tied=tied)


def pairs_of(res, i):
    """read i of a BatchResult (records) or PairsResult (pairs) as an int64 array [rows, 2] of (column, mKmers)"""
    x = res.read(i)
    if x.dtype.names and "mkmers" in x.dtype.names:
        return np.stack([x["col"].astype(np.int64), x["mkmers"].astype(np.int64)], axis=1).reshape(-1, 2)
    if x.dtype.names:
        return np.stack([x["col"].astype(np.int64), x["count"].astype(np.int64)], axis=1).reshape(-1, 2)
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def assert_equal(got_res, want, what=""):
    for i, w in enumerate(want):
        g = pairs_of(got_res, i)
        assert g.shape == w.shape and (g == w).all(), (what, i, g.tolist()[:12], w.tolist()[:12])
