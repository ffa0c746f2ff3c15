"""bench.py --dump-outputs: what dump_outputs writes for a finalized batch - float64 .npy files, every query and match while they fit
the 64 MB limit, past it a seeded sample of whole queries that is the same from run to run."""
import os

import numpy as np

import bench
from kmcp_amd import lib


def _result(n, seed, max_matches=5):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, max_matches, n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(cnt)
    m = np.zeros(int(offs[-1]), dtype=lib.MATCH_DTYPE)
    m["col"] = rng.integers(0, 479232, len(m))
    m["target_idx"] = rng.integers(0, 1 << 20, len(m))
    m["gsize"] = rng.integers(1, 1 << 40, len(m))
    m["mkmers"] = rng.integers(1, 130, len(m))
    for f in ("qcov", "tcov", "jacc", "fpr"):
        m[f] = rng.random(len(m))
    qlen = rng.integers(100, 200, n).astype(np.int32)
    return lib.BatchResult(qlen, (qlen - 20).astype(np.int32), offs, m, 21), cnt


def _load(paths):
    return {os.path.basename(p)[:-len(".npy")]: np.load(p) for p in paths}


def test_dump_writes_every_query_and_match_exactly(tmp_path):
    res, cnt = _result(3000, seed=1)
    a = _load(bench.dump_outputs(str(tmp_path), res))
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["query_index"], np.arange(3000)) and np.array_equal(a["query_len"], res.qlen)
    assert np.array_equal(a["query_kmers"], res.qkmers)
    assert np.array_equal(a["match_query"], np.repeat(np.arange(3000), cnt))
    for f in ("col", "target_idx", "gsize", "mkmers", "qcov", "tcov", "jacc", "fpr"):
        assert np.array_equal(a["match_" + f], res.matches[f].astype(np.float64)), f
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in a)


def test_dump_past_the_limit_keeps_a_fixed_sample_of_whole_queries(tmp_path):
    res, cnt = _result(40000, seed=2)
    limit = 400_000
    paths = bench.dump_outputs(str(tmp_path / "a"), res, limit=limit)
    assert sum(os.path.getsize(p) for p in paths) <= limit
    a = _load(paths)
    sel = a["query_index"].astype(np.int64)
    assert 0 < len(sel) < 40000 and np.all(np.diff(sel) > 0)
    # every match of a sampled query, and nothing else
    want = np.concatenate([res.matches["col"][int(res.offs[i]):int(res.offs[i + 1])] for i in sel])
    assert np.array_equal(a["match_col"], want) and np.array_equal(a["match_query"], np.repeat(sel, cnt[sel]))
    # the same result dumps the same sample; the budget is used, not wasted
    b = _load(bench.dump_outputs(str(tmp_path / "b"), res, limit=limit))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(p) for p in paths) > 0.9 * limit


def test_dump_of_an_empty_batch(tmp_path):
    res, _ = _result(16, seed=3, max_matches=1)
    a = _load(bench.dump_outputs(str(tmp_path), res))
    assert len(a["query_index"]) == 16 and len(a["match_col"]) == 0
