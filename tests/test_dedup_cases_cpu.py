"""The case table of the dedup stage (tests/dedup_cases.py) checked against its own restatement of the routing, without a GPU: what a
case declares — every query's class, the largest bucket of the queries built around one, the launch sequence, the fallback counts — is
what the restatement gives, the cases reach every class at both ends, and every case is inside the contract of kmcpg_dedup_device."""
import numpy as np
import pytest

from tests import dedup_cases as D

IDS = [c.id for c in D.CASES]


def test_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_declared_is_what_the_restatement_gives(case):
    assert [q.cls for q in case.queries] == [D.route(case, q) for q in case.queries]
    assert case.seq == D.tokens(case)
    assert tuple(case.fb) == D.fallbacks(case)
    for q in case.queries:
        name = q.cls.split(":")[0]
        if name in D.BUCKETS:
            got = D.largest_bucket(case, q, D.BUCKETS[name][1])
            assert (got > D.DB_MAXB) == q.cls.endswith(":fallback")
            if q.maxb is not None:
                assert got == q.maxb
        else:
            assert q.maxb is None


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_inside_the_contract(case):
    assert case.queries and case.max_n >= max(len(q.keys) for q in case.queries)
    assert case.mm >= 1 and case.u >= 0 and (case.pre or not case.pre_done)
    for q in case.queries:
        assert q.keys.dtype == D.U64 and q.keys.ndim == 1 and len(q.keys) >= 1
        if case.key_shift:
            assert int(q.keys.max()) <= D.MAX_HASH
    koff, offs, offs2, total = D.layout(case)
    n = np.array([len(q.keys) for q in case.queries])
    assert np.all(koff[1:] > koff[:-1] + n[:-1]) and koff[-1] + n[-1] < total  # a guard of at least one word behind every list
    assert np.array_equal(offs + (offs2 if case.paired else 0), koff) and np.all(offs >= 0)
    assert D.KEY_SHIFT == 9 and D.MAX_HASH & (D.MAX_HASH - 1)


def _entered(cls_prefix, knob=True, pre=0):
    """the numbers of elements to sort with which queries enter a class"""
    return {len(D.to_sort(c, q)) for c in D.CASES if c.big_bucket == knob and c.pre == pre for q in c.queries if q.cls.startswith(cls_prefix)}


def test_every_class_is_entered_at_both_ends():
    u = 4
    assert {c.u for c in D.CASES if c.id.startswith("wave")} == {u}
    wave = {len(q.keys) for c in D.CASES if c.u == u for q in c.queries if q.cls == "wave"}
    assert {u + 1, 8, 9, 63, 64, 65, 511, 512} <= wave
    assert {len(c.queries) for c in D.CASES if c.id.startswith("wave")} >= {1, 4, 5}
    assert any([q.cls for q in c.queries][i:i + 2] == ["keep", "wave"] and len(c.queries[i].keys) == c.u == len(c.queries[i + 1].keys) - 1
               for c in D.CASES for i in range(len(c.queries) - 1))
    assert {513, 2048} <= _entered("b2048") and {2049, 4096} <= _entered("b4096") and {4097, 16384} <= _entered("b16384")
    assert {16385, 20000, 65536} <= _entered("wg:global") and {4097, 10000, 16384} <= _entered("wg:lds", knob=False)
    assert not _entered("wg:lds", knob=True) and not _entered("b16384", knob=False)
    assert {2048} <= _entered("b2048", pre=1) and {2049} <= _entered("b4096", pre=1) and {1} <= _entered("b2048", pre=1)
    huge = {len(q.keys) for c in D.CASES for q in c.queries if q.cls == "huge"}
    assert {65537, 69632, 69633} <= huge
    # 65536 keys beside a huge query (n_hi == HUGE_MIN) and alone
    assert {c.max_n for c in D.CASES for q in c.queries if q.cls == "wg:global" and len(q.keys) == D.HUGE_MIN} == {65536, 65537}
    # 24 against 25 in every instantiation, both paths in both orders of a stride
    for name, (cap, nb, nt, grid) in D.BUCKETS.items():
        assert {24, 25} <= {q.maxb for c in D.CASES for q in c.queries if q.cls.startswith(name)}
        orders = {(c.queries[0].cls, c.queries[-1].cls) for c in D.CASES if len(c.queries) == grid + 1}
        assert orders == {(name + ":fallback", name + ":buckets"), (name + ":buckets", name + ":fallback")}
        strides = [c for c in D.CASES if len(c.queries) == grid + 1]
        assert all(q.cls == "keep" and len(q.keys) == 1 for c in strides for q in c.queries[1:-1])
    assert {(c.queries[0].cls, c.queries[-1].cls) for c in D.CASES if len(c.queries) == 1025} == {("wg:lds", "wg:global"), ("wg:global", "wg:lds")}


def test_pre_done_cases_follow_the_fused_kernel():
    """what the test writes for a pre_done case — the shortened list to scratch, its length to nk_search — is written for the queries
    with a raw count in (max(u, 512), 65536] only and is what k_adj_unique makes of the pre case of the same queries"""
    done = [c for c in D.CASES if c.pre_done]
    assert done
    for c in done:
        twin = [d for d in D.CASES if d.pre and not d.pre_done and len(d.queries) == len(c.queries) and all(x.keys is y.keys for x, y in zip(d.queries, c.queries))]
        assert twin and "adj" in twin[0].seq and "adj" not in c.seq and [t for t in twin[0].seq if t != "adj"] == c.seq
        pre = D.pre_done_state(c)
        for q, (m, lst) in zip(c.queries, pre):
            n = len(q.keys)
            if max(c.u, D.WAVE_CAP) < n <= D.HUGE_MIN:
                assert m == len(lst) == len(D.adj_unique(q.keys)) and np.array_equal(lst, D.adj_unique(q.keys))
                assert np.array_equal(np.unique(lst), np.unique(q.keys))
            else:
                assert m is None and lst is None
    # runs across the lane and tile seams of k_adj_unique, and a repeat that only the sort removes
    k = next(q.keys for c in done for q in c.queries if len(q.keys) == 1500)
    for s in (64, 512, 1024):
        assert k[s - 1] == k[s]
    assert any(len(np.unique(q.keys)) < len(D.adj_unique(q.keys)) for c in done for q in c.queries)
    ms = {(len(q.keys), len(D.adj_unique(q.keys))) for c in done for q in c.queries}
    assert {(20000, 1500), (3000, 1), (5000, 2048), (5000, 2049)} <= ms


def test_special_keys_and_seams():
    by = {c.id: c for c in D.CASES}
    waves = [q.keys for c in D.CASES for q in c.queries if q.cls == "wave"]
    for v in (0, int(D.ALL_ONES)):
        assert any(np.count_nonzero(k == v) == 1 for k in waves) and any(1 < np.count_nonzero(k == v) < len(k) for k in waves)
    s = [np.sort(k) for k in waves]
    assert any(len(k) > 8 and k[7] == k[8] and k[6] != k[7] and k[8] != k[9] for k in s)
    assert any(len(k) > 256 and k[255] == k[256] and k[254] != k[255] and k[256] != k[257] for k in s)
    assert any(np.all(k[1:] > k[:-1]) for k in waves) and any(np.all(k[1:] < k[:-1]) for k in waves) and any(len(np.unique(k)) == 1 for k in waves)
    shift = by["bucket-key-shift"]
    assert all(np.count_nonzero(q.keys == D.MAX_HASH) == 3 and np.count_nonzero(q.keys == 0) == 3 for q in shift.queries[:3])
    for b in range(8):
        k = by["huge-byte-%d" % b].queries[0].keys
        x = k ^ k[0]
        assert np.all(x & ~(D.U64(255) << D.U64(8 * b)) == 0) and len(np.unique(k)) == 256
    k = np.sort(by["huge-seams"].queries[0].keys)
    assert all(k[i - 1] == k[i] for i in (64, 4096, 8192, 69632))
    assert sum(1 for q in by["huge-two"].queries if q.cls == "huge") == 2 and by["huge-paired"].paired
    assert by["huge-u-70000"].u == 70000 and [len(q.keys) for q in by["huge-u-70000"].queries] == [69000, 70001]
    # -m above the raw count in every path
    for cls in ("keep", "wave", "b2048", "b4096", "wg", "huge"):
        assert any(len(q.keys) < c.mm for c in D.CASES for q in c.queries if q.cls.startswith(cls)), cls
    assert by["nk-simple"].seq == ["nk_simple"] and {len(q.keys) < by["nk-simple"].mm for q in by["nk-simple"].queries} == {True, False}


def test_declared_launches_cover_the_stage():
    seen = set()
    for c in D.CASES:
        seen.update(D.identity(r) for r in D.expand(c.seq, len(c.queries), c.u, c.max_n, c.fb))
    assert sorted(seen) == D.ALL_KERNELS
    assert len(D.huge_records(0, 65537)) == 46
    # the large case: one more scan tile than one workgroup's threads, so k_scan_u32 walks two elements per thread
    nw = -(-D.LARGE_N // D.KEYS_PER_WAVE)
    assert -(-256 * nw // D.SCAN_TILE) == 1025 and D.LARGE_C % 2 == 1 and ((D.LARGE_N - 1) // 3) * D.LARGE_C < 1 << 63
    assert D.LARGE_SEQ[-1] == ("huge", 0, D.LARGE_N)


def test_reference_on_a_small_list():
    c = D.Case("x", 4, 3, 0, 0, 0, True, 6, False, [D.Q(np.array([5, 1, 5, 2, 2, 9], dtype=D.U64), "wave", None), D.Q(np.array([3, 1, 3], dtype=D.U64), "keep", None),
                                                  D.Q(np.array([3, 1], dtype=D.U64), "keep", None)], ["dedup", "wave"], (0, 0, 0))
    (a, la), (b, lb), (d, ld) = D.reference(c)
    assert a == 4 and la.tolist() == [1, 2, 5, 9] and b == 3 and lb.tolist() == [3, 1, 3] and d == 0 and ld.tolist() == [3, 1]
    assert D.bucket_of([D.MAX_HASH], D.KEY_SHIFT, 1024).tolist() == [524] and D.bucket_of([int(D.ALL_ONES)], 0, 2048).tolist() == [2047]
    assert D.canonical([("k_dedup_wave",), ("k_rs_hist", 0, 0, 0, 0, 0, 4, 9), ("k_uq_count", 0, 0, 0, 0, 0, 4, 9), ("k_rs_hist", 0, 0, 0, 0, 0, 0, 7)]) == \
        [("k_dedup_wave",), ("k_rs_hist", 0, 0, 0, 0, 0, 0, 7), ("k_rs_hist", 0, 0, 0, 0, 0, 4, 9), ("k_uq_count", 0, 0, 0, 0, 0, 4, 9)]
