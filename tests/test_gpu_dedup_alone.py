"""K1d alone: the sort + unique of the queries above -u (kmcp_amd/csrc/k1_dedup.hip, sort_huge.hip, query.cpp run_dedup) through
kmcpg_dedup_device on hash lists laid out by hand, against np.unique, bit for bit, with a launch witness.

Every case of tests/dedup_cases.py (the smallest batches at each edge: class bounds, lane / tile / wave seams, 24 against 25 keys in a
bucket, one workgroup striding from a fallback query to a bucketed one, keys 0 and ~0, keys that differ in one byte plane, -m above the
raw count, two huge queries, a paired layout, -u above 65 536) is laid out with a guard of a sentinel value in front of and behind both
buffers and slots longer than their lists, NumKmers preset to -7, and after the run

  * NumKmers of every query and the first NumKmers words of its slot are the reference's (np.unique above -u);
  * every word outside the lists of the queries above -u — the guards, the slot tails, the whole slot of a query at or below -u,
    order included — is unchanged, in hashes and in scratch;
  * the witness (`Database.last_dedup_launches()`, written at the launch sites) is the sequence the case declares: the branch of the
    stage with the number of queries each distribution class sent to its bitonic fallback, every kernel with its template parameters,
    grid, block and class, and the 46 launches of the device-wide sort per huge query.  A regression that drops a class, or lets every
    query fall through to the bitonic network, changes no hash; it changes this list.

Over the module the union of the witnessed kernels must be dedup_cases.ALL_KERNELS.  tests/test_dedup_cases_cpu.py checks the table
itself without a GPU."""
import os

import numpy as np
import pytest

from tests import dedup_cases as D

pytestmark = pytest.mark.gpu

GUARD = 64                                  # words of sentinel in front of and behind each buffer
SENT_H, SENT_S = 0x5EA15EA15EA15EA1, 0x6B6B6B6B6B6B6B6B   # no case holds either as a key (checked per case)
KNOB = "KMCPG_DEDUP_BIG_BUCKET"

_state = {}
_witnessed = set()
_done = set()


def _db():
    from kmcp_amd import Database, lib
    if "db" not in _state:  # the handle lends its workspace (the tables of the device-wide sort); the index is never looked at
        db = Database.open_synthetic(lib.SynthSpec(k=21, num_hashes=1, fpr=0.3, n_blocks=1, cols_per_block=8, num_sigs=1000, kmers_per_col=10, seed=1))
        db.set_profiling(1)
        _state["db"] = db
    return _state["db"]


@pytest.fixture(scope="module", autouse=True)
def _close_database():
    yield
    if "db" in _state:
        _state.pop("db").close()


class _Knob:
    def __init__(self, big_bucket):
        self.v = None if big_bucket else "0"

    def __enter__(self):
        self.old = os.environ.pop(KNOB, None)
        if self.v is not None:
            os.environ[KNOB] = self.v

    def __exit__(self, *a):
        os.environ.pop(KNOB, None)
        if self.old is not None:
            os.environ[KNOB] = self.old


def _call(db, *a, **kw):
    """a device error is no mismatch: nothing more is started on a GPU that reported one"""
    import torch
    from kmcp_amd import lib
    try:
        db.dedup_device(*a, **kw)
        torch.cuda.synchronize()
        return db.last_dedup_launches()
    except (lib.KmcpGpuError, RuntimeError) as err:
        pytest.exit("dedup stage: %s" % err, returncode=3)


def _problems(c):
    import torch
    dev = torch.device("cuda:0")
    db = _db()
    koff, offs, offs2, total = D.layout(c)
    n = np.array([len(q.keys) for q in c.queries], dtype=np.int64)
    H = np.full(total + 2 * GUARD, SENT_H, dtype=np.uint64)
    S = np.full(total + 2 * GUARD, SENT_S, dtype=np.uint64)
    nk0 = np.full(len(n), -7, dtype=np.int32)
    free = np.ones(len(H), dtype=bool)       # words the stage must leave alone
    for r, q in enumerate(c.queries):
        assert SENT_H not in q.keys and SENT_S not in q.keys
        at = GUARD + int(koff[r])
        H[at:at + n[r]] = q.keys
        if n[r] > c.u:
            free[at:at + n[r]] = False
    if c.pre_done:  # what the fused k-mer kernel leaves: the list without adjacent repeats in scratch, its length in nk_search
        for r, (m, lst) in enumerate(D.pre_done_state(c)):
            if m is not None:
                S[GUARD + int(koff[r]):GUARD + int(koff[r]) + m] = lst
                nk0[r] = m
    t_h, t_s = torch.from_numpy(H.view(np.int64)).to(dev), torch.from_numpy(S.view(np.int64)).to(dev)
    t_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    t_offs2 = torch.from_numpy(offs2.astype(np.int64)).to(dev) if c.paired else None
    t_raw, t_nk = torch.from_numpy(n.astype(np.int32)).to(dev), torch.from_numpy(nk0).to(dev)
    with _Knob(c.big_bucket):
        launches = _call(db, t_h.data_ptr() + 8 * GUARD, t_s.data_ptr() + 8 * GUARD, t_offs.data_ptr(), t_offs2.data_ptr() if c.paired else None,
                         t_raw.data_ptr(), t_nk.data_ptr(), len(n), c.max_n, c.u, min_matched=c.mm, pre=c.pre, pre_done=c.pre_done, key_shift=c.key_shift)
    _done.add(c.id)
    _witnessed.update(D.identity(w) for w in launches)
    H2, S2, nk = t_h.cpu().numpy().view(np.uint64), t_s.cpu().numpy().view(np.uint64), t_nk.cpu().numpy()
    assert np.array_equal(t_raw.cpu().numpy(), n.astype(np.int32)) and np.array_equal(t_offs.cpu().numpy(), offs)
    problems = []
    want = D.expand(c.seq, len(n), c.u, c.max_n, c.fb)
    got = D.canonical(launches)
    if got != want:
        d = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        problems.append("witness: %d launches for %d declared, first difference at %d: %s for %s" % (len(got), len(want), d, got[d:d + 1], want[d:d + 1]))
    for r, ((num, lst), q) in enumerate(zip(D.reference(c), c.queries)):
        at = GUARD + int(koff[r])
        if int(nk[r]) != num:
            problems.append("query %d (%d keys, %s): NumKmers %d, the reference has %d" % (r, n[r], q.cls, nk[r], num))
            continue
        if n[r] > c.u and n[r] >= c.mm and not np.array_equal(H2[at:at + num], lst):
            d = int(np.flatnonzero(H2[at:at + num] != lst)[0])
            problems.append("query %d (%d keys, %s): element %d of %d is %#x, the reference has %#x" % (r, n[r], q.cls, d, num, int(H2[at + d]), int(lst[d])))
    for name, a, b in (("hashes", H, H2), ("scratch", S, S2)):
        if not np.array_equal(a[free], b[free]):
            w = int(np.flatnonzero(free & (a != b))[0]) - GUARD
            r = int(np.searchsorted(koff, w, side="right")) - 1
            problems.append("%s: word %d (guards at < 0 and >= %d; query %d's slot starts at %d and holds %d keys) was written: %#x" %
                            (name, w, total, r, koff[max(r, 0)], n[max(r, 0)], int(b[w + GUARD])))
    return problems


def _check_case(c):
    problems = _problems(c)
    assert not problems, "%s:\n" % c.id + "\n".join(problems[:12])


@pytest.mark.parametrize("case", D.CASES, ids=[c.id for c in D.CASES])
def test_dedup_case(case):
    _check_case(case)


def test_one_query_of_16385_waves():
    """n = 4096 * 16384 + 1 keys: 1025 scan tiles, so k_scan_u32 walks two elements per thread (seg == 2).  Keys generated and compared on
    the device (1.1 GB of HBM for hashes and scratch, as much again for the temporaries of the fill); guards and slot tail as in the other
    cases.  Measured wall time on an MI355X, allocation, fill and comparison included: 0.25 s."""
    import time

    import torch
    t0 = time.time()
    dev = torch.device("cuda:0")
    db = _db()
    n, C, tail = D.LARGE_N, D.LARGE_C, 5
    t_h = torch.full((n + tail + 2 * GUARD,), SENT_H, dtype=torch.int64, device=dev)
    t_s = torch.full((n + tail + 2 * GUARD,), SENT_S, dtype=torch.int64, device=dev)
    i = torch.arange(n - 1, -1, -1, dtype=torch.int64, device=dev)
    t_h[GUARD:GUARD + n] = torch.div(i, 3, rounding_mode="floor") * C
    del i
    t_offs = torch.zeros(1, dtype=torch.int64, device=dev)
    t_raw, t_nk = torch.full((1,), n, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
    with _Knob(True):
        launches = _call(db, t_h.data_ptr() + 8 * GUARD, t_s.data_ptr() + 8 * GUARD, t_offs.data_ptr(), None, t_raw.data_ptr(), t_nk.data_ptr(), 1, n, 4)
    _witnessed.update(D.identity(w) for w in launches)
    m = (n + 2) // 3
    assert launches == D.expand(D.LARGE_SEQ, 1, 4, n, (0, 0, 0))
    assert int(t_nk.item()) == m
    assert bool(torch.equal(t_h[GUARD:GUARD + m], torch.arange(m, dtype=torch.int64, device=dev) * C))
    for t, s in ((t_h, SENT_H), (t_s, SENT_S)):
        assert bool((t[:GUARD] == s).all()) and bool((t[GUARD + n:] == s).all())
    print("one query of %d keys: %.2f s" % (n, time.time() - t0))


def test_witness_is_per_call_and_needs_profiling():
    by = {c.id: c for c in D.CASES}
    db = _db()
    for cid in ("wave-4", "nk-simple", "wave-4"):
        _check_case(by[cid])
        assert [w[0] for w in db.last_dedup_launches()] == {"wave-4": ["launch_dedup", "k_dedup_wave"], "nk-simple": ["k_nk_simple"]}[cid]
    db.set_profiling(0)
    try:
        assert db.last_dedup_launches() == []
        p = _problems(by["bucket-24-25"])   # everything else of the case still holds
        assert len(p) == 1 and p[0].startswith("witness: 0 launches"), p
        db.set_profiling(1)
        assert db.last_dedup_launches() == []   # nothing was recorded while profiling was off
    finally:
        db.set_profiling(1)


def test_every_kernel_was_witnessed():
    """the union of what the cases above launched is every kernel of the stage (cases that were deselected run here)"""
    for c in D.CASES:
        if c.id not in _done:
            _check_case(c)
    assert sorted(_witnessed) == D.ALL_KERNELS, (sorted(set(D.ALL_KERNELS) - _witnessed), sorted(_witnessed - set(D.ALL_KERNELS)))
