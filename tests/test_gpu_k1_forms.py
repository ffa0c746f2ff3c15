"""Every K1 kernel the plan can launch, alone, against the oracle, with a launch witness.

kmcp_amd/csrc/k1_kmers.hip dispatches ten forms onto 33 kernel instantiations that a batch can reach (k1_forms_plan.ALL_KERNELS; the 34th,
k1_windows_roll<32, 4>, fits no LDS).  For every case of the plan (tests/k1_forms_plan.py: the smallest batches at each edge — tile, wave
and lane seams, the -u / -m bounds, the plan's thresholds, the LDS limits of the rolling kernel, mates that are empty or too short) this

  * runs the k-mer stage alone (kmcpg_kmers_device, _packed, _paired) under the case's KMCPG_K1_FLAGS / KMCPG_WR_WAVES and compares
    every hash — values, order, multiplicity — and every count (NumKmers, and the first mate's count of a pair) with the oracle's
    generate_kmers per mate, mate 1's list followed by mate 2's, sort_unique above -u.  Bit for bit, no tolerance;
  * asserts that the witness (`Database.last_k1_launches()`, written at the launch sites from the launching functions' template
    parameters) names exactly the kernels the plan declares, in order, with their parameters, grids, block sizes and dynamic LDS, and
    that the two list forms left exactly the declared number of reads / segments to the kernel behind them (`left_on_list`): a
    regression that sends everything to the fallback kernel changes no hash, but it changes this number.

Over the module the union of the witnessed instantiations must be ALL_KERNELS.  tests/test_k1_forms_plan_cpu.py checks the plan
itself without a GPU.
"""
import os

import numpy as np
import pytest

from tests import k1_forms_plan as P

pytestmark = pytest.mark.gpu

_KNOBS = ("KMCPG_K1_FLAGS", "KMCPG_WR_WAVES", "KMCPG_K1_DEBUG")


class _Env:
    """the knobs a case may set are cleared first and restored afterwards: a case runs under its own settings only"""

    def __init__(self, kw):
        self.kw, self.old = dict({k: None for k in _KNOBS}, **kw), {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_dbs = {}
_witnessed = set()   # (kernel, p0, p1) over the module
_done = set()        # ids of the cases that ran


def _db(key):
    from kmcp_amd import Database, lib
    if key not in _dbs:
        spec = lib.SynthSpec(k=key.k, num_hashes=1, fpr=0.3, n_blocks=1, cols_per_block=8, num_sigs=1000, kmers_per_col=10, seed=1, scale=key.scale,
                             syncmer_s=key.ws if key.mode == "syn" else 0, minimizer_w=key.ws if key.mode == "min" else 0)
        db = Database.open_synthetic(spec)
        db.set_profiling(1)
        _dbs[key] = db
    return _dbs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_databases():
    yield
    while _dbs:
        _dbs.popitem()[1].close()


def _run(db, c):
    """the k-mer stage alone -> (hashes uint64, where each query's list starts, NumKmers, first mate's count or None)"""
    import torch
    from kmcp_amd import default_params, lib
    dev = torch.device("cuda:0")
    n = len(c.reads)
    seqs, offs = lib.pack_reads(c.reads)
    at = offs[:-1].astype(np.int64)
    total = len(seqs)
    t_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    p = default_params(min_qlen=c.min_qlen, min_matched=1, dedup_threshold=c.u)
    nk1 = None
    if c.paired:
        seqs2, offs2 = lib.pack_reads(c.reads2)
        at = at + offs2[:-1].astype(np.int64)
        total += len(seqs2)
        t_seqs, t_seqs2 = torch.from_numpy(seqs).to(dev), torch.from_numpy(seqs2).to(dev)
        t_offs2 = torch.from_numpy(offs2.view(np.int64)).to(dev)
    t_h = torch.zeros(total + 8, dtype=torch.int64, device=dev)
    t_nk = torch.full((n,), -7, dtype=torch.int32, device=dev)
    with _Env(c.env):
        if c.paired:
            t_nk1 = torch.full((n,), -7, dtype=torch.int32, device=dev)
            db.kmers_device_paired(t_seqs.data_ptr(), t_offs.data_ptr(), t_seqs2.data_ptr(), t_offs2.data_ptr(), n, total, c.max_read_len, t_h.data_ptr(),
                                   t_h.numel(), t_nk.data_ptr(), t_nk1.data_ptr(), params=p)
            nk1 = t_nk1.cpu().numpy()
        elif c.codes:
            codes, exc, tb = lib.pack2(c.reads)
            assert tb == total and len(exc) == len(P.foreign_runs(b"".join(c.reads)))
            pad = np.full((total + 3) // 4 + 16, 0xA5, dtype=np.uint8)    # (what lies behind the last base must not matter)
            pad[:(total + 3) // 4] = codes[:(total + 3) // 4]
            t_codes = torch.from_numpy(pad).to(dev)
            t_exc = torch.from_numpy(exc.view(np.uint8).copy()).to(dev) if len(exc) else None
            t_text = torch.full((total + 16,), ord("G"), dtype=torch.uint8, device=dev)
            db.kmers_device_packed(t_codes.data_ptr(), t_exc.data_ptr() if len(exc) else None, len(exc), t_text.data_ptr(), t_offs.data_ptr(), n, total,
                                   c.max_read_len, t_h.data_ptr(), t_h.numel(), None, t_nk.data_ptr(), params=p)
        else:
            t_seqs = torch.from_numpy(seqs).to(dev)
            db.kmers_device(t_seqs.data_ptr(), t_offs.data_ptr(), n, total, c.max_read_len, t_h.data_ptr(), t_h.numel(), None, t_nk.data_ptr(), params=p)
    torch.cuda.synchronize()
    return t_h.cpu().numpy().view(np.uint64), at, t_nk.cpu().numpy(), nk1


def _check_case(c, O):
    db = _db(c.db)
    ref = P.reference(c, O)
    from kmcp_amd import lib
    try:
        h, at, nk, nk1 = _run(db, c)
    except lib.KmcpGpuError as err:  # a device error is no mismatch: nothing more is started on a GPU that reported one
        pytest.exit("%s: %s" % (c.id, err), returncode=3)
    launches, plan = db.last_k1_launches(), db.last_k1_plan()
    _done.add(c.id)
    _witnessed.update(w[:3] for w in launches)
    problems = []
    e = c.expect
    if launches != e["kernels"]:
        problems.append("launched %s, the plan declares %s" % (launches, e["kernels"]))
    want_plan = dict(form=e["form"], codes_direct=e["codes_direct"], list_fallback=e["list_fallback"], adj_done=e["adj_done"], left_on_list=c.left)
    if plan != want_plan:
        problems.append("plan record %s, declared %s" % (plan, want_plan))
    for i, (raw1, raw2, want, n1) in enumerate(ref):
        L = (len(c.reads[i]), len(c.reads2[i]) if c.paired else None)
        if int(nk[i]) != len(want):
            problems.append("query %d (lengths %s): NumKmers %d, the oracle has %d (%d raw)" % (i, L, nk[i], len(want), len(raw1) + len(raw2)))
            continue
        got = h[int(at[i]):int(at[i]) + len(want)]
        if not np.array_equal(got, want):
            d = int(np.nonzero(got != want)[0][0])
            problems.append("query %d (lengths %s): hash %d of %d is %#x, the oracle has %#x" % (i, L, d, len(want), int(got[d]), int(want[d])))
        if nk1 is not None and int(nk1[i]) != n1:
            problems.append("query %d (lengths %s): first mate's count %d, the oracle has %d" % (i, L, nk1[i], n1))
    assert not problems, "%s:\n" % c.id + "\n".join(problems[:12])


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_k1_form(case, oracle_lib):
    _check_case(case, oracle_lib)


def _windows_of(L, step, window):
    return [(i, i + window) for i in range(0, L - window + 1, step)]


def test_win_once_witness(oracle_lib):
    """overlapping windows of plain k-mers run the four hash-once kernels and no other K1 kernel; windows that do not overlap run none of
    them.  (What they compute — every hash, count and qlen, at the kernels' edges — is compared with the oracle in
    tests/test_gpu_win_forms.py; here NumKmers only.)"""
    from kmcp_amd import default_params, lib
    O = oracle_lib
    key = P.Db(21, "plain", 0, 1)
    db = _db(key)
    reads = [P.rnd(1500, 900), P.rnd(700, 901), put_n(P.rnd(1000, 902))]
    seqs, offs = lib.pack_reads(reads)
    cfg = P.sketch_cfg(O, key)
    with _Env({}):
        for step, window, once in ((100, 300, True), (300, 300, False)):
            got = db.wait(db.submit_windows(seqs, offs, step, window, False, default_params()))
            want = []
            for r in reads:
                for i, e in _windows_of(len(r), step, window):
                    raw = O.generate_kmers(r[i:e], cfg)
                    want.append(len(O.sort_unique(raw)) if len(raw) > 256 else len(raw))
            assert list(got.qkmers) == want
            launches, plan = db.last_k1_launches(), db.last_k1_plan()
            assert plan["left_on_list"] is None
            if once:
                assert plan["form"] == "WinOnce" and [w[:3] for w in launches] == P.WIN_ONCE, (plan, launches)
                assert all(w[3] > 0 for w in launches) and [w[4] for w in launches] == [256, 1024, 256, 256]
                _witnessed.update(w[:3] for w in launches)
            else:
                assert plan["form"] == "Short" and [w[:3] for w in launches] == [("k1_kmers", 0, 0)], (plan, launches)


def put_n(seq):
    return P.put(seq, 450, b"N")


def test_witness_is_per_call_and_needs_profiling(oracle_lib):
    """the log names the launches of the LAST k-mer stage only; nothing is recorded without profiling; the asynchronous path records the
    launches but reads nothing back"""
    from kmcp_amd import default_params
    by_id = {c.id: c for c in P.CASES}
    a, b = by_id["roll-20-w2"], by_id["wave-f35-k21-syn11"]
    db = _db(a.db)
    assert a.db == b.db
    for c in (a, b, a):
        _run(db, c)
        assert db.last_k1_launches() == c.expect["kernels"], c.id
    assert db.last_k1_plan()["left_on_list"] == a.left
    with _Env(a.env):
        db.search(a.reads, params=default_params(min_qlen=0, min_matched=1, dedup_threshold=a.u))
    assert db.last_k1_launches() == a.expect["kernels"]
    assert db.last_k1_plan() == dict(form="WindowsRoll", codes_direct=False, list_fallback=True, adj_done=True, left_on_list=None)
    db.set_profiling(0)
    try:
        assert db.last_k1_launches() == [] and db.last_k1_plan() is None
        h, at, nk, _ = _run(db, a)
        assert [int(x) for x in nk] == [len(w) for _, _, w, _ in P.reference(a, oracle_lib)]
        assert db.last_k1_launches() == [] and db.last_k1_plan() is None
        db.set_profiling(1)
        assert db.last_k1_launches() == []   # nothing was recorded while profiling was off
    finally:
        db.set_profiling(1)


def test_every_instantiation_was_witnessed(oracle_lib):
    """the union of what the cases above launched is every instantiation launch_k1 can be asked for (cases that were deselected run here)"""
    for c in P.CASES:
        if c.id not in _done:
            _check_case(c, oracle_lib)
    if not set(P.WIN_ONCE) <= _witnessed:
        test_win_once_witness(oracle_lib)
    assert sorted(_witnessed) == P.ALL_KERNELS, (sorted(set(P.ALL_KERNELS) - _witnessed), sorted(_witnessed - set(P.ALL_KERNELS)))
