"""Every form of the COBS kernel the dispatcher can launch, against counts taken from the rows, with a witness.

kmcp_amd/csrc/k2_cobs.hip launches 78 instantiations of one body (k2_forms_plan.ALL_FORMS: 40 eight-row and 20 four-row forms
of k2_cobs, 10 chunked long-query forms, 8 pair forms).  The plan (tests/k2_forms_plan.py) declares, for every case — a database
(lane layout x hash functions), a batch (one per plane class) and a setting — which of them must run; every case here

  * searches the batch with `kmcpg_query_device` (KMCPG_FPR_BOUND=0: the list is defined by the count threshold alone) and compares
    the COMPLETE raw hit list — every (read, column, count) with count >= cmin for every query of the batch, nothing else, no
    duplicates — with a reference that is independent of the kernel and of the finalize path: the queries' k-mer hashes from the
    CPU oracle, row = h % NumSigs per block (several hash functions: uint32(hi + lo * i)), the rows copied back from HBM, AND over the
    hash functions, per-column sums in int64 numpy, cmin = max(min_matched, floor(n * min_qcov) + 1);
  * asserts on the witness (`Database.last_k2_launches()`, written at the launch sites from the kernels' template parameters) that
    the instantiations the plan names ran, and only those.

Thresholds sit in the body of the count distribution: the AND of a k-mer's rows is set in ~30 % of the positions, and the two
thresholds of a batch — (a) a min_matched with min_qcov ~ 0, one cmin for all n; (b) a min_qcov with min_matched = 1, cmin varying
inside a wave — are picked from reference counts so that about an eighth of the (query, column) pairs pass: many columns exactly at
cmin and at cmin - 1, runs of neighbouring hits in a lane, sectors that die at every step of the branch and bound.  On top: full copies of
queries (count = n; at a class's maximum the all-ones counter), copies of the last cmin and last cmin - 1 k-mers (the pruning boundary),
in the first and last column of every block and on both sides of every 128-byte sector edge and 1-KiB tile edge of the rows.

Reference queries at the top of the 16- and 24-plane ranges: ONE each (65 534 and 65 535 k-mers; a 65 5xx-row gather per block and hash
function, taken in slices of 4 096 rows so the host never holds a whole unpacked gather), the rest of those batches is short.

Override only (no database reaches them by the default rules):
  * k2_cobs_pair<64,4,16,true>: KMCPG_ROW_ALIGN=64 at open;
  * the 20 four-row forms on indexes below 4 GiB: KMCPG_GROUP_ROWS=4 (`big8` takes k2_cobs<8,{8,10},false,false,4> by the default rule).
"""
import os

import numpy as np
import pytest

from tests import k2_forms_plan as P

pytestmark = pytest.mark.gpu

CAP = 1 << 20          # hit buffer (entries); a reference list holds at most half of it
PASS_SHARE = 0.125     # share of the (query, column) pairs the picked thresholds let pass
SLICE = 4096           # reference rows unpacked at a time
PREPASS_MAX_N = 4100   # queries up to this many k-mers are counted before planting (threshold choice); longer ones are assumed to pass everywhere


class _Env:
    def __init__(self, kw):
        self.kw, self.old = dict(kw), {}

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


# every variable a case may set is cleared first, so a case runs under its own settings only
_KNOBS = ("KMCPG_GROUP_ROWS", "KMCPG_PRUNE", "KMCPG_SPLIT_MIN", "KMCPG_SPLIT_CHUNK", "KMCPG_PAIR", "KMCPG_TAIL_SECTORS", "KMCPG_TAIL_MIN", "KMCPG_SLOT_MAJOR",
          "KMCPG_NT_LOADS", "KMCPG_PRUNE_EVERY", "KMCPG_K2_BLOCK_UNITS", "KMCPG_K2_EXACT_STOP", "KMCPG_K2_PERSIST", "KMCPG_K2_PERSIST_WGS")
_OPEN_KNOBS = ("KMCPG_ROW_ALIGN", "KMCPG_LPR32", "KMCPG_LPR8", "KMCPG_SPLIT_TILES", "KMCPG_FUSE")


def _hash_rows(km, t, nh, ns):
    hv = km if nh == 1 else ((km >> np.uint64(32)).astype(np.uint32) + km.astype(np.uint32) * np.uint32(t)).astype(np.uint64)
    return hv % ns


def ref_counts(db, nh, kms, ncols, n_blocks):
    """[query, global column] match counts from the rows resident in HBM; rows are gathered SLICE at a time"""
    out = np.zeros((len(kms), ncols), dtype=np.int64)
    pieces = []  # (query, lo, hi) pieces of at most SLICE k-mers, packed into slices
    cur, cur_n = [], 0
    for qi, km in enumerate(kms):
        lo = 0
        while lo < len(km):
            hi = min(len(km), lo + SLICE - cur_n)
            cur.append((qi, lo, hi))
            cur_n += hi - lo
            lo = hi
            if cur_n == SLICE:
                pieces.append(cur)
                cur, cur_n = [], 0
    if cur:
        pieces.append(cur)
    for b in range(n_blocks):
        info = db.block_info(b)
        ns, cb, nc = np.uint64(info["num_sigs"]), info["col_base"], info["n_cols"]
        for sl in pieces:
            km = np.concatenate([kms[qi][lo:hi] for qi, lo, hi in sl])
            acc = None
            for t in range(nh):
                bits = db.read_rows(b, _hash_rows(km, t, nh, ns))
                acc = bits if acc is None else (acc & bits)
            un = np.unpackbits(acc, axis=1)[:, :nc]
            pos = 0
            for qi, lo, hi in sl:
                for r0 in range(pos, pos + hi - lo, 255):  # 255 rows fit a uint8 sum; the totals are int64
                    out[qi, cb:cb + nc] += un[r0:min(r0 + 255, pos + hi - lo)].sum(axis=0, dtype=np.uint8)
                pos += hi - lo
    return out


def _cmin(n, min_matched, min_qcov):
    return np.maximum(min_matched, np.floor(n * min_qcov).astype(np.int64) + 1)  # csa.hpp count_threshold


def _pick_thresholds(counts, ns, ncols, n_assumed):
    """(a) the smallest min_matched and (b) the smallest min_qcov (steps of 0.01) that let at most PASS_SHARE of the counted pairs pass
    and keep the list within half of the hit buffer (`n_assumed` uncounted long queries are taken to pass in every column)"""
    budget = min(CAP // 2 - n_assumed * ncols - 4096, int(PASS_SHARE * counts.size))
    assert 0 < budget < counts.size
    flat = np.sort(counts, axis=None)[::-1]
    m = max(1, int(flat[budget]) + 1)                    # at most `budget` counts are larger than the (budget + 1)-th largest
    assert int((counts >= m).sum()) <= budget
    ratio = np.sort((counts / np.maximum(ns, 1)[:, None]).ravel())[::-1]
    q = max(0.05, np.ceil(float(ratio[budget]) * 100) / 100)
    while int((counts >= _cmin(ns, 1, q)[:, None]).sum()) > budget:
        q = round(q + 0.01, 2)
    assert q < 1.0
    return m, float(round(q, 2))


def _edge_columns(db, lay, stride):
    """global columns in the first and last byte of every block and on both sides of every 128-byte edge of the group's rows
    (every eighth of them a 1-KiB tile edge)"""
    cols = set()
    rb = (lay.cols + 7) // 8
    for b in range(lay.blocks):
        base = b * lay.cols
        off = b * rb if lay.step == 0 else 0  # the block's first byte in its group's rows
        cols |= {base, base + min(7, lay.cols - 1), base + lay.cols - 1, base + (rb - 1) * 8}
        for edge in range(128, stride, 128):
            for byte, bit in ((edge - 1, 7), (edge, 0)):  # last column left of the edge, first column right of it
                c = (byte - off) * 8 + bit
                if byte >= off and 0 <= c < lay.cols:
                    cols.add(base + c)
    return sorted(cols)


class _State:
    """one open database with its four batches planted; the reference of a batch is computed once and shared by its cases"""

    def __init__(self, dbk, O):
        import torch
        from kmcp_amd import Database, lib
        self.torch, self.O, self.dbk = torch, O, dbk
        d = P.DB[dbk]
        lay = P.LAYOUT[d.layout]
        self.d, self.lay = d, lay
        self.ncols = lay.blocks * lay.cols
        dens = P.AND_DENSITY ** (1.0 / d.nh)
        kpc = int(round(-np.log(1.0 - dens) * d.num_sigs / d.nh))
        spec = lib.SynthSpec(k=P.K, num_hashes=d.nh, fpr=0.3, n_blocks=lay.blocks, cols_per_block=lay.cols, num_sigs=d.num_sigs, kmers_per_col=kpc,
                             seed=1 + sum(dbk.encode()), sigs_step=lay.step)
        with _Env(dict({k: None for k in _OPEN_KNOBS}, **dict(d.open_env))):
            self.db = Database.open_synthetic(spec)
        try:
            self._prepare()
        except BaseException:
            self.db.close()
            raise

    def close(self):
        self.db.close()

    def _prepare(self):
        torch, O, d, lay, db = self.torch, self.O, self.d, self.lay, self.db
        dev = torch.device("cuda:0")
        # the lane classes, from the pitch the database really got
        strides = {db.block_info(b)["stride"] for b in range(lay.blocks)}
        assert strides == {P.stride_of(d)}, (strides, P.stride_of(d))
        self.classes, self.slots = P.lane_classes(strides.pop(), d.nh, d.open_env)
        info = db.info
        assert info.num_hashes == d.nh and info.n_cols == self.ncols
        self.index_bytes = int(info.matrix_bytes_local)
        cfg = O.sketch_cfg(k=P.K)
        rng = np.random.default_rng(sum(self.dbk.encode()))
        edges = _edge_columns(db, lay, P.stride_of(d))
        self.batches = {}
        for batch, ns0 in sorted(P.BATCH_N.items()):
            ns = np.array(ns0, dtype=np.int64)[rng.permutation(len(ns0))]
            lens = ns + P.K - 1
            offs = np.zeros(len(ns) + 1, dtype=np.int64)
            offs[1:] = np.cumsum(lens)
            seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offs[-1]))]
            kms = [O.generate_kmers(seq[offs[i]:offs[i + 1]].tobytes(), cfg) for i in range(len(ns))]
            assert [len(k) for k in kms] == ns.tolist()
            # thresholds from reference counts of the database as it is now (the long queries are left out: they pass or fail whole)
            short = [i for i in range(len(ns)) if ns[i] <= PREPASS_MAX_N]
            pre = ref_counts(db, d.nh, [kms[i] for i in short], self.ncols, lay.blocks)
            m, q = _pick_thresholds(pre, ns[short], self.ncols, len(ns) - len(short))
            # plants: round-robin over the edge columns (+ a few random ones) and the queries
            cols = edges + [int(c) for c in rng.integers(0, self.ncols, 8)]
            elig = [i for i in range(len(ns)) if ns[i] >= 3]
            tops = [i for i in range(len(ns)) if ns[i] in (254, 255, 1022, 1023, 65534, 65535)]
            for j, c in enumerate(cols):
                i = elig[(j * 7 + batch) % len(elig)]
                n, km = int(ns[i]), kms[i]
                ca, cb = int(_cmin(np.int64(n), m, 1e-9)), int(_cmin(np.int64(n), 1, q))
                kind = j % 5
                if kind == 0:
                    db.plant(c, km)                                   # a full copy
                elif kind in (1, 2) and ca - (kind - 1) <= n:
                    db.plant(c, km[n - (ca - (kind - 1)):])           # the last cmin / cmin - 1 k-mers under threshold (a)
                elif kind in (3, 4) and 1 <= cb - (kind - 3) <= n:
                    db.plant(c, km[n - (cb - (kind - 3)):])           # ... under threshold (b)
            for j, i in enumerate(tops):                              # the class's maximum / the next one's minimum: count = n
                db.plant(cols[(3 * j + 1) % len(cols)], kms[i])
            self.batches[batch] = dict(ns=ns, kms=kms, m=m, q=q, total=int(offs[-1]), maxlen=int(lens.max()),
                                       seq=torch.from_numpy(seq.copy()).to(dev), offs=torch.from_numpy(offs).to(dev), ref=None)
        db.set_profiling(1)

    def reference(self, batch):
        """sorted (read * ncols + col, count) lists of the batch under its two thresholds, from the rows as they are after all plants"""
        B = self.batches[batch]
        if B["ref"] is None:
            from kmcp_amd import default_params
            counts = ref_counts(self.db, self.d.nh, B["kms"], self.ncols, self.lay.blocks)
            ns = B["ns"]
            ref = {}
            for name, mm, qc in (("a", B["m"], 1e-9), ("b", 1, B["q"])):
                cm = _cmin(ns, mm, qc)
                neff = np.where(ns >= mm, ns, 0)            # fewer k-mers than min_matched: not searched
                hit = (counts >= cm[:, None]) & (neff > 0)[:, None]
                r, c = np.nonzero(hit)
                assert len(r) <= CAP // 2, (len(r), CAP)
                at, below = int((counts == cm[:, None]).sum()), int((counts == cm[:, None] - 1).sum())
                print("%s %dp (%s) min_matched %d min_qcov %.2f: %d hits, %d pairs at cmin, %d at cmin - 1, %d queries" % (
                    self.dbk, batch, name, mm, qc, len(r), at, below, len(ns)))
                if batch in (8, 10):                        # the thresholds sit in the body of the distribution
                    assert at >= len(ns) and below >= len(ns), (name, at, below)
                ref[name] = dict(key=r.astype(np.int64) * self.ncols + c, cnt=counts[r, c], qk=neff.astype(np.int32),
                                 params=default_params(min_qlen=0, min_matched=int(mm), min_qcov=float(qc), dedup_threshold=1 << 30))
            B["ref"] = ref
        return B["ref"]

    def run(self, batch, params):
        torch, B = self.torch, self.batches[batch]
        dev = B["seq"].device
        n = len(B["ns"])
        hits = torch.zeros((CAP, 3), dtype=torch.int32, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        qk = torch.zeros(n, dtype=torch.int32, device=dev)
        ql = torch.zeros(n, dtype=torch.int32, device=dev)
        self.db.query_device(B["seq"].data_ptr(), B["offs"].data_ptr(), n, B["total"], B["maxlen"], hits.data_ptr(), CAP, cnt.data_ptr(), qk.data_ptr(),
                             ql.data_ptr(), params=params)
        torch.cuda.synchronize()
        m = int(cnt[0].item())
        assert m <= CAP, (m, CAP)
        h = hits[:m].to(torch.int64)
        key, order = torch.sort(h[:, 0] * self.ncols + h[:, 1])
        return key.cpu().numpy(), h[:, 2][order].cpu().numpy(), qk.cpu().numpy(), [w[:6] for w in self.db.last_k2_launches()]


_state = {}


def _get_state(dbk, O):
    """the last database used stays open (cases are generated database by database; any other order only costs time)"""
    st = _state.get("st")
    if st is not None and st.dbk == dbk:
        return st
    if st is not None:
        _state.pop("st")
        st.close()
    if dbk == P.BIG.key:
        import torch
        need = 2 * P.BIG.num_sigs * 128
        free = torch.cuda.mem_get_info()[0]
        if free < need:
            pytest.skip("the 4-GiB index of the default-rule case needs %.1f GB of free HBM, %.1f GB are free" % (need / 1e9, free / 1e9))
    _state["st"] = _State(dbk, O)
    return _state["st"]


@pytest.fixture(scope="module", autouse=True)
def _close_last_database():
    yield
    st = _state.pop("st", None)
    if st is not None:
        st.close()


def _describe(ncols, want_key, want_cnt, got_key, got_cnt, limit=6):
    w = {int(k): int(c) for k, c in zip(want_key, want_cnt)}
    g = {}
    dup = 0
    for k, c in zip(got_key, got_cnt):
        dup += int(k) in g
        g[int(k)] = int(c)
    miss = [(k // ncols, k % ncols, w[k]) for k in sorted(set(w) - set(g))]
    extra = [(k // ncols, k % ncols, g[k]) for k in sorted(set(g) - set(w))]
    wrong = [(k // ncols, k % ncols, w[k], g[k]) for k in sorted(set(g) & set(w)) if g[k] != w[k]]
    return "%d missing %s, %d extra %s, %d wrong counts (read, col, want, got) %s, %d duplicates" % (
        len(miss), miss[:limit], len(extra), extra[:limit], len(wrong), wrong[:limit], dup)


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_k2_form(case, oracle_lib):
    st = _get_state(case.db, oracle_lib)
    d = st.d
    assert (st.classes, st.slots) == P.lane_classes(P.stride_of(d), d.nh, d.open_env)
    # the plan's expectation is for the database as it really is
    assert list(case.expect) == P.expect(d, case.batch, case.env, index_bytes=st.index_bytes), "the plan was made for another index size"
    ref = st.reference(case.batch)
    env = dict({k: None for k in _KNOBS}, KMCPG_FPR_BOUND="0", **case.env)
    problems = []
    for name in ("a", "b"):
        R = ref[name]
        with _Env(env):
            key, cnt, qk, launches = st.run(case.batch, R["params"])
        forms = sorted(launches)
        if forms != list(case.expect):
            problems.append("threshold (%s): launched %s, the plan expects %s" % (name, [P.fmt(f) for f in forms], [P.fmt(f) for f in case.expect]))
        assert np.array_equal(qk, R["qk"]), "NumKmers of the batch differ from the oracle's"
        if not (np.array_equal(key, R["key"]) and np.array_equal(cnt, R["cnt"])):
            problems.append("threshold (%s: min_matched %d, min_qcov %.2f): %d hits expected, %d returned: %s" % (
                name, R["params"].min_matched, R["params"].min_qcov, len(R["key"]), len(key), _describe(st.ncols, R["key"], R["cnt"], key, cnt)))
    assert not problems, "%s [%s]\n" % (case.id, ", ".join(P.fmt(f) for f in case.expect)) + "\n".join(problems)


def test_witness_is_per_call(oracle_lib):
    """the log names the launches of the LAST call only, needs profiling level >= 1, and records nothing without it"""
    from kmcp_amd import lib
    case8 = next(c for c in P.CASES if c.id == "n8-h1-8p-default")
    case16 = next(c for c in P.CASES if c.id == "n8-h1-16p-default")
    st = _get_state(case8.db, oracle_lib)
    env = dict({k: None for k in _KNOBS}, KMCPG_FPR_BOUND="0")
    with _Env(env):
        for case in (case16, case8, case16):
            launches = st.run(case.batch, st.reference(case.batch)["b"]["params"])[3]
            assert sorted(launches) == list(case.expect), case.id
            assert all(w[6] > 0 for w in st.db.last_k2_launches())
        st.db.set_profiling(0)
        try:
            with pytest.raises(lib.KmcpGpuError):
                st.db.last_k2_launches()
            with pytest.raises(lib.KmcpGpuError):
                st.run(8, st.reference(8)["b"]["params"])   # the query runs; reading the log is what fails
            st.db.set_profiling(1)
            assert st.db.last_k2_launches() == []            # nothing was recorded while profiling was off
        finally:
            st.db.set_profiling(1)
