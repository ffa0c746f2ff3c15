"""The hit buffer's overflow contract of kmcpg_query_device at every place of the COBS kernels that reserves and stores hits
(tests/k2_overflow.py: the sites, the checker, the cases).

Every case searches one batch of about 40 reads with 25 buffers — the one that fits, one row more, none at all, 0, 1, 63, 64, 65, 16
odd sizes in between, one row too few — and then once more with the buffer that fits, as lane.cpp collect() reruns a batch whose count
exceeded its buffer.  The buffer of every run is hit_cap + 4 096 rows of 0x5A5A5A5A, copied back whole: d_counters[0] must be the number of
hits of the batch whatever hit_cap is, the first min(hit_cap, hits) rows must be distinct hits of the reference, written without a hole,
and every row behind them must be as it was.  The witness (Database.last_k2_launches(), last_k2_grids()) must be the plan's in every run: a
small buffer does not change which kernels run, and the grid is what tells the short-read unit's kernels from the body's.

The reference is tests/test_gpu_k2_forms.py's: counts from the rows copied back from HBM (row = h % NumSigs per block, uint32(hi + lo * i) for
several hash functions, AND over the hash functions, int64 sums), never a run of the kernels.  min_matched = 1; min_qcov is picked from
those counts so that about an eighth of the (read, column) pairs pass (KMCPG_FPR_BOUND=0: the count threshold alone defines the list).
One read is copied into the first 200 columns of block 0 and one into the last 200 of the last block: a lane's 16 bytes then hold 128
neighbouring hits, and some buffer ends inside such a run.  Every assertion is an equality or a membership."""
import numpy as np
import pytest

from tests import k2_forms_plan as P
from tests import k2_overflow as V
from tests.test_gpu_k2_forms import _KNOBS, _OPEN_KNOBS, _Env, ref_counts

pytestmark = pytest.mark.gpu

PASS_SHARE = 0.125
T_MIN, T_MAX = 512, 1 << 18
assert set(V.K2_KNOBS) <= set(_KNOBS)


class _State:
    """one open database with the batches of its cases planted; a batch's reference is computed once and shared by its cases"""

    def __init__(self, dbk, O):
        import torch
        from kmcp_amd import Database, default_params, lib
        self.torch, self.dbk = torch, dbk
        d = V.DB[dbk]
        lay = P.LAYOUT[d.layout]
        self.d, self.lay, self.ncols = d, lay, lay.blocks * lay.cols
        self.slots = sum(P.lane_classes(P.stride_of(d), d.nh, d.open_env)[1].values())   # tiles of one block's rows
        dens = P.AND_DENSITY ** (1.0 / d.nh)
        kpc = int(round(-np.log(1.0 - dens) * d.num_sigs / d.nh))
        spec = lib.SynthSpec(k=P.K, num_hashes=d.nh, fpr=0.3, n_blocks=lay.blocks, cols_per_block=lay.cols, num_sigs=d.num_sigs, kmers_per_col=kpc,
                             seed=1 + sum(dbk.encode()), sigs_step=lay.step)
        with _Env(dict({k: None for k in _OPEN_KNOBS}, **dict(d.open_env))):
            self.db = Database.open_synthetic(spec)
        try:
            db, dev = self.db, torch.device("cuda:0")
            assert {db.block_info(b)["stride"] for b in range(lay.blocks)} == {P.stride_of(d)}
            assert db.info.num_hashes == d.nh and db.info.n_cols == self.ncols
            assert int(db.info.matrix_bytes_local) < (4 << 30)          # the plan's expectations are for an index below 4 GiB
            cfg = O.sketch_cfg(k=P.K)
            rng = np.random.default_rng(sum(dbk.encode()))
            self.run_cols = min(V.RUN, lay.cols)
            first = db.block_info(0)["col_base"]
            last = db.block_info(lay.blocks - 1)["col_base"] + lay.cols - self.run_cols
            self.batches = {}
            for batch in sorted({c.batch for c in V.CASES if c.db == dbk}):
                ns = np.array(V.BATCH_N[batch], dtype=np.int64)
                lens = ns + P.K - 1                                     # n = 0: a read one base shorter than k
                offs = np.zeros(len(ns) + 1, dtype=np.int64)
                offs[1:] = np.cumsum(lens)
                seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offs[-1]))]
                kms = [O.generate_kmers(seq[offs[i]:offs[i + 1]].tobytes(), cfg) for i in range(len(ns))]
                assert [len(k) for k in kms] == ns.tolist()
                head, tail = V.planted(batch)
                for c in range(self.run_cols):
                    db.plant(first + c, kms[head])
                    db.plant(last + c, kms[tail])
                self.batches[batch] = dict(ns=ns, kms=kms, total=int(offs[-1]), maxlen=int(lens.max()), head=(head, first), tail=(tail, last),
                                           seq=torch.from_numpy(seq.copy()).to(dev), offs=torch.from_numpy(offs).to(dev), ref=None)
            db.set_profiling(1)
            self.default_params = default_params
        except BaseException:
            self.db.close()
            raise

    def close(self):
        self.db.close()

    def reference(self, batch):
        """the batch's complete list, sorted by key = read * ncols + col, from the rows as they are after every plant — and what must hold
        of it before any run with a small buffer"""
        B = self.batches[batch]
        if B["ref"] is None:
            ns = B["ns"]
            counts = ref_counts(self.db, self.d.nh, B["kms"], self.ncols, self.lay.blocks)
            q = V.pick_qcov(counts, ns, min(int(PASS_SHARE * counts.size), T_MAX - 2 * V.GUARD))
            hit = (counts >= V.cmin(ns, q)[:, None]) & (ns > 0)[:, None]
            r, c = np.nonzero(hit)
            T = len(r)
            assert T_MIN <= T <= T_MAX, (self.dbk, batch, T)
            for i, col0 in (B["head"], B["tail"]):
                assert int(hit[i, col0:col0 + self.run_cols].sum()) == self.run_cols, "a planted read is a hit in every column of its run"
                assert int(hit[i].sum()) >= self.run_cols
            per_read = hit.sum(axis=1)
            B["ref"] = dict(key=r.astype(np.int64) * self.ncols + c, cnt=counts[r, c], qk=ns.astype(np.int32), q=q, per_read=per_read,
                            params=self.default_params(min_qlen=0, min_matched=1, min_qcov=float(q), dedup_threshold=1 << 30))
        return B["ref"]

    def run(self, batch, params, cap):
        """-> (d_counters, the whole buffer [cap + GUARD, 3] ([0, 3] for cap None: hit_cap 0 and no buffer), qkmers, launches, grids)"""
        torch, B = self.torch, self.batches[batch]
        dev = B["seq"].device
        n = len(B["ns"])
        buf = None if cap is None else torch.full((cap + V.GUARD, 3), V.SENTINEL, dtype=torch.int32, device=dev)
        cnt = torch.full((2,), -1, dtype=torch.int64, device=dev)
        qk = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ql = torch.zeros(n, dtype=torch.int32, device=dev)
        self.db.query_device(B["seq"].data_ptr(), B["offs"].data_ptr(), n, B["total"], B["maxlen"], None if buf is None else buf.data_ptr(), cap or 0,
                             cnt.data_ptr(), qk.data_ptr(), ql.data_ptr(), params=params)
        torch.cuda.synchronize()
        out = np.zeros((0, 3), dtype=np.int32) if buf is None else buf.cpu().numpy()
        return cnt.cpu().numpy(), out, qk.cpu().numpy(), self.db.last_k2_launches(), self.db.last_k2_grids()


_state = {}


def _get_state(dbk, O):
    """the last database used stays open (the cases come database by database)"""
    st = _state.get("st")
    if st is not None and st.dbk == dbk:
        return st
    if st is not None:
        _state.pop("st")
        st.close()
    _state["st"] = _State(dbk, O)
    return _state["st"]


@pytest.fixture(scope="module", autouse=True)
def _close_last_database():
    yield
    st = _state.pop("st", None)
    if st is not None:
        st.close()


def _witness(case, st, n_reads, launches, grids):
    """what the record of one run must say; -> problems"""
    problems = []
    if sorted(w[:6] for w in launches) != list(case.expect):
        problems.append("launched %s, the plan expects %s" % ([P.fmt(w[:6]) for w in launches], [P.fmt(f) for f in case.expect]))
    if case.grid is None or not launches:
        return problems
    first, workgroups, grid = launches[0][:6], launches[0][6], grids[0]
    if first != ("plain", 64, 0, V.PLANES[case.batch], False, 4):
        problems.append("the first launch is %s" % P.fmt(first))
    slots = st.lay.blocks * (1 if case.grid == "block" else st.slots)      # units per read: one per block, or one per tile
    if workgroups != (n_reads * slots + 3) // 4:
        problems.append("%d workgroups for %d reads x %d units" % (workgroups, n_reads, slots))
    if case.grid == "resident":
        ok = 1 <= grid <= workgroups
    else:
        ok = grid == (case.grid if isinstance(case.grid, int) else workgroups)
    if not ok:
        problems.append("grid %d (%s; the piece has %d workgroups)" % (grid, case.grid, workgroups))
    return problems


@pytest.mark.parametrize("case", V.CASES, ids=[c.id for c in V.CASES])
def test_hit_buffer_contract(case, oracle_lib):
    st = _get_state(case.db, oracle_lib)
    assert case.expect == tuple(P.expect(st.d, V.BATCH_N[case.batch], case.env))
    R = st.reference(case.batch)
    ns = st.batches[case.batch]["ns"]
    T = len(R["key"])
    if case.site == "C":    # both sides of KMCPG_SPLIT_MIN contribute: the chunked form's site runs on a counter the other site has advanced
        short, long_ = int(R["per_read"][ns <= V.SPLIT_MIN].sum()), int(R["per_read"][ns > V.SPLIT_MIN].sum())
        assert short >= 64 and long_ >= 64 and short + long_ == T, (short, long_, T)
    env = dict({k: None for k in _KNOBS}, KMCPG_FPR_BOUND="0", **case.env)
    caps = V.capacities(T) + [T]
    problems, launches = [], None
    for step, cap in enumerate(caps):
        with _Env(env):
            cnt, buf, qk, launches, grids = st.run(case.batch, R["params"], cap)
        found = V.check_run(R["key"], R["cnt"], st.ncols, cap or 0, int(cnt[0]), buf)
        if int(cnt[1]) != int(ns.max()):
            found.append("d_counters[1] is %d, the longest read has %d k-mers" % (int(cnt[1]), int(ns.max())))
        if not np.array_equal(qk, R["qk"]):
            found.append("NumKmers of the batch differ from the oracle's")
        found += _witness(case, st, len(ns), launches, grids)
        problems += ["run %d, hit_cap %s: %s" % (step, "0 without a buffer" if cap is None else cap, p) for p in found]
    print("%s: T %d (min_qcov %.2f), %d capacities, launches %s, grids %s" % (case.id, T, R["q"], len(caps), [P.fmt(w[:6]) for w in launches], grids))
    assert not problems, "%s: %d hits\n" % (case.id, T) + "\n".join(problems[:40])
