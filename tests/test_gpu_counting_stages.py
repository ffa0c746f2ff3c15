"""The counting stages (K6, K7, K8) TOGETHER on a lane: one loop enqueues their kernels behind K3, one walk of the reads they LEFT serves all
three at collect time, from pairs that come down once (kmcp_amd/csrc/lane.cpp, finalize.cpp left_reads_host).  On the family database,
reads and tables of tests/test_gpu_refstats.py plus its long query (above the device's -f bound: every stage leaves it to the host), the
three read-outs of the default form are the expectation — tests/test_gpu_refstats.py, test_gpu_cooccur.py and test_gpu_recount.py hold
that form against the restatements — and every other way through the lane must give the same bytes for all three:
    (a) every read to the host half of all three stages (the three KMCPG_*_DEVICE=0 knobs)
    (b) each knob alone: the three LEFT arrays differ, the walk hands a read to some stages and not to others
    (c) form (a) behind K4: K3's own offsets come down beside K4's, K3's pairs in one download
    (d) compact results (kmcpg_search_batch_pairs)        (e) three tickets in flight
The search result itself is what it is with the stages off.  host_reads of K6 and K8 is at least the number of matched reads where the
knob sends every read to the host, and below it otherwise; K7's host_reads counts reads with several targets only (kmcpg_cooccur_totals),
so its measure is multi_reads: equal to it where every read goes to the host, below it otherwise."""
import numpy as np
import pytest

from tests.test_gpu_recount import D, R, stage12
from tests.test_gpu_refstats import MIN_QCOV, family, tables  # noqa: F401 (family: the fixture)

pytestmark = pytest.mark.gpu

KNOBS = ("KMCPG_REFSTATS_DEVICE", "KMCPG_COOCCUR_DEVICE", "KMCPG_RECOUNT_DEVICE")
# (form, the knobs at 0, with K4)
FORMS = [("(a) host only", KNOBS, False)] + [(f"(b) {k}=0", (k,), False) for k in KNOBS] + [("(c) host only behind K4", KNOBS, True), ("(d) pairs", (), False),
                                                                                             ("(e) tickets", (), False)]


def test_every_way_through_the_lane_counts_the_same(family, monkeypatch):
    from kmcp_amd import Database, default_params, lib
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    reads = family["reads"] + [family["long_query"]]
    p = default_params(min_qcov=MIN_QCOV)
    same = ("qlen", "qkmers", "offs", "matches")
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        plain, plain_p = db.search(reads, params=p), db.search_pairs(reads, params=p)
        db.set_specific(target, species)
        plain_k4 = db.search(reads, params=p)
        db.set_specific()
        matched = int((np.diff(plain.offs) > 0).sum())
        assert matched > 500 and plain.qkmers[-1] > 512 and len(plain.read(len(reads) - 1)) > 0 and 0 < len(plain_k4.matches) < len(plain.matches)
        db.set_refstats(target, species, hic_min_qcov=0.8)
        db.set_cooccur(target)
        db.set_recount(target, species, hic_min_qcov=0.8)
        inputs = []

        def read_outs():
            """(the bytes of the three read-outs and the totals that do not depend on who counted, host_reads of the three, K7's multi_reads)"""
            k6, t6 = db.refstats_read(n)
            k7, t7 = db.cooccur_read()
            if not inputs:  # one fixed input of the replay: stages 1 and 2 as the default form counted them
                inputs.extend(stage12(db, family, names, target, n, 1.0))
            db.recount_run(*inputs, min_dreads_prop=D, max_mismatch_err=R)
            k8, t8 = db.recount_read()
            assert t6["skipped_launches"] == t7["skipped_launches"] == t8["skipped_launches"] == 0 and t7["left_full"] == t8["left_full"] == 0
            fixed = (k6.tobytes(), k7.tobytes(), k8.tobytes(), t6["matched_reads"], t6["unique_reads"], t7["multi_reads"], t7["device_adds"] + t7["host_adds"],
                     t8["recounted_reads"], t8["unique_reads"], t8["corrected_reads"])
            return fixed, (t6["host_reads"], t7["host_reads"], t8["host_reads"]), t7["multi_reads"]

        res = db.search(reads, params=p)
        assert all(np.array_equal(getattr(res, f), getattr(plain, f)) for f in same), "default: the result changed"
        want, host, multi = read_outs()
        assert want[3] == matched and want[7] > 400 and want[9] >= 50 and multi > 100 and len(inputs[1]) > 10, "the expectation must have something in it"
        assert 1 <= host[0] < matched and 1 <= host[1] < multi and 1 <= host[2] < matched, host  # (the long query at least)
        for form, zero, k4 in FORMS:
            db.refstats_reset()
            db.cooccur_reset()
            db.recount_reset()
            for k in zero:
                monkeypatch.setenv(k, "0")
            if k4:
                db.set_specific(target, species)
            if form == "(d) pairs":
                res = db.search_pairs(reads, params=p)
                assert all(np.array_equal(getattr(res, f), getattr(plain_p, f)) for f in ("qlen", "qkmers", "offs", "pairs")), f"{form}: the result changed"
            elif form == "(e) tickets":
                cuts = [0, 300, 600, len(reads)]
                tickets = [db.submit(*lib.pack_reads(reads[a:b]), params=p) for a, b in zip(cuts, cuts[1:])]
                parts = [db.wait(t) for t in tickets]
                assert np.array_equal(np.concatenate([x.matches for x in parts]), plain.matches), f"{form}: the result changed"
            else:
                res = db.search(reads, params=p)
                assert all(np.array_equal(getattr(res, f), getattr(plain_k4 if k4 else plain, f)) for f in same), f"{form}: the result changed"
            if k4:
                db.set_specific()
            for k in zero:
                monkeypatch.delenv(k)
            got, host, multi = read_outs()
            for name, g, w in zip(("K6", "K7", "K8", "K6 matched", "K6 unique", "K7 multi", "K7 adds", "K8 recounted", "K8 unique", "K8 corrected"), got, want):
                assert g == w, f"{form}: {name} differs from the default form"
            for s, (k, h, all_of_them) in enumerate(zip(KNOBS, host, (matched, multi, matched))):
                if k in zero:
                    assert (h == multi) if s == 1 else (h >= matched), f"{form}: {k}=0 but host_reads {h} of {all_of_them}"
                else:
                    assert 1 <= h < all_of_them, f"{form}: host_reads {h} of {all_of_them} without {k}=0"
        for last in (db.last_refstats, db.last_cooccur, db.last_recount):
            st, _ = last()
            assert st["bad_segments"] == 0 and st["skipped"] == 0
