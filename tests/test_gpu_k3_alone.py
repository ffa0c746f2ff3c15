"""K3 alone (kmcp_amd/csrc/k3_finalize.hip: k3_count, k3_scan_*, k3_scatter, k3_sort_wave, k3_sort_wg and their _set forms), driven
through kmcpg_group_device on hit lists the test lays out (tests/k3_cases.py) and held against the plain numpy restatement there, which
tests/test_k3_reference_cpu.py holds against the host half.  What the cases reach that K2's own output does not: the three-launch scan
with more than one tile and more than 256 tiles, find_run at lane 63, runs that fill or cross a wave, runs broken by a tombstone, a
hit that names no read or column or a hit that fails -T, the second trip of every grid-stride loop, segments of exactly 1 / 2,
512 / 513, 4096 / 4097 matches, read counts that are no multiple of 16 or 64, exact ties in every key component, -T on the boundary
and one ulp on either side, and on a database set the second pass with its witness counters (equal to the restatement's, not merely
at least as large).

Segments of more than 4096 matches are compared as multisets: K3 leaves their order to the host, and kmcpg_finalize_grouped on the
whole device output must equal kmcpg_finalize on the same hits.  Column sizes above 2^32 — the high word of the qcov key — cannot be
reached with a real database: they stay with tests/k3_keys_check.cpp (tests/test_k3_keys_cpu.py).  Every hit list stays inside the
contract of kmcpg_group_device; no case aims at an access out of bounds."""
import numpy as np
import pytest

from tests import k3_cases as K

pytestmark = pytest.mark.gpu

MODE_NAMES = ("qcov", "tcov", "jacc", "nosort")
GUARD = 16
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def single_dir(oracle_lib, tmp_path_factory):
    return K.build_database(oracle_lib, tmp_path_factory.mktemp("k3db"), 4200, seed=700)


@pytest.fixture(scope="module")
def single(single_dir):
    from kmcp_amd import Database
    with Database.open(single_dir, device=0) as db:
        yield db, K.sizes_of(db), None


@pytest.fixture(scope="module")
def the_set(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    tmp = tmp_path_factory.mktemp("k3set")
    dirs = [K.build_database(oracle_lib, tmp / f"m{i}", 1500, seed=710 + i) for i in range(3)]
    with Database.open_set(dirs, device=0) as db:
        yield db, K.sizes_of(db), db.set_info()


_shared = {}


def shared(key, make):
    """a case (or a reference) several tests need: made once, never changed"""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def _same(a, b):
    for f in ("qlen", "qkmers", "ksize", "offs"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.matches.tobytes() == b.matches.tobytes()


def run(handle, name, case, params, ref=None):
    """K3 on the case through kmcpg_group_device; returns read_offs as the device left them and the records kmcpg_finalize_grouped made of
    its output"""
    import torch
    db, sizes, bases = handle
    dev = torch.device("cuda", 0)
    if ref is None:
        ref = K.reference_of(case, sizes, params, bases)
    n, cap = case.n_reads, case.hit_cap
    assert len(case.hits) == cap and len(case.nk) == n and case.nk.min() >= 1
    t_hits = torch.from_numpy(case.hits.view(np.uint32).reshape(-1, 3).view(np.int32)).to(dev)
    t_word = torch.tensor([case.n_hits_word, 0], dtype=torch.int64, device=dev)
    t_nk = torch.from_numpy(case.nk).to(dev)
    t_pairs = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int64, device=dev)  # a pair is one 8-byte word
    t_offs = torch.full((n + 2 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    db.group_device(t_hits.data_ptr(), t_word.data_ptr(), cap, t_nk.data_ptr(), n, t_pairs.data_ptr(), t_offs.data_ptr(), params=params)
    torch.cuda.synchronize()
    witness = db.last_set_order() if bases is not None else None
    assert np.array_equal(t_hits.cpu().numpy().view(np.uint32).reshape(-1).view(K.HIT_DTYPE), case.hits), f"{name}: the hit list was changed"
    assert t_word.cpu().tolist() == [case.n_hits_word, 0], f"{name}: the count word was changed"
    assert bool((t_pairs[cap:] == SENTINEL).all()), f"{name}: pairs written behind hit_cap"
    assert bool((t_offs[n + 2:] == SENTINEL).all()), f"{name}: read_offs written behind n_reads + 2"
    ro = t_offs[:n + 2].cpu().numpy().view(np.uint64).copy()
    pairs = t_pairs[:cap].cpu().numpy().view(np.uint32).reshape(-1, 2)
    msg = K.first_difference(name, ro, pairs, ref)
    assert msg is None, msg
    assert int(ro[n + 1]) == ref.bad, f"{name}: {int(ro[n + 1])} bad hits for {ref.bad}"
    if witness is not None:
        got = (witness["wave_segments"], witness["wg_segments"], witness["long_segments"], witness["device_mixed_runs"])
        assert got == ref.classes + (ref.mixed_runs,), f"{name}: witness (wave, workgroup, long, mixed runs) {got} for {ref.classes + (ref.mixed_runs,)}"
    # the host half behind K3 on the whole device output == the host half alone on the same hits
    ro[n + 1] = 0  # (it refuses a list with bad hits, as kmcpg_finalize does: both get the list without them)
    qlen = case.nk + 20
    grouped = db.finalize_grouped(pairs[:int(ro[n])], ro, case.nk, qlen, params=params)
    _same(grouped, db.finalize(K.well_formed(case, len(sizes)), case.nk, qlen, params=params))
    return ro, grouped


# ---- case 1: class edges ----
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("order", ["runs", "shuffled", "round_robin", "descending", "runs-last-empty"])
def test_class_edges(single, order, mode):
    sizes = single[1]
    case = shared(("edges", order), lambda: K.class_edges(sizes, order.split("-")[0], last_empty=order.endswith("empty")))
    run(single, f"class edges, {order}, {mode}", case, K.params_for(mode))


# ---- case 2: runs and lanes ----
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("drop", [False, True], ids=["T0", "T-drops-a-third"])
def test_runs_and_lanes(single, drop, mode):
    sizes = single[1]
    case, _ = shared("lanes", lambda: K.runs_and_lanes(sizes))
    t = K.tcov_quantile(case, sizes, 1 / 3) if drop else 0.0
    run(single, f"runs and lanes, -T {t}, {mode}", case, K.params_for(mode, t))
    for name, cut in K.prefixes(case).items():
        run(single, f"runs and lanes, {name}, -T {t}, {mode}", cut, K.params_for(mode, t))


# ---- case 3: ties and the -T boundary ----
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_ties_and_the_T_boundary(single, mode):
    sizes = single[1]
    case = shared("ties", lambda: K.ties(sizes))
    third = 1 / 3
    for t in (0.0, third, float(np.nextafter(third, 1)), float(np.nextafter(third, 0)), 0.05):
        run(single, f"ties, -T {t!r}, {mode}", case, K.params_for(mode, t))


# ---- case 4: many reads ----
MILLION = 256 * 4096 + 5


def _many(sizes, n_reads, mode):
    case = shared(("many", n_reads), lambda: K.many_reads(sizes, n_reads, "runs" if n_reads % 2 else "shuffled"))
    p = K.params_for(mode)
    return case, p, shared(("many", n_reads, mode), lambda: K.reference_of(case, sizes, p))


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("n_reads", [4094, 4095, 4096, 4097, 8191, 8192, 65535])
def test_many_reads(single, n_reads, mode):
    case, p, ref = _many(single[1], n_reads, mode)
    run(single, f"{n_reads} reads, {mode}", case, p, ref)


@pytest.mark.parametrize("mode", ["qcov", "tcov"])
def test_a_million_reads(single, mode):
    """257 tiles of the scan (the second trip of k3_scan_sums), a k3_sort_wg grid that strides, a last wave of five reads"""
    case, p, ref = _many(single[1], MILLION, mode)
    run(single, f"{MILLION} reads, {mode}", case, p, ref)


# ---- case 5: many hits ----
def test_many_hits(single):
    """hit_cap above 16384 x 256: the count and scatter grids make a second trip; then the count word above hit_cap"""
    sizes = single[1]
    case = K.many_hits(sizes)
    p = K.params_for("qcov")
    ref = K.reference_of(case, sizes, p)
    run(single, "many hits", case, p, ref)
    run(single, "many hits, the count word above hit_cap", case._replace(n_hits_word=case.hit_cap + 1000), p, ref)


# ---- case 6: workspace reuse ----
def test_workspace_reuse(single):
    """a large batch, then a small one twice, on one handle: each is right, the counters of the earlier call do not leak"""
    sizes = single[1]
    big, p, ref = _many(sizes, MILLION, "tcov")
    run(single, "reuse: a million reads", big, p, ref)
    small = shared(("edges", "runs"), lambda: K.class_edges(sizes, "runs"))
    a = run(single, "reuse: class edges after a million reads", small, p)
    b = run(single, "reuse: class edges again", small, p)
    assert np.array_equal(a[0], b[0])


# ---- case 7: sets ----
@pytest.mark.parametrize("mode", ["qcov", "tcov", "jacc"])
@pytest.mark.parametrize("order", ["runs", "shuffled"])
def test_set_class_edges(the_set, order, mode):
    sizes = the_set[1]
    case = shared(("set", order), lambda: K.class_edges(sizes, order, seed=7, k32=True, big_nk=True))
    run(the_set, f"set, class edges, {order}, {mode}", case, K.params_for(mode))


def test_one_member_set_is_the_database(single, single_dir):
    from kmcp_amd import Database
    sizes = single[1]
    case = shared(("edges", "shuffled"), lambda: K.class_edges(sizes, "shuffled"))
    with Database.open_set([single_dir], device=0) as one:
        assert one.set_info() == [0] and np.array_equal(K.sizes_of(one), sizes)
        for mode in MODE_NAMES:
            p = K.params_for(mode)
            a = run(single, f"database, {mode}", case, p)
            b = run((one, sizes, None), f"one-member set, {mode}", case, p)
            assert np.array_equal(a[0], b[0]) and a[1].matches.tobytes() == b[1].matches.tobytes(), mode
