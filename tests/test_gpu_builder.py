"""kmcpg_builder alone (two-pass `kmcp index`: counts first, then device-resident lists ORed into block matrices in HBM by ONE
kernel launch per scatter call, build_scatter.hip).  The lists are crafted here and put on the device with torch; the files must be
byte for byte those of the oracle (O.build_db) and of kmcpg_build_db (lib.build_db, the one-pass path) on the same lists.  Shapes
are the smallest at which the kernel can still go wrong: rows of 1, 2 and 3 bytes (the aligned 32-bit word of a row's last byte then
straddles rows and, in the last row, the end of the matrix), eight columns racing for the same bytes, hashes that land on row 0 and
on the last row, lists around the keys one wave takes, 1 to 4 hash functions, lists of several blocks in one call / of one block in
several calls / out of order, rounds, and every refusal of scatter_device / end_round / finish.
Witness everywhere: scatter launches == scatter calls that held at least one key of the open round."""
import filecmp
import os

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_build import _yml

pytestmark = pytest.mark.gpu

YML_KEYS = ("version", "unikiVersion", "k", "ks", "hashed", "canonical", "scaled", "scale", "minimizer", "minimizer-w", "syncmer", "syncmer-s",
            "hashes", "numNameGroups", "blocksize", "totalKmers")
SKIP = 0xFFFFFFFF


def random_lists(sizes, seed):
    """columns (name, gsize, chunk_idx, chunks, sorted-unique hashes) of the given sizes"""
    rng = np.random.default_rng(seed)
    cols = []
    for i, n in enumerate(sizes):
        h = np.unique(rng.integers(0, 2**64, size=int(n) + 16, dtype=np.uint64))[:int(n)]
        assert len(h) == n
        cols.append(("c%04d" % i, 1000 + i, i % 3, 3, h))
    return cols


def on_device(arrays):
    """lists back to back in device memory -> (tensor that keeps them alive, device pointer, koff)"""
    import torch
    koff = np.zeros(len(arrays) + 1, dtype=np.uint64)
    koff[1:] = np.cumsum([len(a) for a in arrays], dtype=np.uint64)
    flat = np.concatenate([np.asarray(a, dtype=np.uint64) for a in arrays] + [np.zeros(1, dtype=np.uint64)])
    t = torch.from_numpy(flat.view(np.int64)).to("cuda:0")
    return t, t.data_ptr(), koff


def build(lib, out_dir, cols, calls=None, budget=1 << 34, junk=None, **cfg):
    """The whole call sequence.  calls: lists of column ids (SKIP = an entry to skip, given the list `junk`), every call made in
    every round; default one call with every column in order.  -> (R001 directory, info, planned rounds)"""
    import torch
    calls = [list(range(len(cols)))] if calls is None else calls
    junk = np.arange(70, dtype=np.uint64) if junk is None else junk
    staged = []
    for call in calls:
        t, ptr, koff = on_device([junk if c == SKIP else cols[c][4] for c in call])
        staged.append((t, ptr, koff, np.array(call, dtype=np.uint32)))
    with lib.Builder(device=0, **cfg) as b:
        b.add_cols([(n, g, ci, nch, len(h)) for n, g, ci, nch, h in cols])
        nb, nr = b.plan(budget)
        col_round = [b.col_place(c)[2] for c in range(len(cols))]
        want_launches = 0
        for r in range(nr):
            b.begin_round(r)
            assert b.info()["matrix_bytes_resident"] <= budget
            for (_, ptr, koff, ids), call in zip(staged, calls):
                b.scatter_device(ptr, koff, ids)
                want_launches += any(c != SKIP and col_round[c] == r and len(cols[c][4]) for c in call)
            b.end_round(out_dir)
            assert b.info()["matrix_bytes_resident"] == 0
        got = b.finish(out_dir)
        info = b.info()
        torch.cuda.synchronize()
    assert info["scatter_launches"] == want_launches and info["scatter_calls"] == nr * len(calls), info
    assert info["rounds_done"] == nr and info["matrix_bytes_peak"] <= budget
    assert info["keys_scattered"] == sum(len(c[4]) for c in cols)
    return got, info, nr


def assert_same_files(got, ref, whole=False):
    """block files byte for byte, __db.yml by value; whole: every file byte for byte (the one-pass path writes the same alias)"""
    yr, yg = _yml(os.path.join(ref, "__db.yml")), _yml(os.path.join(got, "__db.yml"))
    assert yr["files"] == yg["files"] and len(yr["files"]) >= 1
    for key in YML_KEYS:
        assert yr[key] == yg[key], key
    assert float(yr["fpr"]) == float(yg["fpr"])
    for f in yr["files"]:
        assert filecmp.cmp(os.path.join(ref, f), os.path.join(got, f), shallow=False), f
    assert open(os.path.join(ref, "__name_mapping.tsv")).read() == open(os.path.join(got, "__name_mapping.tsv")).read()
    assert sorted(os.listdir(got)) == sorted(os.listdir(ref))
    if whole:
        assert filecmp.cmp(os.path.join(ref, "__db.yml"), os.path.join(got, "__db.yml"), shallow=False)


def check_against_both(O, lib, tmp_path, cols, calls=None, budget=1 << 34, oracle=True, **cfg):
    got, info, nr = build(lib, str(tmp_path / "two"), cols, calls, budget, **cfg)
    one = lib.build_db(str(tmp_path / "one"), cols, **cfg)
    assert_same_files(got, one, whole=True)
    if oracle:
        rules = {k: cfg[k] for k in ("kmers_x", "block_size_x", "kmers_8", "kmers_1") if k in cfg}
        ref = O.build_db(str(tmp_path / "oracle"), O.sketch_cfg(k=cfg.get("k", 21)), cols, num_hashes=cfg.get("num_hashes", 1), fpr=cfg.get("fpr", 0.3),
                         threads=cfg.get("threads", 32), block_size=cfg.get("block_size", 0), rules=O.BlockRules(**rules) if rules else None)
        assert_same_files(got, ref)
    return got, info, nr


def matrix_of(path, num_sigs, row_bytes):
    raw = np.fromfile(path, dtype=np.uint8)
    return raw[len(raw) - num_sigs * row_bytes:].reshape(num_sigs, row_bytes)


@pytest.mark.parametrize("n_cols, block_size, row_bytes", [(1, 8, [1]), (7, 8, [1]), (8, 8, [1]), (9, 8, [1, 1]), (17, 8, [1, 1, 1]),
                                                           (9, 24, [2]), (17, 24, [3]), (40, 24, [3, 2])])
def test_bit_and_byte_edges(oracle_lib, tmp_path, n_cols, block_size, row_bytes):
    from kmcp_amd import lib
    cols = random_lists(np.random.default_rng(n_cols).integers(40, 300, size=n_cols), seed=500 + n_cols)
    got, info, _ = check_against_both(oracle_lib, lib, tmp_path, cols, block_size=block_size, num_hashes=2)
    odb = oracle_lib.OracleDB(got)
    try:
        assert [(odb.block_info(b)[1] + 7) // 8 for b in range(odb.nblocks)] == row_bytes
    finally:
        odb.close()


def test_eight_columns_race_for_every_byte(oracle_lib, tmp_path):
    """the same few thousand hashes in all eight columns of a block, one call: every touched byte is 0xFF"""
    from kmcp_amd import lib
    h = random_lists([3000], seed=510)[0][4]
    cols = [("same%d" % i, 5000, 0, 1, h) for i in range(8)]
    got, info, _ = check_against_both(oracle_lib, lib, tmp_path, cols, block_size=8, num_hashes=3)
    with lib.Builder(device=-1, block_size=8, num_hashes=3) as b:
        b.add_cols([(n, g, ci, nch, len(x)) for n, g, ci, nch, x in cols])
        assert b.plan(1 << 30) == (1, 1)
        bi = b.block_info(0)
    m = matrix_of(os.path.join(got, "_block001.uniki"), bi["num_sigs"], bi["row_bytes"])
    assert bi["row_bytes"] == 1 and set(np.unique(m).tolist()) == {0, 0xFF}
    assert 2000 < int((m == 0xFF).sum()) <= 3 * 3000
    assert info["scatter_launches"] == 1


@pytest.mark.parametrize("n_cols", [3, 12])
def test_first_and_last_row(oracle_lib, tmp_path, n_cols):
    """num_hashes 1: the hash is the row once reduced.  NumSigs - 1 and 2 NumSigs - 1 land on the last row, 0 and NumSigs on row 0"""
    from kmcp_amd import lib
    n = 200
    with lib.Builder(device=-1, block_size=16) as b:
        b.add_cols([("c", 1, 0, 1, n)] * n_cols)
        assert b.plan(1 << 30) == (1, 1)
        bi = b.block_info(0)
    ns = bi["num_sigs"]
    cols = random_lists([n] * n_cols, seed=520)
    edge = n_cols - 1  # the last column: the last byte of every row
    h = random_lists([n + 50], seed=521)[0][4]  # the others of the list land on neither row
    h = np.unique(np.concatenate([np.array([0, ns - 1, ns, 2 * ns - 1], dtype=np.uint64), h[(h % np.uint64(ns) != 0) & (h % np.uint64(ns) != ns - 1)]]))[:n]
    assert len(h) == n and list(h[:4]) == [0, ns - 1, ns, 2 * ns - 1]
    cols[edge] = cols[edge][:4] + (h,)
    got, _, _ = check_against_both(oracle_lib, lib, tmp_path, cols, block_size=16)
    m = matrix_of(os.path.join(got, "_block001.uniki"), ns, bi["row_bytes"])
    bit = 1 << (7 - edge % 8)
    assert m[0, edge // 8] & bit and m[ns - 1, edge // 8] & bit
    others = [c for c in range(n_cols) if c != edge and not (cols[c][4] % np.uint64(ns) == ns - 1).any()]
    for c in others:  # and nobody else's bit in the last row
        assert not m[ns - 1, c // 8] & (1 << (7 - c % 8)), c


def test_lists_around_a_waves_slice(oracle_lib, tmp_path):
    from kmcp_amd import lib
    with lib.Builder(device=-1) as b:
        S = b.info()["slice_keys"]
    assert S >= 128
    sizes = [0, 1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, S, 0, S, S, S]
    cols = random_lists(sizes, seed=530)
    # one call: the lists in order, an empty list between two full ones (columns 9 10 11), a skipped entry between two full ones (12 SKIP 13)
    call = list(range(12)) + [12, SKIP, 13]
    _, info, _ = check_against_both(oracle_lib, lib, tmp_path, cols, calls=[call], block_size=8, num_hashes=2)
    assert info["scatter_launches"] == 1 and info["lists_skipped"] == 1


@pytest.mark.parametrize("num_hashes", [1, 2, 3, 4])
def test_hash_functions(oracle_lib, tmp_path, num_hashes):
    from kmcp_amd import lib
    cols = random_lists(np.random.default_rng(7).integers(0, 1500, size=21), seed=540)
    check_against_both(oracle_lib, lib, tmp_path, cols, block_size=8, num_hashes=num_hashes, fpr=0.05)


@pytest.mark.parametrize("shape", ["one_call", "one_list_per_call", "blocks_interleaved", "reversed"])
def test_call_shapes(oracle_lib, tmp_path, shape):
    from kmcp_amd import lib
    n = 29
    cols = random_lists(np.random.default_rng(8).integers(1, 900, size=n), seed=550)  # 4 blocks of 8, 8, 8, 5 columns
    calls = {"one_call": None,                                              # lists of several blocks in one call
             "one_list_per_call": [[c] for c in range(n)],                  # the lists of one block spread over several calls
             "blocks_interleaved": [list(range(i, n, 5)) for i in range(5)],
             "reversed": [list(range(n - 1, 14, -1)), list(range(14, -1, -1))]}[shape]  # another order than the columns
    _, info, _ = check_against_both(oracle_lib, lib, tmp_path, cols, calls=calls, block_size=8, num_hashes=2)
    assert info["scatter_launches"] == (1 if calls is None else len(calls))


def test_rounds(oracle_lib, tmp_path):
    """equal columns: equal blocks.  A budget of exactly one block gives as many rounds as blocks, and the same files"""
    from kmcp_amd import lib
    cols = random_lists([150] * 24, seed=560)
    with lib.Builder(device=-1, block_size=8) as b:
        b.add_cols([(n, g, ci, nch, len(h)) for n, g, ci, nch, h in cols])
        assert b.plan(1 << 30) == (3, 1)
        one = b.block_info(0)["num_sigs"] * b.block_info(0)["row_bytes"] + 8
    calls = [list(range(0, 24, 2)), list(range(1, 24, 2))]
    all_dir, info_all, nr_all = build(lib, str(tmp_path / "all"), cols, calls, budget=3 * one, block_size=8)
    one_dir, info_one, nr_one = build(lib, str(tmp_path / "each"), cols, calls, budget=one, block_size=8)
    two_dir, info_two, nr_two = build(lib, str(tmp_path / "two"), cols, calls, budget=2 * one + 7, block_size=8)
    assert (nr_all, nr_one, nr_two) == (1, 3, 2)
    assert info_all["matrix_bytes_peak"] == 3 * one and info_one["matrix_bytes_peak"] == one and info_two["matrix_bytes_peak"] == 2 * one
    assert info_one["lists_skipped"] == 3 * 24 - 24 and info_all["lists_skipped"] == 0
    ref = oracle_lib.build_db(str(tmp_path / "oracle"), oracle_lib.sketch_cfg(k=21), cols, block_size=8)
    for d in (all_dir, one_dir, two_dir):
        assert_same_files(d, ref)
    assert_same_files(one_dir, all_dir, whole=True)
    with pytest.raises(lib.KmcpGpuError) as e:
        build(lib, str(tmp_path / "small"), cols, calls, budget=one - 1, block_size=8)
    assert "block 1 " in str(e.value) and str(one) in str(e.value) and str(one - 1) in str(e.value)
    assert not os.path.exists(tmp_path / "small")


def test_big_genome_tiers(oracle_lib, tmp_path):
    """the shape of tests/test_gpu_build.py::test_big_genome_block_rules, -X 16: blocks of 32, 16, 8 and 1 columns, in two rounds"""
    from kmcp_amd import lib
    O = oracle_lib
    base = synth.random_genomes(75, 9000, seed=81)
    lens = [1000] * 40 + [2200] * 20 + [4500] * 11 + [8000] * 4
    cols = synth.make_columns([g[:n] for g, n in zip(base, lens)], O.sketch_cfg(k=21))
    rules = dict(kmers_x=1500, block_size_x=16, kmers_8=3000, kmers_1=6000)
    got, info, nr = check_against_both(O, lib, tmp_path, cols, budget=40000, threads=2, block_size=32, **rules)
    assert len(_yml(os.path.join(got, "__db.yml"))["files"]) == 10 and nr >= 2


def test_uniform_sigs(oracle_lib, tmp_path):
    """the shape of tests/test_gpu_build.py::test_uniform_num_sigs_makes_blocks_groupable, mode 1 (not in the reference: the one-pass
    path is the reference here)"""
    from kmcp_amd import lib
    O = oracle_lib
    rng = np.random.default_rng(5)
    lens = rng.integers(3000, 9000, size=320)
    cols = synth.make_columns([g[:n] for g, n in zip(synth.random_genomes(320, 9000, seed=83), lens)], O.sketch_cfg(k=21))
    got, info, nr = check_against_both(O, lib, tmp_path, cols, oracle=False, threads=8, uniform_sigs=1)
    odb = O.OracleDB(got)
    try:
        assert odb.nblocks == 8 and len({odb.block_info(b)[0] for b in range(8)}) == 1
    finally:
        odb.close()


def test_refusals_leave_the_handle_usable(oracle_lib, tmp_path):
    from kmcp_amd import lib
    EINVAL = -1
    cols = random_lists([100, 200, 300, 0, 400, 500, 600, 700, 800, 900], seed=570)  # block_size 8: blocks of 8 and 1 columns
    out = str(tmp_path / "two")
    t, ptr, koff = on_device([c[4] for c in cols])
    ids = np.arange(len(cols), dtype=np.uint32)

    def refused(call, *words):
        with pytest.raises(lib.KmcpGpuError) as e:
            call()
        assert e.value.code == EINVAL, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    with lib.Builder(device=-1, block_size=8) as probe:  # a budget of exactly the larger block: two rounds
        probe.add_cols([(n, g, ci, nch, len(h)) for n, g, ci, nch, h in cols])
        assert probe.plan(1 << 30) == (2, 1)
        budget = max(probe.block_info(i)["num_sigs"] * probe.block_info(i)["row_bytes"] for i in range(2)) + 8
    with lib.Builder(device=0, block_size=8) as b:
        b.add_cols([(n, g, ci, nch, len(h)) for n, g, ci, nch, h in cols])
        assert b.plan(budget) == (2, 2)
        b.begin_round(0)
        # a list one key shorter than in pass 1: the column and both counts
        short = koff.copy()
        short[3:] -= 1  # column 2 loses a key
        refused(lambda: b.scatter_device(ptr, short, ids), "column 2 (c0002)", "299", "300")
        refused(lambda: b.scatter_device(ptr, koff[:3], np.array([0, 10], dtype=np.uint32)), "column 10 out of range")
        refused(lambda: b.scatter_device(ptr, koff[[0, 1, 1]], np.array([0, 0], dtype=np.uint32)), "column 0")  # 100 keys, then 0: the length differs
        t2, ptr2, koff2 = on_device([cols[1][4], cols[1][4]])
        refused(lambda: b.scatter_device(ptr2, koff2, np.array([1, 1], dtype=np.uint32)), "column 1 (c0001) given twice")
        assert b.info()["scatter_launches"] == 0 and b.info()["scatter_calls"] == 0  # refused before anything was launched
        b.scatter_device(ptr, koff[:6], ids[:5])           # columns 0 .. 4 (3 is empty)
        refused(lambda: b.scatter_device(ptr, koff[:3], ids[:2]), "given twice in round 0")
        refused(lambda: b.end_round(out), "was not scattered", "c000")
        assert not os.path.exists(out)                     # a block file is never written with a column missing
        refused(lambda: b.finish(out), "kmcpg_builder_finish out of order")
        t3, ptr3, koff3 = on_device([c[4] for c in cols[5:]])
        b.scatter_device(ptr3, koff3, ids[5:])
        b.end_round(out)
        refused(lambda: b.finish(out), "round 1 was never built", "kmcpg_builder_begin_round expected")
        refused(lambda: b.begin_round(0), "round 0 is built already")
        assert not os.path.exists(os.path.join(out, "R001", "__db.yml"))
        b.begin_round(1)
        b.scatter_device(ptr, koff, ids)
        b.end_round(out)
        got = b.finish(out)
        info = b.info()
        refused(lambda: b.begin_round(0), "out of order")
    assert info["scatter_launches"] == 3 and info["scatter_calls"] == 3 and info["rounds_done"] == 2
    ref = oracle_lib.build_db(str(tmp_path / "oracle"), oracle_lib.sketch_cfg(k=21), cols, block_size=8)
    assert_same_files(got, ref)
    assert_same_files(got, lib.build_db(str(tmp_path / "one"), cols, block_size=8), whole=True)
    del t, t2, t3
