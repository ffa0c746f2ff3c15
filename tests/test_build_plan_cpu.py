"""The block layout as a function of the k-mer counts (kmcp_amd/csrc/build_plan.hpp), without a GPU: a planning-only kmcpg_builder
(device -1) must place every column where the oracle's restatement of index.go:787-894 places it (oracle.block_layout), size every
block as CalcSignatureSize does, follow the uniform_sigs rules as restated here, and cut the blocks into rounds as
the ten lines of rounds_of() do; every call out of order is refused by name.  tests/build_plan_check.cpp compiles the same header with
g++ -Wall -Werror (no HIP in it) and is run on the same cases."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = dict(kmers_x=1500, kmers_8=3000, kmers_1=6000)  # the scaled-down thresholds of tests/test_gpu_build.py::test_big_genome_block_rules


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from kmcp_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    lib.load().kmcpg_builder_open  # the symbol this file is about
    return lib


def cases():
    """(counts, cfg) — cfg as the keyword arguments of lib.Builder"""
    rng = np.random.default_rng(20)
    out = []
    for n in [1, 2, 7, 8, 9, 17, 40, 64, 100, 257, 600, 3000]:
        for style in range(4):
            if style == 0:    # anything, zeros included
                counts = rng.integers(0, 5000, size=n) * (rng.random(n) > 0.1)
            elif style == 1:  # few distinct values: the tie order decides
                counts = rng.choice([0, 3, 3, 50, 50, 50, 700], size=n)
            elif style == 2:  # four size classes around the tier thresholds, -X below -b
                counts = rng.choice([0, 1, 900, 1500, 1501, 2999, 3000, 3001, 6000, 6001, 9000], size=n)
            else:             # the same with -X above -b: the -x tier does not exist
                counts = rng.integers(0, 9000, size=n)
            cfg = dict(num_hashes=int(rng.integers(1, 5)), fpr=float(rng.choice([0.3, 0.05, 0.01])), uniform_sigs=int(rng.integers(0, 3)))
            if style < 2:
                cfg.update(threads=int(rng.choice([1, 2, 8, 32])), block_size=int(rng.choice([0, 0, 8, 24])))
            else:
                cfg.update(threads=2, block_size=32, block_size_x=16 if style == 2 else 256, **TIERS)
            out.append((counts.astype(np.uint64), cfg))
    return out


def expected(O, counts, cfg):
    """-> (block of every column (-1: none), place in the block, NumSigs per block)"""
    n = len(counts)
    order = np.argsort(counts, kind="stable")  # ascending, input order breaks ties
    bs, th = cfg.get("block_size", 0), max(1, cfg.get("threads", 32))
    sblock = bs if bs > 0 else (int(n / th) + 7) // 8 * 8
    sblock = max(8, min(sblock, n))
    rules = O.BlockRules(kmers_x=cfg.get("kmers_x", 0), block_size_x=cfg.get("block_size_x", 0), kmers_8=cfg.get("kmers_8", 0), kmers_1=cfg.get("kmers_1", 0))
    nb, blk = O.block_layout(counts[order], sblock, rules)
    block = np.full(n, -1, dtype=np.int64)
    pos = np.full(n, -1, dtype=np.int64)
    fill = [0] * nb
    biggest = [0] * nb
    for i, c in enumerate(order):
        if blk[i]:
            b = int(blk[i]) - 1
            block[c], pos[c] = b, fill[b]
            fill[b] += 1
            biggest[b] = max(biggest[b], int(counts[c]))
    sigs = [int(O.lib().ko_calc_signature_size(m, cfg["num_hashes"], cfg["fpr"])) for m in biggest]
    # uniform_sigs, restated: per size tier, 1 = the tier's largest NumSigs, 2 = a 5/4 ladder above the tier's smallest, capped at the largest
    if cfg["uniform_sigs"]:
        kx, k8, k1 = (cfg.get(k) or d << 20 for k, d in (("kmers_x", 10), ("kmers_8", 20), ("kmers_1", 200)))
        skip_x = (cfg.get("block_size_x") or 256) >= sblock
        tier = [3 if m > k1 else 2 if m > k8 else 1 if (m > kx and not skip_x) else 0 for m in biggest]
        # a block's tier is that of any of its columns; the smallest decides no differently than the fullest
        for t in range(4):
            mine = [b for b in range(nb) if tier[b] == t]
            if not mine:
                continue
            lo, hi = min(sigs[b] for b in mine), max(sigs[b] for b in mine)
            for b in mine:
                if cfg["uniform_sigs"] == 1:
                    sigs[b] = hi
                else:
                    step = lo
                    while step < sigs[b]:
                        step = step + step // 4 + 1
                    sigs[b] = min(step, hi)
    return block, pos, sigs, fill


def rounds_of(matrix_bytes, budget):
    """blocks in file order; a round closes when the next block's matrix_bytes + 8 would exceed the budget; None: a block above it"""
    rounds, used, r = [], 0, 0
    for mb in matrix_bytes:
        if mb + 8 > budget:
            return None
        if used and used + mb + 8 > budget:
            r, used = r + 1, 0
        used += mb + 8
        rounds.append(r)
    return rounds


def budgets_of(matrix_bytes):
    """from "one block" to "all blocks", and one byte below the largest block"""
    big, total = max(matrix_bytes) + 8, sum(matrix_bytes) + 8 * len(matrix_bytes)
    return [big, (big + total) // 2, total, total + 1000, big - 1]


def planned(lib, counts, cfg, budget):
    b = lib.Builder(device=-1, **cfg)
    b.add_cols([("c%d" % i, 100, 0, 1, int(c)) for i, c in enumerate(counts)])
    return b, b.plan(budget)


def test_layout_equals_oracle(built, oracle_lib):
    lib, O = built, oracle_lib
    checked_blocks = 0
    for counts, cfg in cases():
        block, pos, sigs, fill = expected(O, counts, cfg)
        if not sigs:  # nothing but empty columns: no block, no round
            b, (nb, nr) = planned(lib, counts, cfg, 1 << 40)
            assert (nb, nr) == (0, 0)
            assert all(b.col_place(c) == (b.NO_BLOCK,) * 3 for c in range(len(counts)))
            b.close()
            continue
        mbytes = [s * ((f + 7) // 8) for s, f in zip(sigs, fill)]
        for budget in budgets_of(mbytes):
            want = rounds_of(mbytes, budget)
            if want is None:
                b = lib.Builder(device=-1, **cfg)
                b.add_cols([("c%d" % i, 100, 0, 1, int(c)) for i, c in enumerate(counts)])
                with pytest.raises(lib.KmcpGpuError) as e:
                    b.plan(budget)
                big = mbytes.index(max(mbytes))
                assert "block %d " % (big + 1) in str(e.value) and str(max(mbytes) + 8) in str(e.value) and str(budget) in str(e.value), str(e.value)
                b.close()
                continue
            b, (nb, nr) = planned(lib, counts, cfg, budget)
            assert nb == len(sigs) and nr == want[-1] + 1, (cfg, budget)
            for bi in range(nb):
                assert b.block_info(bi) == dict(num_sigs=sigs[bi], n_cols=fill[bi], row_bytes=(fill[bi] + 7) // 8, round=want[bi]), (cfg, bi)
            if budget == budgets_of(mbytes)[0]:  # the columns' places do not depend on the budget: once per case
                for c in range(len(counts)):
                    got = b.col_place(c)
                    if block[c] < 0:
                        assert got == (b.NO_BLOCK,) * 3
                    else:
                        assert got == (block[c], pos[c], want[block[c]]), (cfg, c)
            checked_blocks += nb
            b.close()
    assert checked_blocks > 1000


def test_call_order_is_enforced_by_name(built, tmp_path):
    lib = built
    b = lib.Builder(device=-1, block_size=8)

    def refused(call, code, *words):
        with pytest.raises(lib.KmcpGpuError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    EINVAL, EDEVICE = -1, -4
    koff, cols = np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    # nothing but add_cols and plan before the plan, and plan needs a column
    refused(lambda: b.plan(1 << 30), EINVAL, "kmcpg_builder_add_cols expected")
    refused(lambda: b.col_place(0), EINVAL, "kmcpg_builder_col_place out of order", "kmcpg_builder_plan expected")
    refused(lambda: b.block_info(0), EINVAL, "kmcpg_builder_plan expected")
    refused(lambda: b.begin_round(0), EINVAL, "kmcpg_builder_begin_round out of order", "kmcpg_builder_plan expected")
    refused(lambda: b.scatter_device(0, koff, cols), EINVAL, "kmcpg_builder_plan expected")
    refused(lambda: b.end_round(str(tmp_path)), EINVAL, "kmcpg_builder_plan expected")
    refused(lambda: b.finish(str(tmp_path)), EINVAL, "kmcpg_builder_plan expected")
    b.add_cols([("a", 10, 0, 2, 5)])
    b.add_cols([("a", 10, 1, 2, 7), ("empty", 10, 0, 1, 0)])
    refused(lambda: b.plan(0), EINVAL, "explicit matrix_budget")  # a planning-only builder has no HBM to ask
    assert b.plan(1 << 30) == (1, 1)
    # after the plan: no more columns, no second plan; rounds are expected
    refused(lambda: b.add_cols([("x", 1, 0, 1, 1)]), EINVAL, "kmcpg_builder_add_cols out of order", "kmcpg_builder_begin_round expected")
    refused(lambda: b.plan(1 << 30), EINVAL, "kmcpg_builder_begin_round expected")
    refused(lambda: b.scatter_device(0, koff, cols), EINVAL, "kmcpg_builder_begin_round expected")
    refused(lambda: b.end_round(str(tmp_path)), EINVAL, "kmcpg_builder_begin_round expected")
    refused(lambda: b.finish(str(tmp_path)), EINVAL, "kmcpg_builder_begin_round expected")
    refused(lambda: b.col_place(3), EINVAL, "column 3 out of range")
    refused(lambda: b.block_info(1), EINVAL, "block 1 out of range")
    refused(lambda: b.begin_round(1), EINVAL, "round 1 out of range")
    refused(lambda: b.begin_round(0), EDEVICE, "planning-only")
    assert not os.path.exists(tmp_path / "R001")
    assert b.col_place(2) == (b.NO_BLOCK,) * 3 and b.col_place(0) == (0, 0, 0) and b.col_place(1) == (0, 1, 0)
    info = b.info()
    assert info["rounds_done"] == 0 and info["scatter_calls"] == 0 and info["slice_keys"] >= 64
    b.close()
    # the configuration is validated at open, reserved fields included
    refused(lambda: lib.Builder(device=-1, num_hashes=5), EINVAL)
    refused(lambda: lib.Builder(device=-1, fpr=1.0), EINVAL)
    cfg = lib.BuilderCfg()
    cfg.build = lib.BuildCfg(k=21, canonical=1, num_hashes=1, fpr=0.3)
    cfg.reserved[1] = 1
    import ctypes as C
    h = C.c_void_p()
    assert lib.load().kmcpg_builder_open(C.byref(cfg), -1, C.byref(h)) == EINVAL and b"reserved" in lib.load().kmcpg_last_error()
    # a plan the thresholds forbid is refused as kmcpg_build_db refuses it
    b = lib.Builder(device=-1, kmers_x=5000, kmers_8=3000, kmers_1=6000)
    b.add_cols([("a", 10, 0, 1, 5)])
    refused(lambda: b.plan(1 << 30), EINVAL, "-x < -8 < -1")
    b.close()


def test_header_compiles_for_the_host_and_agrees(built, oracle_lib, tmp_path):
    O = oracle_lib
    exe, path = str(tmp_path / "build_plan_check"), str(tmp_path / "cases.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "build_plan_check.cpp"),
                    os.path.join(ROOT, "kmcp_amd", "csrc", "fpr.cpp")], check=True)
    total = 0
    with open(path, "w") as fh:
        for counts, cfg in cases():
            block, pos, sigs, fill = expected(O, counts, cfg)
            mbytes = [s * ((f + 7) // 8) for s, f in zip(sigs, fill)]
            for budget in (budgets_of(mbytes) if sigs else [1 << 40]):
                want = rounds_of(mbytes, budget)
                fh.write("%d %d %d %d %d %d %d %d %d %r %d\n" % (len(counts), cfg.get("threads", 32), cfg.get("block_size", 0), cfg.get("kmers_x", 0),
                                                                 cfg.get("block_size_x", 0), cfg.get("kmers_8", 0), cfg.get("kmers_1", 0),
                                                                 cfg["uniform_sigs"], cfg["num_hashes"], cfg["fpr"], budget))
                fh.write(" ".join(str(int(c)) for c in counts) + "\n")
                fh.write("%d %d\n" % (len(sigs), -1 if want is None else (want[-1] + 1 if want else 0)))
                fh.write(" ".join("%d %d" % (b, p) for b, p in zip(block, pos)) + "\n")
                fh.write(" ".join("%d %d" % (s, 0 if want is None else want[i]) for i, s in enumerate(sigs)) + "\n")
                total += 1
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("%d cases, 0 wrong" % total) and total > 200, r.stdout
