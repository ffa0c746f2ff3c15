"""The short-read path of k2_cobs<64, 8, false, false, 4>: the bytes it asks the memory system for, to the byte.

An index with the row shape of a GTDB-scale block — 14 976 columns = 1 872-byte rows on a 1 920-byte pitch: two tiles of the 64-lane
class, 15 sectors of 128 bytes — in three blocks of different NumSigs (three groups), searched with planted and random reads at
profiling level 2, where the kernel counts its 16-byte row loads and 8-byte hash loads.  Neither count depends on timing, so every
assertion is an equality.

The reference is computed on the CPU from the rows the reads address, copied back from HBM (as tests/test_gpu_k2_forms.py takes its
counts): per (read, block, sector) the running maximum over the sector's columns of the match count after d rows, m[d], gives

    stop = the first d in 0..n with m[d] + (n - d) < cmin    (no column of the sector can reach the threshold any more), or n

which is the number of rows ANY correct algorithm has to see of that sector.  What each setting of the two knobs must then fetch:

    KMCPG_K2_EXACT_STOP=1                rows = stop
    KMCPG_K2_EXACT_STOP=0, BLOCK_UNITS=1 rows = min(n, stop rounded up to a multiple of 4): tests before every 4-row group
    both 0 (the plain form)              rows = stop rounded up to a multiple of 4, at least 4, past n where n is no multiple of 4:
                                         4-row groups with a test after each (the all-zero row stands in for rows past the end)
    KMCPG_K2_BLOCK_UNITS=1               hashes = 8 n bytes per (read, group)
    KMCPG_K2_BLOCK_UNITS=0, EXACT_STOP=1 hashes = 8 n bytes per (read, tile)
    both 0                               hashes per (read, tile) = 8 x the k-mers of the 64-k-mer chunks the wave entered: it leaves after
                                         the chunk in which its last sector stopped

That the plain form reproduces its row of this table is what shows the model itself to be right.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 21
COLS, BLOCKS, NUM_SIGS, SIGS_STEP = 14976, 3, 30011, 4099
PITCH, SECTORS, TILES = 1920, 15, 2          # 1 872 bytes of row on a 64-byte grid; whole sectors; 1 024 + 896 bytes
FORM = ("plain", 64, 0, 8, False, 4)
CAP = 1 << 18
N_RANDOM = 200
KNOBS = ("KMCPG_GROUP_ROWS", "KMCPG_PRUNE", "KMCPG_PRUNE_EVERY", "KMCPG_SLOT_MAJOR", "KMCPG_NT_LOADS", "KMCPG_SPLIT_MIN", "KMCPG_FPR_BOUND",
         "KMCPG_K2_BLOCK_UNITS", "KMCPG_K2_EXACT_STOP")


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


def _cmin(n, min_matched, min_qcov):
    return max(min_matched, int(np.floor(n * min_qcov)) + 1)  # csa.hpp count_threshold


def _stops(bits, n, cmin):
    """bits: [n, SECTORS * 1024] 0/1 of one (read, block); -> per sector the first d with max count + rows left < cmin, else n"""
    run = np.zeros((n + 1, SECTORS), dtype=np.int64)
    run[1:] = np.cumsum(bits, axis=0, dtype=np.int16).reshape(n, SECTORS, 1024).max(axis=2)
    dead = run + (n - np.arange(n + 1))[:, None] < cmin
    return np.where(dead.any(axis=0), dead.argmax(axis=0), n)


@pytest.fixture(scope="module")
def state(oracle_lib):
    import torch
    from kmcp_amd import Database, default_params, lib
    O = oracle_lib
    rng = np.random.default_rng(20261017)
    kpc = int(round(-np.log(1.0 - 0.3) * NUM_SIGS))  # Bloom density 0.3, the FPR the benchmark's indexes are built with
    spec = lib.SynthSpec(k=K, num_hashes=1, fpr=0.3, n_blocks=BLOCKS, cols_per_block=COLS, num_sigs=NUM_SIGS, kmers_per_col=kpc, seed=77,
                         sigs_step=SIGS_STEP)
    with _Env({k: None for k in ("KMCPG_ROW_ALIGN", "KMCPG_LPR32", "KMCPG_LPR8", "KMCPG_SPLIT_TILES", "KMCPG_FUSE")}):
        db = Database.open_synthetic(spec)
    try:
        assert [db.block_info(b)["stride"] for b in range(BLOCKS)] == [PITCH] * BLOCKS
        assert len({db.block_info(b)["num_sigs"] for b in range(BLOCKS)}) == BLOCKS
        # reads: 150 bp (130 k-mers: 32 groups of 4 and 2 rows) for the most part; other lengths for n = 4 j, n below one group, n below
        # min_matched (not searched) and a read shorter than k
        lens = [150] * N_RANDOM + [151, 152, 153, 149, 100, 84, 36, 33, 23, 22, 20]
        lens = np.array(lens, dtype=np.int64)[rng.permutation(len(lens))]
        offs = np.zeros(len(lens) + 1, dtype=np.int64)
        offs[1:] = np.cumsum(lens)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offs[-1]))]
        cfg = O.sketch_cfg(k=K)
        kms = [O.generate_kmers(seq[offs[i]:offs[i + 1]].tobytes(), cfg) for i in range(len(lens))]
        params = default_params(min_qlen=0, dedup_threshold=1 << 30)  # min_matched 10, min_qcov 0.55: cmin = 72 of 130
        ns = np.array([len(k) for k in kms], dtype=np.int64)
        assert ns.tolist() == np.maximum(lens - K + 1, 0).tolist()
        # plants, round-robin over columns at the edges of blocks, tiles and sectors and in the 640-column last sector: whole reads (the
        # sector never stops), the last cmin and cmin - 1 k-mers (a hit and a near miss decided by the last row), the first cmin - 1
        # and the first 40 (a column that leads early and is lost)
        cols = [0, 1023, 1024, 8191, 8192, 14335, 14336, COLS - 1, COLS, COLS + 5000, 2 * COLS - 1, 2 * COLS + 8191, 2 * COLS + 8192, 3 * COLS - 1]
        planted = [i for i in range(len(lens)) if ns[i] >= 100][:5 * len(cols)]
        for j, i in enumerate(planted):
            n, km, c = int(ns[i]), kms[i], cols[j % len(cols)]
            cm = _cmin(n, params.min_matched, params.min_qcov)
            db.plant(c, {0: km, 1: km[n - cm:], 2: km[n - cm + 1:], 3: km[:cm - 1], 4: km[:40]}[j // len(cols)])
        # the model, from the rows as they are now
        searched = np.where(ns >= params.min_matched, ns, 0)
        stop = np.zeros((len(lens), BLOCKS, SECTORS), dtype=np.int64)
        hits = 0
        for b in range(BLOCKS):
            nsig = np.uint64(db.block_info(b)["num_sigs"])
            rows = db.read_rows(b, np.concatenate(kms) % nsig)
            pad = np.zeros((rows.shape[0], SECTORS * 128), dtype=np.uint8)
            pad[:, :rows.shape[1]] = rows
            at = 0
            for i, km in enumerate(kms):
                n = len(km)
                if searched[i]:
                    bits = np.unpackbits(pad[at:at + n], axis=1)
                    cm = _cmin(n, params.min_matched, params.min_qcov)
                    stop[i, b] = _stops(bits, n, cm)
                    hits += int((bits.sum(axis=0) >= cm).sum())
                at += n
        dev = torch.device("cuda:0")
        db.set_profiling(2)
        st = dict(db=db, torch=torch, params=params, ns=searched, stop=stop, hits=hits, n_reads=len(lens), total=int(offs[-1]), maxlen=int(lens.max()),
                  seq=torch.from_numpy(seq.copy()).to(dev), offs=torch.from_numpy(offs).to(dev))
        yield st
    finally:
        db.close()


def _run(st, block_units, exact_stop):
    torch, db, n = st["torch"], st["db"], st["n_reads"]
    dev = st["seq"].device
    hits = torch.zeros((CAP, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    qk = torch.zeros(n, dtype=torch.int32, device=dev)
    ql = torch.zeros(n, dtype=torch.int32, device=dev)
    env = dict({k: None for k in KNOBS}, KMCPG_GROUP_ROWS="4", KMCPG_FPR_BOUND="0", KMCPG_K2_BLOCK_UNITS=block_units, KMCPG_K2_EXACT_STOP=exact_stop)
    with _Env(env):
        db.query_device(st["seq"].data_ptr(), st["offs"].data_ptr(), n, st["total"], st["maxlen"], hits.data_ptr(), CAP, cnt.data_ptr(), qk.data_ptr(),
                        ql.data_ptr(), params=st["params"])
        torch.cuda.synchronize()
    assert np.array_equal(qk.cpu().numpy(), st["ns"].astype(np.int32))
    h = hits[:int(cnt[0].item())].to(torch.int64).cpu().numpy()
    order = np.lexsort((h[:, 1], h[:, 0]))
    return db.last_gathered_bytes(), db.last_hash_bytes(), [w[:6] for w in db.last_k2_launches()], h[order]


def _model(st, block_units, exact_stop):
    ns, stop = st["ns"], st["stop"]
    n3 = ns[:, None, None]
    up4 = (stop + 3) // 4 * 4
    if exact_stop:
        rows = stop
    elif block_units:
        rows = np.minimum(n3, up4)
    else:
        rows = np.maximum(up4, 4)
    rows = np.where(n3 > 0, rows, 0)
    if block_units:
        hashes = 8 * BLOCKS * int(ns.sum())
    elif exact_stop:
        hashes = 8 * BLOCKS * TILES * int(ns.sum())
    else:
        hashes = 0
        for lo, hi in ((0, 8), (8, SECTORS)):  # the sectors of the two tiles
            last = rows[:, :, lo:hi].max(axis=2)
            hashes += 8 * int(np.minimum(ns[:, None], (last + 63) // 64 * 64).sum())
    return 128 * int(rows.sum()), hashes


@pytest.mark.parametrize("block_units,exact_stop", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["plain", "block-units", "exact-stop", "both"])
def test_bytes_fetched(state, block_units, exact_stop):
    got_rows, got_hashes, launches, hits = _run(state, block_units, exact_stop)
    want_rows, want_hashes = _model(state, block_units, exact_stop)
    floor_rows = 128 * int(np.where(state["ns"][:, None, None] > 0, state["stop"], 0).sum())
    print("block_units %d exact_stop %d: row bytes %d (model %d, floor %d: x %.4f), hash bytes %d (model %d), %d hits" % (
        block_units, exact_stop, got_rows, want_rows, floor_rows, got_rows / floor_rows, got_hashes, want_hashes, len(hits)))
    assert launches == [FORM]
    assert got_rows == want_rows
    assert got_hashes == want_hashes
    assert len(hits) == state["hits"] > 0
    if exact_stop:
        assert got_rows == floor_rows  # nothing is fetched that the bound does not prove necessary


def test_same_hits_under_every_setting(state):
    """(read, column, count) of every hit: the four settings differ in what they fetch, not in what they find"""
    ref = _run(state, 0, 0)[3]
    for bu, es in ((1, 0), (0, 1), (1, 1)):
        assert np.array_equal(_run(state, bu, es)[3], ref), (bu, es)
