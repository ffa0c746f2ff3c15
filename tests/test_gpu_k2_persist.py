"""The persistent short-read COBS kernel (k2_cobs.hip k2_cobs_persist, KMCPG_K2_PERSIST): resident waves that take their (read, slot)
units from a queue, eight at a time, until it is dry.  Hits and bytes, to the byte, on every grid.

The index has the shape of tests/test_gpu_k2_exact_stop.py — three blocks of 14 976 columns and different NumSigs, 1 872-byte rows on
a 1 920-byte pitch: two tiles, 15 sectors, six slots — and the reference is that test's: the rows the reads address are copied back
from HBM and counted on the CPU.  Per (read, block, sector) the running maximum of the columns' counts gives the row at which the
sector can no longer reach the threshold (`stop`), per (read, column) the count gives the hits.  What a batch must then fetch:

    short reads (the persistent kernel)   rows = 128 B x stop per sector; hashes = 8 n B per (read, tile)
    reads above KMCPG_SPLIT_MIN           (left to the chunked launch behind it, which does not prune) every sector's rows up to the
                                          next multiple of 8 per chunk of 1 024 k-mers; hashes = 8 n B per (read, tile)

Nothing is compared with a run of the launched form: KMCPG_K2_PERSIST=0 is one more case held against the same model, which is what
shows the model (its chunked part included) to be right.  Two batches: 8 planes (n up to 254: 0, 1, 3, 4, 5, 129-131 and 254 among
130s, three reads of 400 k-mers in between) and 10 planes (255 and 1 022 among others, two reads of 1 500).  151 and 41 reads on six
slots: 906 and 246 units, neither a multiple of the claim run of 8, no slot boundary on a multiple of 8 either (claims straddle
them), and fewer units than the default grid has waves.  KMCPG_K2_PERSIST_WGS=1 is one workgroup over every unit — hundreds of units
and every slot change inside a wave; 3 is a grid that is no divisor of anything; 4 096 has waves that find the queue dry at once.
Two thresholds: the default (0.55: unrelated sectors stop early) and 0.36, in the body of the count distribution (mean 0.3 n), where
thousands of hits come in runs and few sectors stop.

The witness of the kernel that ran is the record's grid (`Database.last_k2_grids()`): the launched form runs on the piece's
workgroups, the persistent kernel on the grid it was given — KMCPG_K2_PERSIST_WGS, or what the chip holds at once, cut to the piece.
Both batches are smaller than a chip, so a third one, p8 nineteen times over (BIG), has a piece no chip holds at once: there the
default grid must be smaller than the piece."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 21
COLS, BLOCKS, NUM_SIGS, SIGS_STEP = 14976, 3, 30011, 4099
PITCH, SECTORS, TILES = 1920, 15, 2
CAP = 1 << 21
CLAIM_RUN = 8  # k2_claim.hpp K2_CLAIM_RUN
QCOVS = (0.55, 0.36)
# A piece larger than any chip's fill: a workgroup is four waves, a SIMD holds at most 10 (8 on gfx950), so a CU holds at most 10
# workgroups of this kernel and 16 is beyond any; 256 CUs is the MI355X, and 16 x 256 = 4 096 also exceeds 10 x the 304 CUs of the
# largest CDNA part.  p8 x 19 = 2 869 reads on six slots: 17 214 units, 4 304 workgroups.  (Its hits, 19 x 41 365, fit CAP.)
BIG, BIG_REP, CHIP_WORKGROUPS = "p8x19", 19, 16 * 256
KNOBS = ("KMCPG_GROUP_ROWS", "KMCPG_PRUNE", "KMCPG_PRUNE_EVERY", "KMCPG_SLOT_MAJOR", "KMCPG_NT_LOADS", "KMCPG_SPLIT_MIN", "KMCPG_SPLIT_CHUNK",
         "KMCPG_FPR_BOUND", "KMCPG_K2_BLOCK_UNITS", "KMCPG_K2_EXACT_STOP", "KMCPG_K2_PERSIST", "KMCPG_K2_PERSIST_WGS")
# batch -> (planes, KMCPG_SPLIT_MIN, k-mers per read in batch order)
BATCHES = {
    "p8": (8, 254, [130] * 20 + [0, 1, 3, 4, 5] + [130] * 30 + [400] + [129, 130, 131, 254] + [130] * 40 + [400, 400] + [254, 1, 130] + [130] * 46),
    "p10": (10, 1022, [130] * 8 + [255, 1022, 0, 1] + [1500] + [300, 700, 130, 1022] + [130] * 10 + [1500] + [255, 5, 4] + [130] * 10),
}


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


def _stops(run, n, cmin):
    """run: [n + 1, SECTORS] largest count of a sector's columns after d rows -> the first d with run[d] + rows left < cmin, else n"""
    dead = run + (n - np.arange(n + 1))[:, None] < cmin
    return np.where(dead.any(axis=0), dead.argmax(axis=0), n)


@pytest.fixture(scope="module")
def state(oracle_lib):
    import torch
    from kmcp_amd import Database, default_params, lib
    O = oracle_lib
    rng = np.random.default_rng(20261020)
    kpc = int(round(-np.log(1.0 - 0.3) * NUM_SIGS))  # Bloom density 0.3, as the benchmark's indexes
    spec = lib.SynthSpec(k=K, num_hashes=1, fpr=0.3, n_blocks=BLOCKS, cols_per_block=COLS, num_sigs=NUM_SIGS, kmers_per_col=kpc, seed=78,
                         sigs_step=SIGS_STEP)
    with _Env({k: None for k in ("KMCPG_ROW_ALIGN", "KMCPG_LPR32", "KMCPG_LPR8", "KMCPG_SPLIT_TILES", "KMCPG_FUSE")}):
        db = Database.open_synthetic(spec)
    try:
        assert [db.block_info(b)["stride"] for b in range(BLOCKS)] == [PITCH] * BLOCKS
        assert len({db.block_info(b)["num_sigs"] for b in range(BLOCKS)}) == BLOCKS
        cfg = O.sketch_cfg(k=K)
        dev = torch.device("cuda:0")
        batches = {}
        for name, (npl, split_min, want_n) in BATCHES.items():
            lens = np.array([n + K - 1 if n else K - 1 for n in want_n], dtype=np.int64)
            offs = np.zeros(len(lens) + 1, dtype=np.int64)
            offs[1:] = np.cumsum(lens)
            seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offs[-1]))]
            kms = [O.generate_kmers(seq[offs[i]:offs[i + 1]].tobytes(), cfg) for i in range(len(lens))]
            assert [len(k) for k in kms] == want_n
            units = len(lens) * BLOCKS * TILES
            assert units % CLAIM_RUN != 0 and len(lens) % CLAIM_RUN != 0 and units < 4 * ((units + 3) // 4)
            batches[name] = dict(npl=npl, split_min=split_min, kms=kms, ns=np.array(want_n, dtype=np.int64), n_reads=len(lens), total=int(offs[-1]),
                                 maxlen=int(lens.max()), seq=torch.from_numpy(seq.copy()).to(dev), offs=torch.from_numpy(offs).to(dev))
        # plants at the edges of blocks, tiles and sectors: whole reads (a sector that never stops, a hit with count n) and the first
        # 40 k-mers (a column that leads early and is lost under the default threshold)
        cols = [0, 1023, 1024, 8191, 8192, 14335, 14336, COLS - 1, COLS, COLS + 5000, 2 * COLS - 1, 2 * COLS + 8191, 2 * COLS + 8192, 3 * COLS - 1]
        j = 0
        for bt in batches.values():
            for i, km in enumerate(bt["kms"]):
                if len(km) >= 100 and i % 3 == 0:
                    db.plant(cols[j % len(cols)], km if (j // len(cols)) % 2 == 0 else km[:40])
                    j += 1
        # the model's inputs, from the rows as they are now: per (read, block) the sectors' running maxima, per read every column's count
        for bt in batches.values():
            kms = bt["kms"]
            bt["run"] = [[None] * BLOCKS for _ in kms]
            bt["counts"] = [np.zeros(BLOCKS * COLS, dtype=np.int32) for _ in kms]
            for b in range(BLOCKS):
                nsig = np.uint64(db.block_info(b)["num_sigs"])
                rows = db.read_rows(b, np.concatenate(kms) % nsig)
                pad = np.zeros((rows.shape[0], SECTORS * 128), dtype=np.uint8)
                pad[:, :rows.shape[1]] = rows
                at = 0
                for i, km in enumerate(kms):
                    n = len(km)
                    if n:
                        cum = np.cumsum(np.unpackbits(pad[at:at + n], axis=1), axis=0, dtype=np.int16)
                        run = np.zeros((n + 1, SECTORS), dtype=np.int64)
                        run[1:] = cum.reshape(n, SECTORS, 1024).max(axis=2)
                        bt["run"][i][b] = run
                        bt["counts"][i][b * COLS:(b + 1) * COLS] = cum[-1, :COLS]
                    at += n
        # BIG: the reads of p8 BIG_REP times over — the model's inputs are p8's, read for read
        src = batches["p8"]
        lens = np.diff(src["offs"].cpu().numpy())
        offs = np.zeros(BIG_REP * len(lens) + 1, dtype=np.int64)
        offs[1:] = np.cumsum(np.tile(lens, BIG_REP))
        big = dict(src, kms=src["kms"] * BIG_REP, ns=np.tile(src["ns"], BIG_REP), n_reads=BIG_REP * src["n_reads"], total=int(offs[-1]),
                   seq=src["seq"].repeat(BIG_REP), offs=torch.from_numpy(offs).to(dev), run=src["run"] * BIG_REP, counts=src["counts"] * BIG_REP)
        units = big["n_reads"] * BLOCKS * TILES
        assert units % CLAIM_RUN != 0 and big["n_reads"] % CLAIM_RUN != 0 and (units + 3) // 4 > CHIP_WORKGROUPS
        batches[BIG] = big
        db.set_profiling(2)
        yield dict(db=db, torch=torch, default_params=default_params, batches=batches)
    finally:
        db.close()


def _model(bt, qcov):
    """-> (row bytes, hash bytes, hits [(read, column, count)] in (read, column) order)"""
    rows = hashes = 0
    hits = []
    for i, n in enumerate(bt["ns"].tolist()):
        if n == 0:
            continue
        cm = _cmin(n, 1, qcov)
        hashes += 8 * BLOCKS * TILES * n
        if n > bt["split_min"]:  # the chunked form: no pruning, 8-row groups, chunks of 1 024 k-mers
            rows += BLOCKS * SECTORS * 128 * sum((min(1024, n - k0) + 7) // 8 * 8 for k0 in range(0, n, 1024))
        else:
            rows += 128 * sum(int(_stops(bt["run"][i][b], n, cm).sum()) for b in range(BLOCKS))
        c = bt["counts"][i]
        col = np.nonzero(c >= cm)[0]
        hits.append(np.stack([np.full(len(col), i, dtype=np.int64), col, c[col].astype(np.int64)], axis=1))
    return rows, hashes, np.concatenate(hits)


def _run(st, bt, qcov, persist, wgs):
    torch, db, n = st["torch"], st["db"], bt["n_reads"]
    dev = bt["seq"].device
    hits = torch.zeros((CAP, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    qk = torch.zeros(n, dtype=torch.int32, device=dev)
    ql = torch.zeros(n, dtype=torch.int32, device=dev)
    params = st["default_params"](min_qlen=0, dedup_threshold=1 << 30, min_matched=1, min_qcov=qcov)
    env = dict({k: None for k in KNOBS}, KMCPG_GROUP_ROWS="4", KMCPG_FPR_BOUND="0", KMCPG_SPLIT_MIN=bt["split_min"], KMCPG_K2_PERSIST=persist,
               KMCPG_K2_PERSIST_WGS=wgs)
    with _Env(env):
        db.query_device(bt["seq"].data_ptr(), bt["offs"].data_ptr(), n, bt["total"], bt["maxlen"], hits.data_ptr(), CAP, cnt.data_ptr(), qk.data_ptr(),
                        ql.data_ptr(), params=params)
        torch.cuda.synchronize()
    assert np.array_equal(qk.cpu().numpy(), bt["ns"].astype(np.int32))
    assert int(cnt[0].item()) <= CAP
    h = hits[:int(cnt[0].item())].to(torch.int64).cpu().numpy()
    launches, grids = db.last_k2_launches(), db.last_k2_grids()
    assert len(grids) == len(launches)
    return db.last_gathered_bytes(), db.last_hash_bytes(), launches, grids, h[np.lexsort((h[:, 1], h[:, 0]))]


def _check(st, name, qcov, persist, wgs):
    bt = st["batches"][name]
    got_rows, got_hashes, launches, grids, hits = _run(st, bt, qcov, persist, wgs)
    want_rows, want_hashes, want_hits = _model(bt, qcov)
    print("%s qcov %.2f persist %s wgs %s: row bytes %d (model %d), hash bytes %d (model %d), %d hits (model %d), launches %s, grids %s" % (
        name, qcov, persist, wgs, got_rows, want_rows, got_hashes, want_hashes, len(hits), len(want_hits), launches, grids))
    assert len(want_hits) > 0
    assert np.array_equal(hits, want_hits)
    assert got_rows == want_rows
    assert got_hashes == want_hashes
    # every launch but the persistent one (the first record, where there is one) runs on its piece's workgroups
    assert [g for g in grids[1:]] == [w[6] for w in launches[1:]]
    return launches, grids


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_model_holds_for_the_launched_form(state, name):
    """one unit per wave, as launched (KMCPG_K2_PERSIST=0): the same model, and the record every persistent run must leave too"""
    bt = state["batches"][name]
    launches, grids = _check(state, name, QCOVS[0], 0, None)
    units = bt["n_reads"] * BLOCKS * TILES
    assert launches[0] == ("plain", 64, 0, bt["npl"], False, 4, (units + 3) // 4)
    assert [w[0] for w in launches[1:]] == ["split"]
    assert grids[0] == launches[0][6]  # one wave per unit: the launched form
    state.setdefault("witness", {})[name] = launches


@pytest.mark.parametrize("wgs", [None, 1, 3, 4096], ids=["resident", "one-workgroup", "three-workgroups", "more-waves-than-units"])
@pytest.mark.parametrize("qcov", QCOVS, ids=["stops", "runs-of-hits"])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_persistent_waves(state, name, qcov, wgs):
    bt = state["batches"][name]
    launches, grids = _check(state, name, qcov, 1, wgs)
    units = bt["n_reads"] * BLOCKS * TILES
    # the witness names the plan's piece, whatever grid its waves ran on: today's record
    assert launches[0] == ("plain", 64, 0, bt["npl"], False, 4, (units + 3) // 4)
    assert [w[0] for w in launches[1:]] == ["split"]
    if name in state.get("witness", {}):
        assert launches == state["witness"][name]
    # ... and the grid is the persistent kernel's: the one asked for, or the chip's fill cut to the piece
    if wgs is None:
        assert 1 <= grids[0] <= launches[0][6]
    else:
        assert grids[0] == wgs


def test_persistent_grid_is_the_chips_fill(state):
    """a piece of more workgroups than a chip holds at once: the default grid is smaller than the piece, the hits and bytes the model's"""
    bt = state["batches"][BIG]
    launches, grids = _check(state, BIG, QCOVS[0], 1, None)
    units = bt["n_reads"] * BLOCKS * TILES
    assert launches[0] == ("plain", 64, 0, bt["npl"], False, 4, (units + 3) // 4)
    assert [w[0] for w in launches[1:]] == ["split"]
    assert launches[0][6] > CHIP_WORKGROUPS
    assert 1 <= grids[0] < launches[0][6]
