"""Index inspection on the GPU (kmcpg_block_density, kmcpg_col_ones, kmcpg_open_files, kmcp-inspect): every count against a recount of
the same bits with numpy — from the bytes of the .uniki file at offset0 for databases on disk, from read_row_range for synthetic
handles — MSB of a byte = first column (kmcp/cmd/index-density.go:177-185).  Counts are integers: equality is exact.  The launch
witness says which kernel form served a call: bins below 256 rows take the bit-extract form, all others the carry-save form with
the narrowest lane group (4, 8, 16, 32, 64) that covers the 16-byte lanes the block's bytes overlap."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import synth, uniki

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSPECT = os.path.join(ROOT, "kmcp_amd", "kmcp-inspect")
KMCP = os.path.join(ROOT, "kmcp_amd", "kmcp")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from kmcp_amd import lib
    if not (os.path.exists(lib.LIB_PATH) and os.path.exists(INSPECT)):
        g.build()
    return lib


def expected_lpr(byte_off, row_bytes):
    lanes = (byte_off + row_bytes + 15) // 16 - byte_off // 16
    for lpr in (4, 8, 16, 32):
        if lanes <= lpr:
            return lpr
    return 64


def bin_sizes(num_sigs):
    return [1, 7, 64, 255, 256, 1000, num_sigs, num_sigs + 1]


def check_block(db, block, rows, byte_off, seen):
    """every bin size of the issue's list + a sub-range that starts past row 0 and ends inside a bin, against the recount"""
    bi = db.block_info(block)
    ns, nc, rb = bi["num_sigs"], bi["n_cols"], bi["row_bytes"]
    assert rows.shape == (ns, rb)
    lpr = expected_lpr(byte_off, rb)
    for br in bin_sizes(ns):
        got = db.block_density(block, br)
        want = uniki.recount(rows, nc, br)
        assert got.shape == want.shape == (nc, (ns + br - 1) // br)
        assert np.array_equal(got, want), (block, br, np.argwhere(got != want)[:5])
        w = db.last_density_launch()
        if br < 256:
            assert w["form"] == "small" and w["launches"] >= 1
        else:
            assert w["form"] == "csa" and w["lpr"] == lpr and w["npl"] == 12 and w["workgroups"] >= 1 and w["launches"] >= 1
            seen.add(lpr)
    # rows 3 .. : 2 1/2 bins of the carry-save form, 4 bins + 3 rows of the other
    for br, n in ((256, 2 * 256 + 128), (300, min(ns - 3, 1000)), (64, 4 * 64 + 3)):
        if 3 + n > ns:
            continue
        got = db.block_density(block, br, first_row=3, n_rows=n)
        want = uniki.recount(rows, nc, br, 3, n)
        assert np.array_equal(got, want), (block, br, n)
    # a range that runs to the block's last row from its middle
    got = db.block_density(block, 256, first_row=ns // 2)
    assert np.array_equal(got, uniki.recount(rows, nc, 256, ns // 2, 0))


@pytest.fixture(scope="module")
def narrow_dbs(tmp_path_factory, oracle_lib):
    """three single-block databases of 1-, 5- and 39-byte rows (5, 37 and 312 columns): a few thousand rows each"""
    out = []
    for n_genomes, n_chunks in ((5, 1), (37, 1), (39, 8)):
        tmp = tmp_path_factory.mktemp(f"dens{n_genomes}x{n_chunks}")
        genomes = synth.random_genomes(n_genomes, 1500 * n_chunks, seed=100 + n_genomes)
        r001 = synth.make_db(tmp, genomes, k=21, n_chunks=n_chunks, overlap=50, threads=1)
        files = uniki.db_files(r001)
        assert len(files) == 1
        out.append((str(tmp), r001, os.path.join(r001, files[0])))
    return out


def test_narrow_blocks_ungrouped(L, narrow_dbs):
    seen = set()
    widths = []
    for _, r001, f in narrow_dbs:
        h = uniki.read_header(f)
        widths.append(h["row_bytes"])
        assert h["num_sigs"] > 2000
        with L.Database.open(r001, device=0) as db:
            rows = uniki.read_rows(f, h)
            check_block(db, 0, rows, 0, seen)
            ones = db.col_ones()
            assert ones.dtype == np.uint64 and np.array_equal(ones, uniki.recount(rows, len(h["names"]), h["num_sigs"])[:, 0])
    assert widths == [1, 5, 39] and seen == {4}


@pytest.fixture(scope="module")
def grouped_db(tmp_path_factory, oracle_lib, L):
    """blocks of 39, 39 and 1 bytes per row, and of 5, 5 and 1, each trio with one NumSigs (uniform_sigs = 1): resident they share one row of
    79 / 11 bytes, and the second and third block start at bytes 39, 78 / 5, 10 of it"""
    out = []
    for n_cols, block_size in ((312 + 312 + 5, 312), (40 + 40 + 3, 40)):
        tmp = tmp_path_factory.mktemp(f"densg{block_size}")
        genomes = synth.random_genomes(n_cols, 1200 + 7 * block_size, seed=block_size)
        cols = synth.make_columns(genomes, oracle_lib.sketch_cfg(k=21))
        r001 = L.build_db(str(tmp), cols, k=21, block_size=block_size, uniform_sigs=1)
        out.append((str(tmp), r001))
    return out


def test_narrow_blocks_grouped_at_odd_byte_offsets(L, grouped_db):
    seen = set()
    for (_, r001), want_rb in zip(grouped_db, ([39, 39, 1], [5, 5, 1])):
        files = uniki.db_files(r001)
        hs = [uniki.read_header(os.path.join(r001, f)) for f in files]
        assert [h["row_bytes"] for h in hs] == want_rb
        assert len({h["num_sigs"] for h in hs}) == 1
        with L.Database.open(r001, device=0) as db:
            strides = {db.block_info(b)["stride"] for b in range(len(files))}
            assert strides == {128 if want_rb[0] == 39 else 16}  # one group: the pitch of the sum of the rows
            byte_off = 0
            all_ones = []
            for b, (f, h) in enumerate(zip(files, hs)):
                rows = uniki.read_rows(os.path.join(r001, f), h)
                check_block(db, b, rows, byte_off, seen)
                all_ones.append(uniki.recount(rows, len(h["names"]), h["num_sigs"])[:, 0])
                byte_off += h["row_bytes"]
            ones = db.col_ones()
            assert np.array_equal(ones, np.concatenate(all_ones))  # every block at once
            assert db.last_density_launch()["launches"] == 1        # one pass over the one group
    assert seen == {4}


def synthetic_rows(db, block):
    bi = db.block_info(block)
    rows = np.zeros((bi["num_sigs"], bi["row_bytes"]), dtype=np.uint8)
    db.read_row_range(block, 0, rows)
    return rows


@pytest.mark.parametrize("cols,want_lpr", [(1000, 8), (8203, 64), (3001, 32), (1500, 16)])
def test_synthetic_blocks_of_every_lane_form(L, cols, want_lpr):
    """125-byte rows on the 8-lane form; 8203 columns (not a multiple of 8) = 1026-byte rows: a full 64-lane tile and a second one of one
    lane; the 32- and 16-lane forms; 5000 rows, so a bin of all rows is cut at the planes' capacity"""
    spec = L.SynthSpec(k=21, num_hashes=1, fpr=0.3, n_blocks=2, cols_per_block=cols, num_sigs=5000, kmers_per_col=1700, seed=cols, scale=0,
                       syncmer_s=0, minimizer_w=0, sigs_step=13)
    seen = set()
    with L.Database.open_synthetic(spec, device=0) as db:
        per_block = []
        for b in range(2):
            rows = synthetic_rows(db, b)
            assert 0.05 < np.unpackbits(rows[:64]).mean() < 0.6
            if b == 1 or cols <= 1500:
                check_block(db, b, rows, 0, seen)
            per_block.append(uniki.recount(rows, cols, rows.shape[0])[:, 0])
        assert seen == {want_lpr}
        ones = db.col_ones()
        assert np.array_equal(ones, np.concatenate(per_block))
        sums = np.concatenate([db.block_density(b, 1000).sum(axis=1, dtype=np.uint64) for b in range(2)])
        assert np.array_equal(ones, sums)  # col_ones = the sum over a column's bins
        assert db.last_density_launch()["form"] == "csa"


def test_planting_raises_one_column_only(L):
    spec = L.SynthSpec(k=21, num_hashes=1, fpr=0.3, n_blocks=2, cols_per_block=200, num_sigs=40000, kmers_per_col=1, seed=9, scale=0, syncmer_s=0,
                       minimizer_w=0, sigs_step=0)
    with L.Database.open_synthetic(spec, device=0) as db:
        before = db.col_ones()
        assert before.max() < 400  # all but empty
        rng = np.random.default_rng(5)
        hashes = rng.integers(0, 2**63, size=3000, dtype=np.uint64)
        hashes = np.concatenate([hashes, hashes[:500]])  # repeats do not count twice
        col = 200 + 77
        rows_hit = np.unique(hashes % np.uint64(40000))
        already = db.read_rows(1, rows_hit)
        was_set = (already[:, 77 // 8] >> (7 - 77 % 8)) & 1
        db.plant(col, hashes)
        after = db.col_ones()
        diff = after.astype(np.int64) - before.astype(np.int64)
        assert diff[col] == len(rows_hit) - int(was_set.sum())
        diff[col] = 0
        assert not diff.any()


def test_open_files_on_one_block_of_a_database(L, grouped_db):
    _, r001 = grouped_db[0]
    files = uniki.db_files(r001)
    with L.Database.open(r001, device=0) as full:
        want = full.block_density(1, 500)
        want_ones = full.col_ones()
        cb = full.block_info(1)["col_base"]
        nc = full.block_info(1)["n_cols"]
    with L.Database.open_files([os.path.join(r001, files[1])], device=0) as one:
        assert one.info.n_blocks == 1 and one.info.n_blocks_local == 1 and one.info.n_cols == nc
        assert np.array_equal(one.block_density(0, 500), want)
        assert np.array_equal(one.col_ones(), want_ones[cb:cb + nc])
        h = uniki.read_header(os.path.join(r001, files[1]))
        rows = np.zeros((10, h["row_bytes"]), dtype=np.uint8)
        one.read_row_range(0, 5, rows)
        assert np.array_equal(rows, uniki.read_rows(os.path.join(r001, files[1]), h)[5:15])
        assert one.col_info(3)[0] == h["names"][3]
        with pytest.raises(L.KmcpGpuError) as e:
            one.search([b"ACGT" * 40])
        assert e.value.code == -6
        seqs, offs = L.pack_reads([b"ACGT" * 40])
        with pytest.raises(L.KmcpGpuError) as e:
            one.submit(seqs, offs)
        assert e.value.code == -6
    # two files in another order than the database lists them: blocks numbered in argument order
    with L.Database.open_files([os.path.join(r001, files[2]), os.path.join(r001, files[0])], device=0) as two:
        h2 = uniki.read_header(os.path.join(r001, files[2]))
        assert two.block_info(0)["n_cols"] == len(h2["names"])
        assert np.array_equal(two.block_density(0, 256), uniki.recount(uniki.read_rows(os.path.join(r001, files[2]), h2), len(h2["names"]), 256))


def test_density_between_submit_and_wait(L, oracle_lib, tmp_path):
    genomes = synth.random_genomes(6, 30000, seed=21)
    r001 = synth.make_db(tmp_path, genomes, k=21, n_chunks=4, overlap=150, threads=2)
    reads = synth.sample_reads(genomes, 300, 150, sub_rate=0.01, seed=8, frac_random=0.1)
    seqs, offs = L.pack_reads(reads)
    files = uniki.db_files(r001)
    odb = oracle_lib.OracleDB(r001)
    with L.Database.open(r001, device=0) as db:
        t1 = db.submit(seqs, offs)
        d1 = db.block_density(0, 512)
        t2 = db.submit(seqs, offs)
        ones = db.col_ones()
        r1 = db.wait(t1)
        d2 = db.block_density(len(files) - 1, 3)
        r2 = db.wait(t2)
        assert synth.assert_parity(odb, r1, reads) > 0
        assert synth.assert_parity(odb, r2, reads) > 0
        want_ones = []
        for b, f in enumerate(files):
            h = uniki.read_header(os.path.join(r001, f))
            rows = uniki.read_rows(os.path.join(r001, f), h)
            want_ones.append(uniki.recount(rows, len(h["names"]), h["num_sigs"])[:, 0])
            if b == 0:
                assert np.array_equal(d1, uniki.recount(rows, len(h["names"]), 512))
            if b == len(files) - 1:
                assert np.array_equal(d2, uniki.recount(rows, len(h["names"]), 3))
        assert np.array_equal(ones, np.concatenate(want_ones))
    odb.close()


def test_error_codes(L, narrow_dbs):
    _, r001, f = narrow_dbs[2]
    with L.Database.open(r001, device=0) as db:
        ns, nc = db.block_info(0)["num_sigs"], db.block_info(0)["n_cols"]
        for kw in (dict(bin_rows=0), dict(bin_rows=8, first_row=ns), dict(bin_rows=8, first_row=10, n_rows=ns - 9)):
            with pytest.raises(L.KmcpGpuError) as e:
                db.block_density(0, **kw)
            assert e.value.code == -1
        with pytest.raises(L.KmcpGpuError) as e:
            db.block_density(1, 8)
        assert e.value.code == -1
        spec = L.DensitySpec(256, 0, 0, 0)
        n_bins = db.density_bins(0, 256)
        buf = np.zeros(nc * n_bins, dtype=np.uint32)
        assert L.load().kmcpg_block_density(db._h, 0, C.byref(spec), buf.ctypes.data, nc * n_bins - 1) == -1
        bad = L.DensitySpec(256, 0, 0, 7)
        assert L.load().kmcpg_block_density(db._h, 0, C.byref(bad), buf.ctypes.data, buf.size) == -1
        assert L.load().kmcpg_block_density(db._h, 0, C.byref(spec), buf.ctypes.data, buf.size) == 0
        ones = np.zeros(nc, dtype=np.uint64)
        assert L.load().kmcpg_col_ones(db._h, ones.ctypes.data, nc - 1) == -1
    with L.Database.open(r001, device=-1) as meta:
        with pytest.raises(L.KmcpGpuError) as e:
            meta.block_density(0, 256)
        assert e.value.code == -4
        with pytest.raises(L.KmcpGpuError) as e:
            meta.col_ones()
        assert e.value.code == -4


def test_error_codes_paged_and_sharded(L, grouped_db):
    _, r001 = grouped_db[0]
    with L.Database.open_paged(r001, device=0, passes=2) as paged:
        assert paged.paged_info()[0] == 2
        with pytest.raises(L.KmcpGpuError) as e:
            paged.block_density(0, 256)
        assert e.value.code == -6
        with pytest.raises(L.KmcpGpuError) as e:
            paged.col_ones()
        assert e.value.code == -6
    with L.Database.open_devices(r001, [0, 0]) as front:
        with pytest.raises(L.KmcpGpuError) as e:
            front.block_density(0, 256)
        assert e.value.code == -6
        with pytest.raises(L.KmcpGpuError) as e:
            front.col_ones()
        assert e.value.code == -6
    # one shard of two: the other shard's blocks are not local, their columns count 0
    files = uniki.db_files(r001)
    with L.Database.open(r001, device=0, shard_rank=0, shard_count=2) as sh:
        local = [sh.block_info(b)["local"] for b in range(len(files))]
        assert any(local) and not all(local)
        ones = sh.col_ones()
        for b, f in enumerate(files):
            h = uniki.read_header(os.path.join(r001, f))
            bi = sh.block_info(b)
            part = ones[bi["col_base"]:bi["col_base"] + bi["n_cols"]]
            if bi["local"]:
                assert np.array_equal(part, uniki.recount(uniki.read_rows(os.path.join(r001, f), h), bi["n_cols"], h["num_sigs"])[:, 0])
            else:
                assert not part.any()
                with pytest.raises(L.KmcpGpuError) as e:
                    sh.block_density(b, 256)
                assert e.value.code == -1


def run(args):
    return subprocess.run(args, capture_output=True)


def test_cli_index_density_tsv_and_pgm(L, narrow_dbs, tmp_path):
    _, r001, f = narrow_dbs[2]
    ns = uniki.read_header(f)["num_sigs"]
    for flags, kw in ((["--bins", "100"], dict(bins=100)), (["-b", "7"], dict(bins=7)), (["--bin-size", "300"], dict(bin_size=300)),
                      (["-s", "1"], dict(bin_size=1)), ([], dict()), (["-s", str(ns)], dict(bin_size=ns))):
        want = uniki.density_tsv(f, **kw).encode()
        r = run([INSPECT, "index-density"] + flags + [f])
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (flags, r.stdout[:200], want[:200])
        out = str(tmp_path / "d.tsv.gz")
        r = run([KMCP, "utils", "index-density"] + flags + ["-o", out, f])
        assert r.returncode == 0, r.stderr
        assert gzip.open(out, "rb").read() == want
    # the reference's quirk: --bins 100 prints floor(NumSigs / binSize) counts, which is more than 100 unless 100 divides NumSigs
    bins, bs = uniki.density_bins(ns, bins=100)
    line = uniki.density_tsv(f, bins=100).split("\n")[1].split("\t")
    assert line[2] == "100" and len(line[4].split(",")) == ns // bs
    for flags, kw in ((["--bins", "100"], dict(bins=100)), (["--bin-size", "300"], dict(bin_size=300)), (["--bin-size", str(ns // 4)], dict(bin_size=ns // 4))):
        img = str(tmp_path / "d.pgm")
        r = run([INSPECT, "index-density"] + flags + ["-o", str(tmp_path / "d.tsv"), "--out-img", img, "--verbose", f])
        assert r.returncode == 0, r.stderr
        assert open(img, "rb").read() == uniki.density_pgm(f, **kw), flags
        assert b"minimum count in bins of" in r.stderr and b"maximum count in bins of" in r.stderr


def test_cli_ref_info_measured(L, grouped_db, tmp_path):
    db_dir, r001 = grouped_db[1]
    files = uniki.db_files(r001)
    rows = uniki.ref_info_rows(r001, files)
    ones = np.concatenate([uniki.recount(uniki.read_rows(os.path.join(r001, f)), len(uniki.read_header(os.path.join(r001, f))["names"]),
                                         uniki.read_header(os.path.join(r001, f))["num_sigs"])[:, 0] for f in files])
    r = run([INSPECT, "ref-info", "-d", db_dir, "--measured"])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().split("\n")
    assert lines[0] == "file\ti\ttarget\tchunkIdx\tchunks\tkmers\tfpr\tones\tfprMeasured" and lines[-1] == ""
    assert len(lines) - 2 == len(rows) == len(ones)
    for line, row, o in zip(lines[1:-1], rows, ones):
        g = line.split("\t")
        assert g[:6] == [row[0], str(row[1]), row[2], str(row[3]), str(row[4]), str(row[5])]
        assert abs(float(g[6]) - row[6]) <= 1e-6
        assert int(g[7]) == int(o)
        assert abs(float(g[8]) - (float(o) / row[7]) ** row[8]) <= 1e-6


def test_uniform_sigs_lowers_the_measured_fpr(L, oracle_lib, tmp_path):
    """two blocks, one with half the k-mers per column: uniform_sigs = 1 gives it the other block's NumSigs, and every one of its columns
    then has a measured false-positive rate (ones / NumSigs) ^ hashes that is not higher — about half, in fact: the same k-mers in twice
    the rows (bit density 1 - exp(-k / NumSigs): 0.16 instead of 0.30), so 3/4 of the old value is a safe upper bound"""
    genomes = synth.random_genomes(16, 6000, seed=31) + synth.random_genomes(16, 3000, seed=32)
    cols = synth.make_columns(genomes, oracle_lib.sketch_cfg(k=21))
    measured = {}
    for u in (0, 1):
        r001 = L.build_db(str(tmp_path / f"u{u}"), cols, k=21, block_size=16, uniform_sigs=u)
        with L.Database.open(r001, device=0) as db:
            assert db.info.n_blocks == 2
            ns = [db.block_info(b)["num_sigs"] for b in range(2)]
            names = [db.col_info(c)[0] for c in range(32)]
            ones = db.col_ones()
            measured[u] = (ns, np.array([float(ones[c]) / ns[c // 16] for c in range(32)]) ** db.info.num_hashes, names)
    assert measured[0][2] == measured[1][2]
    grew = [b for b in range(2) if measured[1][0][b] > measured[0][0][b]]
    assert len(grew) == 1
    for b in range(2):
        f0, f1 = measured[0][1][16 * b:16 * b + 16], measured[1][1][16 * b:16 * b + 16]
        if b in grew:
            assert (f1 <= f0).all()
            assert (f1 < 0.75 * f0).all()
        else:
            assert measured[1][0][b] == measured[0][0][b] and np.array_equal(f1, f0)
