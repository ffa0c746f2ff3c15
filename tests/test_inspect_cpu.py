"""kmcp-inspect without a GPU: `ref-info` (kmcp/cmd/ref-info.go:107-149) byte for byte against text formatted here from the headers,
the `kmcp utils ...` spellings of the dispatcher, the refusals of `index-density` (index-density.go:150-155 would divide by zero, panic
or print nothing there) and the argument checks of the density calls on a metadata-only handle."""
import gzip
import os
import subprocess

import pytest

from tests import synth, uniki

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSPECT = os.path.join(ROOT, "kmcp_amd", "kmcp-inspect")
KMCP = os.path.join(ROOT, "kmcp_amd", "kmcp")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from kmcp_amd import lib
    if not (os.path.exists(lib.LIB_PATH) and os.path.exists(INSPECT) and os.path.exists(KMCP)):
        g.build()
    return lib


@pytest.fixture(scope="module")
def small_db(tmp_path_factory, oracle_lib):
    tmp = tmp_path_factory.mktemp("inspect_db")
    genomes = synth.random_genomes(7, 6000, seed=3)
    r001 = synth.make_db(tmp, genomes, k=21, n_chunks=3, overlap=100, threads=4)
    return str(tmp), r001


def run(args, **kw):
    return subprocess.run(args, capture_output=True, **kw)


def expected_ref_info(r001, header=True):
    rows = uniki.ref_info_rows(r001, uniki.db_files(r001))
    text = "file\ti\ttarget\tchunkIdx\tchunks\tkmers\tfpr\n" if header else ""
    for fn, i, target, ci, nch, kmers, fpr, _, _ in rows:
        text += "%s\t%d\t%s\t%d\t%d\t%d\t%f\n" % (fn, i, target, ci, nch, kmers, fpr)
    return text, rows


def assert_same_ref_info(got, want, want_rows, header=True):
    """byte-equal but for the fpr column, which is compared as a float within 1e-6: one unit of the last digit %f prints (pow may differ in
    the last bit between libraries)"""
    gl, wl = got.split("\n"), want.split("\n")
    assert len(gl) == len(wl)
    assert gl[-1] == "" and wl[-1] == ""
    if header:
        assert gl[0] == wl[0]
    body = gl[1:-1] if header else gl[:-1]
    assert len(body) == len(want_rows) and len(body) > 0
    for line, wline, row in zip(body, wl[1:-1] if header else wl[:-1], want_rows):
        g, w = line.split("\t"), wline.split("\t")
        assert g[:6] == w[:6] and len(g) == 7
        assert abs(float(g[6]) - row[6]) <= 1e-6
        assert len(g[6].split(".")[1]) == 6


def test_ref_info_plain_no_header_and_gz(built, small_db, tmp_path):
    db, r001 = small_db
    assert len(uniki.db_files(r001)) > 1
    want, rows = expected_ref_info(r001)
    r = run([INSPECT, "ref-info", "-d", db])
    assert r.returncode == 0, r.stderr
    assert_same_ref_info(r.stdout.decode(), want, rows)
    want_h, _ = expected_ref_info(r001, header=False)
    r = run([INSPECT, "ref-info", "-d", db, "-H"])
    assert r.returncode == 0, r.stderr
    assert_same_ref_info(r.stdout.decode(), want_h, rows, header=False)
    out = str(tmp_path / "ri.tsv.gz")
    r = run([INSPECT, "ref-info", "--db-dir", db, "-o", out])
    assert r.returncode == 0, r.stderr
    assert_same_ref_info(gzip.open(out, "rb").read().decode(), want, rows)
    out2 = str(tmp_path / "ri.tsv")
    r = run([INSPECT, "ref-info", "-d", db, "--out-file", out2, "--no-header-row"])
    assert r.returncode == 0, r.stderr
    assert_same_ref_info(open(out2).read(), want_h, rows, header=False)


def test_dispatcher_sends_the_two_utils_to_kmcp_inspect(built, small_db):
    db, r001 = small_db
    want, rows = expected_ref_info(r001)
    r = run([KMCP, "utils", "ref-info", "-d", db])
    assert r.returncode == 0, r.stderr
    assert_same_ref_info(r.stdout.decode(), want, rows)
    r = run([KMCP, "-j", "4", "utils", "ref-info", "-d", db, "-H"])  # persistent flags in front of the command are handed on
    assert r.returncode == 0, r.stderr
    r = run([KMCP, "utils", "index-density", "-"])
    assert r.returncode == 255 and b"stdin not supported" in r.stderr
    r = run([KMCP, "--help"])
    assert r.returncode == 0 and b"kmcp utils index-density" in r.stdout and b"kmcp utils ref-info" in r.stdout


def test_other_utils_still_go_to_the_reference_binary(built, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "KMCP_REFERENCE_BIN"}
    env["PATH"] = str(tmp_path)  # no reference `kmcp` to be found
    r = run([KMCP, "utils", "filter", "x.tsv"], env=env)
    assert r.returncode == 255 and b"not part of this build" in r.stderr
    r = run([KMCP, "utils"], env=env)
    assert r.returncode == 255 and b"not part of this build" in r.stderr
    fake = tmp_path / "kmcp"
    fake.write_text("#!/bin/sh\necho reference \"$@\"\n")
    fake.chmod(0o755)
    r = run([KMCP, "utils", "filter", "x.tsv"], env=env)
    assert r.returncode == 0 and r.stdout == b"reference utils filter x.tsv\n"


def test_index_density_refuses_what_the_reference_cannot_bin(built, small_db):
    _, r001 = small_db
    f = os.path.join(r001, uniki.db_files(r001)[0])
    ns = uniki.read_header(f)["num_sigs"]
    r = run([INSPECT, "index-density", "--bins", str(ns + 1), f])  # binSize = NumSigs / bins = 0
    assert r.returncode == 255 and b"bin size is 0" in r.stderr and r.stdout == b""
    r = run([INSPECT, "index-density", "--bins", "0", f])
    assert r.returncode == 255 and r.stdout == b""
    r = run([INSPECT, "index-density", "--bin-size", str(ns + 1), f])
    assert r.returncode == 255 and b"larger than" in r.stderr and r.stdout == b""
    r = run([INSPECT, "index-density", "-"])
    assert r.returncode == 255 and b"stdin not supported" in r.stderr
    r = run([INSPECT, "index-density"])
    assert r.returncode == 255 and b"stdin not supported" in r.stderr
    r = run([INSPECT, "index-density", "--out-img", "x.jpg", f])
    assert r.returncode == 255 and b"JPEG is not offered" in r.stderr
    r = run([INSPECT, "index-density", "--bin-size", "1", "--out-img", "x.pgm", f])  # bins = NumSigs + 1 >= 65536 only for large files
    if ns + 1 >= 65536:
        assert r.returncode == 255 and b"too large for plotting" in r.stderr


def test_density_spec_checks_on_a_metadata_only_handle(built, small_db):
    lib = built
    _, r001 = small_db
    files = uniki.db_files(r001)
    with lib.Database.open(r001, device=-1) as db:
        ns = db.block_info(0)["num_sigs"]
        assert db.density_bins(0, 1) == ns
        assert db.density_bins(0, ns) == 1 and db.density_bins(0, ns + 1) == 1
        assert db.density_bins(0, 256) == (ns + 255) // 256
        assert db.density_bins(0, 100, first_row=50, n_rows=250) == 3
        assert db.density_bins(0, 100, first_row=ns - 1) == 1
        for kw in (dict(bin_rows=0), dict(bin_rows=8, reserved=1), dict(bin_rows=8, first_row=ns), dict(bin_rows=8, first_row=1, n_rows=ns),
                   dict(bin_rows=8, first_row=ns + 5, n_rows=1)):
            with pytest.raises(lib.KmcpGpuError) as e:
                db.density_bins(0, **kw)
            assert e.value.code == -1, kw
        with pytest.raises(lib.KmcpGpuError) as e:
            db.density_bins(len(files), 8)
        assert e.value.code == -1
        # a cap that is too small is an argument error whatever the handle; with room, a metadata-only handle has no device
        import ctypes as C
        import numpy as np
        spec = lib.DensitySpec(ns, 0, 0, 0)
        n_cols = db.block_info(0)["n_cols"]
        buf = np.zeros(n_cols, dtype=np.uint32)
        assert lib.load().kmcpg_block_density(db._h, 0, C.byref(spec), buf.ctypes.data, n_cols - 1) == -1
        assert lib.load().kmcpg_block_density(db._h, 0, C.byref(spec), buf.ctypes.data, n_cols) == -4
        ones = np.zeros(int(db.info.n_cols), dtype=np.uint64)
        assert lib.load().kmcpg_col_ones(db._h, ones.ctypes.data, len(ones) - 1) == -1
        assert lib.load().kmcpg_col_ones(db._h, ones.ctypes.data, len(ones)) == -4
    # the same headers through kmcpg_open_files, metadata only: blocks in argument order, every block local
    paths = [os.path.join(r001, f) for f in reversed(files)]
    with lib.Database.open_files(paths, device=-1) as db:
        assert db.info.n_blocks == len(files) and db.info.n_blocks_local == len(files)
        for i, p in enumerate(paths):
            h = uniki.read_header(p)
            bi = db.block_info(i)
            assert bi["num_sigs"] == h["num_sigs"] and bi["n_cols"] == len(h["names"]) and bi["local"]
            assert db.col_info(bi["col_base"])[0] == h["names"][0]
        assert db.density_bins(0, 7) == (uniki.read_header(paths[0])["num_sigs"] + 6) // 7
        with pytest.raises(lib.KmcpGpuError) as e:
            db.search([b"ACGT" * 20])
        assert e.value.code == -6
    with pytest.raises(lib.KmcpGpuError) as e:
        lib.Database.open_files([os.path.join(r001, "no_such.uniki")], device=-1)
    assert e.value.code == -2
