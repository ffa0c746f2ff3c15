"""kmcpg_sketch_genomes (`kmcp compute --split-number` on the GPU: chunks read in place, K1, segmented sort + unique) against the
oracle: every list equals O.sort_unique(O.generate_kmers(chunk, cfg)) exactly, for the chunks synth.split_chunks cuts and the
reference's drop rule (compute.go:713) keeps.  The launch witness pins what the segmented sort is for: the number of launches does
not depend on the number of chunks."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

MODES = {
    "plain": dict(k=21),
    "scaled": dict(k=21, scale=10),
    "syncmer": dict(k=21, syncmer_s=11),
    "minimizer": dict(k=21, minimizer_w=8),
    "two_k": dict(k=(21, 31)),
}


def expected_lists(O, genomes, mode, n, overlap, min_ref):
    """[(genome, chunk_idx, chunks, sorted-unique hashes)] as `kmcp compute` + sort would give them; mode = a key of MODES or the
    Sketcher's keyword arguments themselves"""
    kw = dict(MODES[mode] if isinstance(mode, str) else mode)
    ks = kw.pop("k")
    ks = [ks] if isinstance(ks, int) else list(ks)
    cfgs = [O.sketch_cfg(k=k, **kw) for k in ks]
    out = []
    for gi, g in enumerate(genomes):
        chunks = [g] if (n <= 1 or len(g) < min_ref) else synth.split_chunks(g, n, overlap)
        kept = [c for c in chunks if not (len(c) - 1 <= overlap or len(c) < min(ks))]
        for ci, c in enumerate(kept):
            h = np.concatenate([O.generate_kmers(c, cfg) for cfg in cfgs])
            out.append((gi, ci, len(kept), O.sort_unique(h)))
    return out


def check(O, genomes, mode, n, overlap, min_ref=0):
    from kmcp_amd import lib
    want = expected_lists(O, genomes, mode, n, overlap, min_ref)
    with lib.Sketcher(device=0, **(MODES[mode] if isinstance(mode, str) else mode)) as sk:
        with sk.sketch(genomes, split_number=n, split_overlap=overlap, split_min_ref=min_ref) as got:
            assert len(got) == len(want)
            for i, (gi, ci, of, h) in enumerate(want):
                assert (int(got.genome[i]), int(got.chunk_idx[i]), int(got.chunks[i])) == (gi, ci, of), i
                lst = got.list(i)
                assert len(lst) == len(h), (i, gi, ci, len(lst), len(h))
                assert np.array_equal(lst, h), (i, gi, ci)
            assert int(got.koff[len(want)]) == sum(len(w[3]) for w in want)
        launches = sk.last_sketch_launches()
    return want, launches


def decorated(length, seed):
    """a genome with runs of N, lower case and IUPAC bytes"""
    g = bytearray(synth.random_genomes(1, length, seed)[0])
    rng = np.random.default_rng(seed + 1)
    for _ in range(12):
        p = int(rng.integers(0, length - 400))
        g[p:p + int(rng.integers(1, 300))] = b"N" * 300
    g = g[:length]
    for _ in range(20):
        p = int(rng.integers(0, length - 2000))
        g[p:p + 1500] = bytes(g[p:p + 1500]).lower()
    for p in rng.integers(0, length, size=40):
        g[int(p)] = b"RYKMSWBDHVn-"[int(p) % 12]
    return bytes(g)


@pytest.mark.parametrize("mode", list(MODES))
def test_chunk_lists_equal_the_oracle(oracle_lib, mode):
    O = oracle_lib
    base = synth.random_genomes(2, 700000, seed=301)
    genomes = [
        base[0],             # 10 chunks of ~70 k bases: above 65 536 k-mers each
        base[1][:500000],    # 10 chunks of ~50 k: below
        decorated(200000, 302),
        base[1][1000:1015],  # below split_min_ref and shorter than k: its one chunk is dropped
        base[1][2000:2025],  # below split_min_ref: one short chunk (k = 31 finds nothing in it)
        b"",
    ]
    want, launches = check(O, genomes, mode, n=10, overlap=20, min_ref=100)
    assert len(want) == 10 + 10 + 10 + 0 + 1
    assert len(launches) == 1 and launches[0]["segments"] == len(want)
    if mode == "scaled":
        assert launches[0]["key_bits"] == 61 and launches[0]["passes"] == 8
    else:
        assert launches[0]["key_bits"] == 64 and launches[0]["passes"] == 8


@pytest.mark.parametrize("mode", ["plain", "scaled", "syncmer"])
def test_one_chunk_of_millions_of_kmers_beside_split_genomes(oracle_lib, mode):
    O = oracle_lib
    big = synth.random_genomes(1, 3000000, seed=303)[0]
    # some repeated sequence: duplicates to drop
    big = big[:2000000] + big[500000:1500000]
    other = synth.random_genomes(1, 4000000, seed=304)[0]
    want, _ = check(O, [big, other], mode, n=10, overlap=150, min_ref=3500000)
    assert len(want) == 11 and want[0][2] == 1
    if mode == "plain":
        assert 1900000 < len(want[0][3]) < 2100000


def test_empty_batch_and_genomes_without_chunks():
    from kmcp_amd import lib
    with lib.Sketcher(k=21, device=0) as sk:
        with sk.sketch([]) as got:
            assert len(got) == 0 and list(got.koff) == [0]
        with sk.sketch([b"ACGT", b""], split_number=3, split_overlap=10) as got:
            assert len(got) == 0 and list(got.koff) == [0]
        with sk.sketch([b"A" * 100]) as got:  # one chunk, one distinct k-mer
            assert len(got) == 1 and len(got.list(0)) == 1


def test_a_batch_cut_into_pieces(oracle_lib, monkeypatch):
    O = oracle_lib
    genomes = synth.random_genomes(7, 90000, seed=305) + [decorated(120000, 306)]
    whole, l1 = check(O, genomes, "plain", n=4, overlap=100)
    assert len(l1) == 1
    monkeypatch.setenv("KMCPG_SKETCH_PIECE_BASES", "100000")
    pieces, l2 = check(O, genomes, "plain", n=4, overlap=100)
    assert len(l2) >= 7 and sum(x["segments"] for x in l2) == len(whole) == len(pieces)
    check(O, genomes, "two_k", n=4, overlap=100)


def test_refusals():
    from kmcp_amd import lib
    for kw in (dict(k=0), dict(k=65), dict(k=21, minimizer_w=8, syncmer_s=11), dict(k=list(range(21, 30)))):
        with pytest.raises(lib.KmcpGpuError):
            lib.Sketcher(device=0, **kw)
    with lib.Sketcher(k=21, device=0) as sk:
        with pytest.raises(lib.KmcpGpuError):
            sk.sketch([b"ACGT" * 100], split_number=70000)


def test_launches_do_not_depend_on_the_number_of_chunks(oracle_lib):
    """The same bases as 8 chunks and as 512 chunks, every chunk above 65 536 k-mers (where the per-read path sorts device-wide, one
    read at a time): the segmented sort launches the same kernels."""
    from kmcp_amd import lib
    O = oracle_lib
    cfg = O.sketch_cfg(k=21)
    g = synth.random_genomes(1, 512 * 66000, seed=307)[0]
    seen = {}
    with lib.Sketcher(k=21, device=0) as sk:
        for n in (8, 512):
            chunks = synth.split_chunks(g, n, 0)
            assert len(chunks) == n and min(len(c) for c in chunks) - 20 > 65536
            with sk.sketch([g], split_number=n, split_overlap=0) as got:
                assert len(got) == n
                for i in (0, n // 2, n - 1):
                    assert np.array_equal(got.list(i), O.sort_unique(O.generate_kmers(chunks[i], cfg))), (n, i)
            rec = sk.last_sketch_launches()
            assert len(rec) == 1
            seen[n] = rec[0]
    a, b = seen[8], seen[512]
    assert (a["segments"], b["segments"]) == (8, 512)
    assert a["launches"] == b["launches"] and a["passes"] == b["passes"] == 8
    assert a["launches"] == 2 + 5 * 8 + 5 + 1
    # the same k-mers up to the k - 1 positions lost at every cut
    assert abs(a["keys"] - b["keys"]) <= 20 * 512 and a["keys"] > 33000000


# ---- the segmented sort at its edges, through the sketcher (tests/test_gpu_sort_segments.py has the sort alone) ----
@pytest.mark.parametrize("scale,key_bits,passes,length", [
    (256, 57, 8, 300000),     # maxHash == 2**56
    (257, 56, 7, 1500000),    # above 10000 hashes kept: a list longer than one wave, 7 passes (the result lands in the other buffer)
    (1000, 55, 7, 3000000),   # the scale of the genome-search index
    (65537, 48, 6, 1500000),
])
def test_fracminhash_scales_skip_radix_passes(oracle_lib, scale, key_bits, passes, length):
    O = oracle_lib
    g = synth.random_genomes(1, length, seed=310 + passes)[0]
    genomes = [g, g[:length // 7], g[1000:1000 + length // 3]]
    want, launches = check(O, genomes, dict(k=21, scale=scale), n=1, overlap=0)
    assert len(want) == 3 and len(launches) == 1
    assert (launches[0]["key_bits"], launches[0]["passes"]) == (key_bits, passes)
    assert int(O.lib().ko_max_hash(scale)).bit_length() == key_bits
    assert max(int(w[3][-1]) for w in want if len(w[3])).bit_length() <= key_bits
    if scale in (257, 1000):
        assert len(want[0][3]) > 4096, len(want[0][3])


@pytest.mark.parametrize("kw", [dict(k=21, scale=300, syncmer_s=11), dict(k=21, scale=300, minimizer_w=8)], ids=["syncmer", "minimizer"])
def test_fracminhash_of_syncmers_and_minimizers(oracle_lib, kw):
    """key_bits < 64 relies on every k-mer kernel form dropping hashes above maxHash"""
    O = oracle_lib
    base = synth.random_genomes(1, 700000, seed=320)[0]
    genomes = [base, decorated(200000, 321), base[5000:5100], base[:70000]]
    want, launches = check(O, genomes, kw, n=4, overlap=30, min_ref=1000)
    assert len(want) == 4 + 4 + 1 + 4 and len(launches) == 1
    assert (launches[0]["key_bits"], launches[0]["passes"]) == (56, 7)
    assert sum(len(w[3]) for w in want) > 300


def test_eight_kmer_sizes(oracle_lib):
    """eight parts, the upper ones empty for the short genomes"""
    O = oracle_lib
    ks = (15, 21, 25, 31, 41, 51, 61, 64)
    base = synth.random_genomes(1, 40000, seed=330)[0]
    genomes = [base[:30], base, base[100:164], decorated(9000, 331), base[:63], base[200:215]]
    assert len(genomes[0]) == 30 and len(genomes[2]) == 64
    want, launches = check(O, genomes, dict(k=ks), n=1, overlap=0)
    assert len(want) == len(genomes) and len(launches) == 1
    cfgs = [O.sketch_cfg(k=k) for k in ks]
    assert [len(O.generate_kmers(genomes[0], c)) for c in cfgs] == [16, 10, 6, 0, 0, 0, 0, 0]
    assert [len(O.generate_kmers(genomes[2], c)) for c in cfgs] == [50, 44, 40, 34, 24, 14, 4, 1]
    assert launches[0]["keys"] == sum(len(O.generate_kmers(g, c)) for g in genomes for c in cfgs)
    want, _ = check(O, genomes, dict(k=ks), n=3, overlap=20, min_ref=1000)
    assert len(want) == 1 + 3 + 1 + 3 + 1 + 0


def test_chunks_of_an_exact_number_of_kmers(oracle_lib):
    """lists of 4095, 4096, 4097 and 8192 raw keys (a wave of the sort owns 4096), lists of equal keys and identical neighbours"""
    O = oracle_lib
    cfg = O.sketch_cfg(k=21)
    r = synth.random_genomes(2, 20000, seed=340)
    rep = r[1][:6000]
    genomes = [r[0][:4095 + 20], r[0][:4096 + 20], r[0][5000:5000 + 4097 + 20], r[0][10000:10000 + 8192 + 20], b"N" * 200, b"A" * 9000, b"AC" * 4500,
               rep, rep, rep]
    raw = [len(O.generate_kmers(g, cfg)) for g in genomes]
    assert raw == [4095, 4096, 4097, 8192, 0, 8980, 8980, 5980, 5980, 5980]
    want, launches = check(O, genomes, "plain", n=1, overlap=0)
    assert len(want) == len(genomes) and [w[0] for w in want] == list(range(len(genomes)))
    assert [len(w[3]) for w in want[4:7]] == [0, 1, 2]
    assert np.array_equal(want[7][3], want[8][3]) and np.array_equal(want[8][3], want[9][3])
    assert launches[0]["keys"] == sum(raw) and launches[0]["passes"] == 8
