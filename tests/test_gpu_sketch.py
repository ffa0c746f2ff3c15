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
    """[(genome, chunk_idx, chunks, sorted-unique hashes)] as `kmcp compute` + sort would give them"""
    kw = dict(MODES[mode])
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
    with lib.Sketcher(device=0, **MODES[mode]) as sk:
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
