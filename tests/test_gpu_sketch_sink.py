"""kmcpg_sketch_genomes_to (Sketcher.sketch_to): the lists a sketch call returns, delivered piece by piece in device memory.  The sink
copies every piece's lists down from d_hashes itself and the test compares them with what Sketcher.sketch returns on the same genomes
(tests/test_gpu_sketch.py holds that against the oracle), chunk by chunk, in the five sketch modes; with a small
KMCPG_SKETCH_PIECE_BASES a call has several pieces, each with its own koff from 0; a sink that fails ends the call with its code and
the sketcher goes on working."""
import numpy as np
import pytest

from tests import synth
from tests.test_gpu_sketch import MODES

pytestmark = pytest.mark.gpu


def genomes_small():
    base = synth.random_genomes(2, 60000, seed=401)
    return [base[0], base[1][:30000], base[1][1000:1015], b"", base[1][2000:2100]]


def collect(lib, sk, genomes, **kw):
    """-> pieces [(first_chunk, genome, chunk_idx, chunks, koff, hashes)] copied inside the sink"""
    pieces = []

    def sink(p):
        assert int(p["koff"][0]) == 0 and len(p["koff"]) == p["n_chunks"] + 1
        h = lib.copy_from_device(p["d_hashes"], int(p["koff"][-1]), np.uint64, p["stream"])
        pieces.append((p["first_chunk"], p["genome"], p["chunk_idx"], p["chunks"], p["koff"], h))

    sk.sketch_to(genomes, sink, **kw)
    return pieces


def assert_pieces_equal_sketch(lib, sk, genomes, pieces, **kw):
    with sk.sketch(genomes, **kw) as want:
        at = 0
        for first, genome, chunk_idx, chunks, koff, h in pieces:
            assert first == at
            for i in range(len(genome)):
                c = at + i
                assert (int(genome[i]), int(chunk_idx[i]), int(chunks[i])) == (int(want.genome[c]), int(want.chunk_idx[c]), int(want.chunks[c])), c
                assert np.array_equal(h[int(koff[i]):int(koff[i + 1])], want.list(c)), c
            at += len(genome)
        assert at == len(want)
        return len(want), int(want.koff[len(want)])


@pytest.mark.parametrize("mode", list(MODES))
def test_pieces_deliver_the_lists_of_sketch(mode, monkeypatch):
    from kmcp_amd import lib
    genomes = genomes_small()
    kw = dict(split_number=4, split_overlap=20, split_min_ref=1000)
    with lib.Sketcher(device=0, **MODES[mode]) as sk:
        pieces = collect(lib, sk, genomes, **kw)
        assert len(pieces) == 1
        launches_to = sk.last_sketch_launches()
        n, keys = assert_pieces_equal_sketch(lib, sk, genomes, pieces, **kw)
        assert n == 4 + 4 + 0 + 0 + 1 and keys > 1000
        assert launches_to == sk.last_sketch_launches()  # the same launch records from both entry points
        # the same call in pieces: three at least, each with its own lists
        monkeypatch.setenv("KMCPG_SKETCH_PIECE_BASES", "30000")
        pieces = collect(lib, sk, genomes, **kw)
        assert len(pieces) >= 3 and len(sk.last_sketch_launches()) == len(pieces)
        assert assert_pieces_equal_sketch(lib, sk, genomes, pieces, **kw) == (n, keys)


def test_counting_sink_reads_koff_alone():
    from kmcp_amd import lib
    genomes = genomes_small()
    counts = []
    with lib.Sketcher(k=21, device=0) as sk:
        sk.sketch_to(genomes, lambda p: counts.extend(np.diff(p["koff"]).tolist()), split_number=4, split_overlap=20, split_min_ref=1000)
        with sk.sketch(genomes, split_number=4, split_overlap=20, split_min_ref=1000) as want:
            assert counts == [len(want.list(i)) for i in range(len(want))]
        calls = []
        sk.sketch_to([], calls.append)
        sk.sketch_to([b"ACGT", b""], calls.append, split_number=3, split_overlap=10)
        assert calls == []  # no chunk, no piece


def test_a_failing_sink_ends_the_call_and_the_sketcher_works_on(monkeypatch):
    from kmcp_amd import lib
    genomes = genomes_small()
    monkeypatch.setenv("KMCPG_SKETCH_PIECE_BASES", "30000")
    with lib.Sketcher(k=21, device=0) as sk:
        seen = []

        def failing(p):
            seen.append(p["first_chunk"])
            return -6 if len(seen) == 2 else 0

        with pytest.raises(lib.KmcpGpuError) as e:
            sk.sketch_to(genomes, failing, split_number=4, split_overlap=20, split_min_ref=1000)
        assert e.value.code == -6 and len(seen) == 2  # the sink's code, and no piece after it

        def raising(p):
            raise ValueError("from the sink")

        with pytest.raises(ValueError, match="from the sink"):
            sk.sketch_to(genomes, raising, split_number=4, split_overlap=20, split_min_ref=1000)
        pieces = collect(lib, sk, genomes, split_number=4, split_overlap=20, split_min_ref=1000)
        assert len(pieces) >= 3
        assert_pieces_equal_sketch(lib, sk, genomes, pieces, split_number=4, split_overlap=20, split_min_ref=1000)
