"""The databases and queries of tests/test_gpu_dbset.py, built once per session: three members that overlap (A and B share two genomes:
exact ties across members; C holds mutated copies of four genomes of A: near ties) and reads that hit them — 2 000 short read pairs and 40
reads of 12 kb, whose > 10 000 k-mers make neighbouring counts print the same qCov."""
import numpy as np

from tests import synth

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def mutate(seq, rate, rng):
    r = np.frombuffer(seq, dtype=np.uint8).copy()
    m = rng.random(len(r)) < rate
    r[m] = _ACGT[rng.integers(0, 4, size=int(m.sum()))]
    return r.tobytes()


def build(tmp, seed=300):
    rng = np.random.default_rng(seed)
    genomes = synth.random_genomes(14, 20000, seed=seed)
    names = [f"g{i:02d}" for i in range(14)]
    a = synth.make_db(tmp / "A", genomes[:8], k=21, n_chunks=2, threads=4, names=names[:8])
    b = synth.make_db(tmp / "B", genomes[6:], k=21, n_chunks=2, threads=4, names=names[6:])
    c = synth.make_db(tmp / "C", [mutate(g, 0.01, rng) for g in genomes[:4]], k=21, n_chunks=2, threads=4, names=[f"m{i:02d}" for i in range(4)])
    # mates from one fragment (read 2 from the other strand, 100 bases further on); read 1 alone is the single-end input
    reads = synth.sample_reads(genomes, 2000, 150, sub_rate=0.01, seed=seed + 1, frac_random=0.1)
    reads2 = []
    for i in range(2000):
        g = genomes[int(rng.integers(0, 14))]
        p = int(rng.integers(0, len(g) - 400))
        r1, r2 = mutate(g[p:p + 150], 0.01, rng), mutate(g[p + 250:p + 400], 0.01, rng).translate(_COMP)[::-1]
        if i % 2:
            reads[i] = r1
            reads2.append(r2)
        else:  # (an unrelated mate: the pair's k-mers are diluted)
            reads2.append(_ACGT[rng.integers(0, 4, size=150)].tobytes())
    long_reads = []
    for i in range(40):
        g = genomes[i % 14]
        p = int(rng.integers(0, len(g) - 12000))
        long_reads.append(mutate(g[p:p + 12000], 0.002, rng))
    return dict(genomes=genomes, dirs=[a, b, c], reads=reads + long_reads, reads2=reads2 + [mutate(r, 0.002, rng)[:150] for r in long_reads])
