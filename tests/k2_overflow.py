"""The hit buffer's overflow contract (include/kmcp_gpu.h, kmcpg_query_device) at every place of the COBS kernels that reserves and
stores hits: the checker of one run and the declared cases of tests/test_gpu_k2_overflow.py.  No GPU and no library is needed to import
it: tests/test_k2_overflow_cpu.py holds the checker against crafted outputs and the table against k2_forms_plan on every machine.

The contract: d_counters[0] receives the number of hits PRODUCED, whatever the buffer holds (lane.cpp collect() sizes its rerun by it);
only hit_cap hits are stored, each of them a real hit, none twice; nothing is written at or behind hits[hit_cap]; hit_cap == 0 with no
buffer at all is a legal "count only" call.

Three pieces of device code emit hits, all by the same pattern (one atomicAdd on the counter per wave, `if (idx < hit_cap)` stores):

    A  the epilogue of k2_cobs_body.inc        every k2_cobs<...> form without K2F_ bits, k2_cobs_pair: 4 to 64 lanes per unit, up to 16
                                               different reads share one reservation
    B  k2_emit_tile (k2_short.hpp)             the short-read unit: launched (KMCPG_K2_PERSIST=0), persistent (k2_cobs_persist<8|10>), block
                                               units (KMCPG_K2_BLOCK_UNITS=1)
    C  k_threshold_long (k2_cobs.hip)          the chunked long-query form, on the counter the A or B launches before it have advanced

A case is a database of k2_forms_plan (or `x2`, below), a batch of about 40 reads, and the settings that send the batch to one of the
sites; its witness comes from k2_forms_plan.expect.  The 8-plane batch has two forms: "8" (no read above 254 k-mers, so that it stays
on 8 planes under the default rules) and "8s" — the same with a read of 400 k-mers and three more short ones — for the cases that set
KMCPG_SPLIT_MIN=16: there every read above 16 k-mers, the 400 included, goes to the chunked form and the others stay on 8 planes.
"""
from collections import namedtuple

import numpy as np

from tests import k2_forms_plan as P

GUARD = 4096             # rows behind hits[hit_cap] that a run must leave alone
SENTINEL = 0x5A5A5A5A    # every word of the buffer before a run; no read index, column or count of a case can equal it
TOMBSTONE = 0xFFFFFFFF   # kmcpg_hit::read of a reserved place without a column (k2_cobs_body.inc); never produced by a sound index
RUN = 200                # columns a planted read fills at the front of block 0 and at the back of the last block

# the short-read unit's variables: they act only under KMCPG_GROUP_ROWS=4 (k2_plan.hpp short_flags), and tests/test_gpu_k2_forms.py
# _KNOBS — what is cleared before every run — must name them
K2_KNOBS = ("KMCPG_K2_BLOCK_UNITS", "KMCPG_K2_EXACT_STOP", "KMCPG_K2_PERSIST", "KMCPG_K2_PERSIST_WGS")


# ---- the checker ---------------------------------------------------------------------------------------------------------------------
def check_run(ref_keys, ref_cnts, ncols, cap, counter0, buf, sentinel=SENTINEL):
    """One run of kmcpg_query_device with hit_cap = cap against the complete reference list.

    ref_keys, ref_cnts: every hit of the batch, sorted by key = read * ncols + col, with its count (T = len(ref_keys)).
    counter0: d_counters[0] after the run.  buf: the WHOLE device buffer after the run, [cap + GUARD, 3] 32-bit words (read, col, count),
    every word `sentinel` before the run ([0, 3] for the call without a buffer).
    -> problems, one string per broken promise, each starting with its name: counter, hole, tombstone, duplicate, foreign, count,
    beyond, list."""
    ref_keys = np.asarray(ref_keys, dtype=np.int64)
    ref_cnts = np.asarray(ref_cnts, dtype=np.int64)
    buf = np.ascontiguousarray(buf).view(np.uint32).reshape(-1, 3)
    T = len(ref_keys)
    m = min(int(cap), T)
    assert len(buf) >= m and np.all(ref_keys[1:] > ref_keys[:-1])
    problems = []
    if int(counter0) != T:
        problems.append("counter: d_counters[0] is %d, the batch has %d hits (hit_cap %d)" % (int(counter0), T, cap))
    head, rest = buf[:m], buf[m:]
    untouched = np.all(head == np.uint32(sentinel), axis=1)
    if untouched.any():
        problems.append("hole: %d of the first %d rows were never written, the first at index %d" % (int(untouched.sum()), m, int(untouched.argmax())))
    at = np.nonzero(~untouched)[0]           # what was stored, by index
    rows = head[at].astype(np.int64)
    tomb = rows[:, 0] == TOMBSTONE
    if tomb.any():
        problems.append("tombstone: %d rows, the first at index %d" % (int(tomb.sum()), int(at[tomb.argmax()])))
    at, rows = at[~tomb], rows[~tomb]
    keys = rows[:, 0] * int(ncols) + rows[:, 1]
    uniq, first, n_of = np.unique(keys, return_index=True, return_counts=True)
    if len(uniq) != len(keys):
        k = int(uniq[n_of > 1][0])
        problems.append("duplicate: %d keys are stored more than once, (read %d, col %d) at indices %s" % (
            int((n_of > 1).sum()), k // ncols, k % ncols, at[keys == k][:4].tolist()))
    pos = np.minimum(np.searchsorted(ref_keys, keys), max(T - 1, 0))
    member = (ref_keys[pos] == keys) & (rows[:, 1] < ncols) if T else np.zeros(len(keys), dtype=bool)
    if (~member).any():
        i = int((~member).argmax())
        problems.append("foreign: %d stored tuples are no hits of the batch, the first (read %d, col %d, count %d) at index %d" % (
            int((~member).sum()), rows[i, 0], rows[i, 1], rows[i, 2], int(at[i])))
    wrong = member.copy()
    wrong[member] = ref_cnts[pos[member]] != rows[member, 2]
    if wrong.any():
        i = int(wrong.argmax())
        problems.append("count: %d stored hits carry a wrong count, the first (read %d, col %d) %d instead of %d at index %d" % (
            int(wrong.sum()), rows[i, 0], rows[i, 1], rows[i, 2], int(ref_cnts[pos[i]]), int(at[i])))
    touched = np.any(rest != np.uint32(sentinel), axis=1)
    if touched.any():
        i = int(touched.argmax())
        problems.append("beyond: %d rows at or behind index min(hit_cap, hits) = %d were written, the first at index %d: %s" % (
            int(touched.sum()), m, m + i, rest[i].tolist()))
    if cap >= T:
        order = np.argsort(keys, kind="stable")
        if not (len(keys) == T and np.array_equal(keys[order], ref_keys) and np.array_equal(rows[order, 2], ref_cnts)):
            problems.append("list: the %d stored hits are not the batch's %d" % (len(keys), T))
    return problems


def capacities(T):
    """the hit_cap values of a case with T hits, in the order they run: the buffer that fits and the one with a row to spare, then every
    buffer that is too small — none at all (None: hit_cap 0 and no pointer), 0, 1, the wave's edge, 16 odd values spread over (65, T - 1),
    T - 1.  (The caller ends with T once more: the rerun of lane.cpp collect().)"""
    assert T >= 512
    odd = sorted({int(v) | 1 for v in np.linspace(65, T - 1, 18)[1:-1]})
    assert len(odd) == 16 and 65 < odd[0] and odd[-1] < T - 1
    return [T + 1, T, None, 0, 1, 63, 64, 65] + odd + [T - 1]


def pick_qcov(counts, ns, budget):
    """the smallest min_qcov (steps of 0.01, min_matched = 1) that lets at most `budget` of the counted (read, column) pairs pass — as
    tests/test_gpu_k2_forms.py _pick_thresholds picks its threshold (b)"""
    assert 0 < budget < counts.size
    ratio = np.sort((counts / np.maximum(ns, 1)[:, None]).ravel())[::-1]
    q = max(0.05, np.ceil(float(ratio[budget]) * 100) / 100)
    while int(((counts >= cmin(ns, q)[:, None]) & (ns > 0)[:, None]).sum()) > budget:
        q = round(q + 0.01, 2)
    assert q < 1.0
    return float(round(q, 2))


def cmin(ns, min_qcov, min_matched=1):
    return np.maximum(min_matched, np.floor(np.asarray(ns) * min_qcov).astype(np.int64) + 1)  # csa.hpp count_threshold


# ---- databases and batches -----------------------------------------------------------------------------------------------------------
# x2: the row shape of tests/test_gpu_k2_exact_stop.py with padding bits in the last byte — 14 973 columns = 1 872-byte rows on a 1 920-byte
# pitch, two tiles of the 64-lane class (1 024 + 896 bytes), three blocks of different NumSigs.  Registered where P.expect looks layouts
# up, as `big8` is; P.LAYOUTS and P.DBS (what the forms test runs) do not get it.
X2 = P.Layout("x2", 14973, 3, 4099, 1920, 1920)
P.LAYOUT.setdefault("x2", X2)
DB = dict(P.DB)
DB["x2-h1"] = P.Db("x2-h1", "x2", 1, (), P.NUM_SIGS)

SPLIT_MIN = P.SPLIT_SMALL
_8 = [130] * 31 + [0, 1, 5, 64, 129, 131, 254]
_ORDER = np.random.default_rng(20261020)


def _shuffled(ns):
    return [int(n) for n in np.array(ns)[_ORDER.permutation(len(ns))]]


# NumKmers of the reads, in batch order; neither size is a multiple of 4 (the last workgroup of a 64-lane launch is part-filled)
BATCH_N = {
    "8": _shuffled(_8),
    "8s": _shuffled(_8 + [400, 16, 12, 9]),          # for KMCPG_SPLIT_MIN=16: six reads stay short, the 400 goes to the chunked form too
    "10": _shuffled(_8[1:] + [255, 1022]),
    "16": _shuffled([1023, 1024, 1025, 1100, 1300, 1500, 1536, 1700, 1900, 2000, 2047, 2048, 2048]),   # at most 2 048: k2_ask_long does not ask
}
PLANES = {"8": 8, "8s": 8, "10": 10, "16": 16}     # of the launches that are not chunked


def planted(batch):
    """(the read copied into the first RUN columns of block 0, the read copied into the last RUN columns of the last block): two reads
    of 130 k-mers (16 planes: the first and the last read); in "8s" the second one is the read of 16 k-mers, so that the short reads'
    site has a run of hits in one lane as the chunked form has"""
    ns = BATCH_N[batch]
    if batch == "16":
        return 0, len(ns) - 1
    i130 = [i for i, n in enumerate(ns) if n == 130]
    return i130[0], (ns.index(16) if batch == "8s" else i130[-1])


# grid: what Database.last_k2_grids()[0] must be — None: not asserted (site A on layouts whose every setting takes site A);
# "piece": the record's workgroups (one wave per unit); "resident": 1 .. workgroups (the persistent kernel's default grid); an int: that
# many (KMCPG_K2_PERSIST_WGS); "block": the record's workgroups, which are those of one unit per (read, block)
Case = namedtuple("Case", "id site db batch env expect grid")

_GR4 = {"KMCPG_GROUP_ROWS": "4"}


def _case(site, dbk, batch, name, env=None, grid=None):
    env = dict(env or {})
    return Case("%s-%s-p%s-%s" % (site.lower(), dbk, batch, name), site, dbk, batch, env, tuple(P.expect(DB[dbk], BATCH_N[batch], env)), grid)


def _cases():
    c = [_case("A", dbk, "8", "default") for dbk in ("n4s-h1", "f8-h1", "n16a-h3", "n32a-h1", "n64p-h1", "t3-h1")]
    c += [_case("A", "n8-h1", "10", "gr4", _GR4),
          _case("C", "n8-h1", "8s", "split16", {"KMCPG_SPLIT_MIN": str(SPLIT_MIN)}),
          _case("C", "n8-h1", "8s", "split16-chunk64", {"KMCPG_SPLIT_MIN": str(SPLIT_MIN), "KMCPG_SPLIT_CHUNK": "64"}),
          _case("A", "p16-h1", "16", "pair"),
          _case("B", "n64f-h1", "8", "gr4-persist", _GR4, "resident")]
    x2 = [("A", "8", "plain", dict(_GR4, KMCPG_K2_EXACT_STOP="0", KMCPG_K2_BLOCK_UNITS="0"), "piece"),
          ("B", "8", "launched", dict(_GR4, KMCPG_K2_PERSIST="0"), "piece"),
          ("B", "10", "launched", dict(_GR4, KMCPG_K2_PERSIST="0"), "piece"),
          ("B", "8", "persist", dict(_GR4, KMCPG_K2_PERSIST="1"), "resident"),
          ("B", "10", "persist", dict(_GR4, KMCPG_K2_PERSIST="1"), "resident"),
          ("B", "8", "persist-wgs1", dict(_GR4, KMCPG_K2_PERSIST="1", KMCPG_K2_PERSIST_WGS="1"), 1),
          ("B", "8", "persist-wgs3", dict(_GR4, KMCPG_K2_PERSIST="1", KMCPG_K2_PERSIST_WGS="3"), 3),
          ("B", "8", "block-exact", dict(_GR4, KMCPG_K2_BLOCK_UNITS="1", KMCPG_K2_EXACT_STOP="1"), "block"),
          ("B", "8", "block", dict(_GR4, KMCPG_K2_BLOCK_UNITS="1", KMCPG_K2_EXACT_STOP="0"), "block"),
          ("C", "8s", "gr4-split16", dict(_GR4, KMCPG_SPLIT_MIN=str(SPLIT_MIN)), "resident")]
    c += [_case(site, "x2-h1", batch, name, env, grid) for site, batch, name, env, grid in x2]
    return c


CASES = _cases()   # database by database: the test keeps the last one open
