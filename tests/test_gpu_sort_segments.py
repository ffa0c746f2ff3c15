"""The segmented sort + unique of sort_segments.hip alone (kmcpg_sort_segments_device), on keys the test lays out: every number of
radix passes (both parities of the buffer the result lands in), segments around the 4096 keys of a wave, equal keys across wave and
segment borders, up to 8 parts with empty ones and foreign data between the lists, max_waves above the true number of waves, and
more segments / histogram tiles than one pass of the single-workgroup scan covers.

The reference is numpy: list s is np.unique of the concatenation over parts of keys[p * part_stride + in_off[s] : ... + cnt[p][s]].
Equality is exact; koff must be the cumulative unique counts, koff[n_segs + 1] the raw total.  Every case stays inside the sort's
contract (no key has a bit at or above key_bits, fewer than 2^32 raw keys)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE = 4096  # SEGSORT_KEYS_PER_WAVE


class Layout:
    """Raw lists as SegSortIn describes them.  lists[s] = the raw keys of segment s (uint64); splits[s] = how many of them each part
    holds (default: the first part holds all); gaps[s] = words between the room of list s and that of list s + 1 (room = the largest
    part of the list).  Every word that belongs to no list holds `filler`."""

    def __init__(self, lists, parts=1, splits=None, gaps=None, filler=0, cnt_stride=None, tail_gap=0):
        n = len(lists)
        self.parts, self.n_segs = parts, n
        self.cnt_stride = n if cnt_stride is None else cnt_stride
        assert self.cnt_stride >= n
        self.filler = filler
        cnt = np.full((parts, max(self.cnt_stride, 1)), 12345, dtype=np.int32)  # entries past n_segs: never to be read
        in_off = np.zeros(max(n, 1), dtype=np.uint64)
        at = 0
        for s, lst in enumerate(lists):
            sp = [len(lst)] + [0] * (parts - 1) if splits is None or splits[s] is None else list(splits[s])
            assert len(sp) == parts and sum(sp) == len(lst) and min(sp) >= 0
            cnt[:, s] = sp
            in_off[s] = at
            at += max(sp) + (0 if gaps is None else gaps[s])
        self.part_stride = at + tail_gap
        keys = np.full(max(parts * self.part_stride, 1), filler, dtype=np.uint64)
        for s, lst in enumerate(lists):
            i = 0
            for p in range(parts):
                c = int(cnt[p, s])
                o = p * self.part_stride + int(in_off[s])
                keys[o:o + c] = lst[i:i + c]
                i += c
        self.keys, self.in_off, self.cnt = keys, in_off, cnt
        self.sizes = [len(x) for x in lists]
        self.raw_total = sum(self.sizes)
        self.true_waves = sum((x + WAVE - 1) // WAVE for x in self.sizes)

    def reference(self):
        """[np.unique of the concatenation over parts] per segment, read from the laid-out arrays"""
        out = []
        for s in range(self.n_segs):
            o = int(self.in_off[s])
            out.append(np.unique(np.concatenate(
                [self.keys[p * self.part_stride + o:p * self.part_stride + o + int(self.cnt[p, s])] for p in range(self.parts)]).astype(np.uint64)))
        return out


def run(lay, key_bits, max_waves=None, want=None):
    """sorts the layout on the GPU and checks lists, koff and the launch record; returns the record"""
    import torch

    from kmcp_amd import lib
    dev = torch.device("cuda", 0)
    if max_waves is None:
        max_waves = lay.true_waves
    if want is None:
        want = lay.reference()
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)  # noqa: E731
    t_keys, t_off, t_cnt = up(lay.keys, np.int64), up(lay.in_off, np.int64), up(lay.cnt.reshape(-1), np.int32)
    out_cap = lay.parts * lay.part_stride
    guard = 16  # words behind out_cap: never to be written
    t_out = torch.full((out_cap + guard,), -2, dtype=torch.int64, device=dev)
    t_koff = torch.full((lay.n_segs + 2 + guard,), -3, dtype=torch.int64, device=dev)
    rec = lib.sort_segments_device(t_keys.data_ptr(), t_off.data_ptr(), t_cnt.data_ptr(), lay.part_stride, lay.cnt_stride, lay.parts, lay.n_segs,
                                   max_waves, key_bits, t_out.data_ptr(), out_cap, t_koff.data_ptr())
    out = t_out.cpu().numpy().view(np.uint64)
    koff = t_koff.cpu().numpy().view(np.uint64)
    n = lay.n_segs
    assert np.array_equal(t_keys.cpu().numpy().view(np.uint64), lay.keys), "the raw lists were changed"
    assert (koff[n + 2:] == np.uint64(2**64 - 3)).all() and (out[out_cap:] == np.uint64(2**64 - 2)).all()
    want_koff = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    assert int(koff[n + 1]) == lay.raw_total
    bad = np.flatnonzero(koff[:n + 1] != want_koff)
    assert len(bad) == 0, ("koff", int(bad[0]), int(koff[bad[0]]), int(want_koff[bad[0]]), lay.sizes[max(int(bad[0]) - 1, 0)])
    flat = np.concatenate(want) if want else np.zeros(0, dtype=np.uint64)
    got = out[:len(flat)]
    if not np.array_equal(got, flat):
        i = int(np.flatnonzero(got != flat)[0])
        s = int(np.searchsorted(want_koff, i, side="right")) - 1
        raise AssertionError(f"list {s} (size {lay.sizes[s]}) differs at its key {i - int(want_koff[s])}: {int(got[i]):#x} for {int(flat[i]):#x}")
    passes = (key_bits + 7) // 8
    assert (rec["kind"], rec["passes"], rec["key_bits"], rec["segments"], rec["keys"]) == (0, passes, key_bits, n, lay.raw_total)
    assert rec["workgroups"] == (max_waves + 3) // 4
    if max_waves:
        assert rec["launches"] == 2 + 5 * passes + 5 + 1
    return rec


def uniform(rng, key_bits, n, avoid=None):
    """n keys uniform below 2**key_bits, none equal to `avoid`"""
    k = rng.integers(0, 1 << key_bits, size=n, dtype=np.uint64)
    if avoid is not None:
        k[k == np.uint64(avoid)] = np.uint64(avoid ^ 1)
    return k


def distinct(rng, key_bits, n, avoid=None):
    """n distinct keys below 2**key_bits in random order"""
    k = np.unique(uniform(rng, key_bits, n + n // 4 + 64, avoid))
    assert len(k) >= n
    return rng.permutation(k)[:n]


# ---- key widths ----
WIDTH_SIZES = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 0, 0, 8191, 8192, 8193, 12289, 1]


@pytest.mark.parametrize("key_bits", [1, 8, 9, 16, 17, 24, 32, 33, 40, 41, 48, 49, 56, 57, 61, 64])
def test_every_key_width(key_bits):
    """1 to 8 passes: with an odd number the sorted keys are in the second buffer and the unique step writes the first.  Gaps between
    the lists hold a filler (where key_bits leaves room for a value that is in no list)."""
    rng = np.random.default_rng(1000 + key_bits)
    top = (1 << key_bits) - 1
    passes = (key_bits + 7) // 8
    filler = None if key_bits < 8 else 0x5A & top
    lists = []
    for s, n in enumerate(WIDTH_SIZES):
        k = uniform(rng, key_bits, n, filler)
        if key_bits >= 33 and n >= 4095:
            base = int(uniform(rng, key_bits, 1)[0]) & ~0xFF & ~(0xFF << (8 * (passes - 1)))
            hi = np.arange(1 << (key_bits - 8 * (passes - 1)), dtype=np.uint64) << np.uint64(8 * (passes - 1))  # differ in the top used byte alone
            lo = np.arange(256, dtype=np.uint64)                                                               # differ in byte 0 alone
            planted = np.concatenate([np.uint64(base) | hi, np.uint64(base) | lo, (np.uint64(base) | lo)[::3]])
            assert filler not in planted
            at = rng.choice(n, size=len(planted), replace=False)
            k[at] = planted
        if n >= 2 and s % 2 == 0 or n >= 4095:  # the smallest and the largest key, more than once in the long lists
            at = rng.choice(n, size=min(n, 6), replace=False)
            k[at[:len(at) // 2]] = 0
            k[at[len(at) // 2:]] = top
        lists.append(k)
    assert all(int(k.max()) <= top for k in lists if len(k))
    lay = Layout(lists, filler=filler or 0, gaps=None if filler is None else [(0, 1, 300)[s % 3] for s in range(len(lists))])
    want = lay.reference()
    assert want[6][0] == 0 and want[6][-1] == top and want[14][0] == 0 and want[14][-1] == top
    rec = run(lay, key_bits, want=want)
    assert rec["passes"] == passes
    if filler is not None:
        assert all(filler not in w for w in want)


# ---- equal keys across wave and segment borders ----
def run_at(rng, key_bits, first_rank, n=8192, run_len=100):
    """n keys, all distinct but one value that occurs run_len times and, once sorted, fills ranks first_rank .. first_rank + run_len - 1"""
    d = np.sort(distinct(rng, key_bits, n - run_len + 1))
    k = np.concatenate([d, np.full(run_len - 1, d[first_rank], dtype=np.uint64)])
    assert np.array_equal(np.flatnonzero(np.sort(k) == d[first_rank]), np.arange(first_rank, first_rank + run_len))
    return rng.permutation(k)


@pytest.mark.parametrize("key_bits", [64, 40])  # 8 passes and 5: the unique step reads either buffer
def test_equal_keys_across_a_wave_border(key_bits):
    rng = np.random.default_rng(2000 + key_bits)
    lists = [
        np.full(8193, 0x1234567 + key_bits, dtype=np.uint64),  # three waves of one value
        run_at(rng, key_bits, 4046),                           # the run crosses the border at 4096
        uniform(rng, key_bits, 77),
        run_at(rng, key_bits, 3996),                           # ends at rank 4095
        run_at(rng, key_bits, 4096),                           # starts at rank 4096
        np.full(4096, 5, dtype=np.uint64),
        np.full(4097, 5, dtype=np.uint64),
    ]
    lay = Layout(lists)
    want = lay.reference()
    assert [len(w) for w in want[:2]] == [1, 8093] and len(want[3]) == len(want[4]) == 8093
    run(lay, key_bits, want=want)


@pytest.mark.parametrize("key_bits", [64, 40])
def test_equal_keys_across_a_segment_border(key_bits):
    """a segment's first key is a head whatever precedes it"""
    rng = np.random.default_rng(2100 + key_bits)

    def ending_in(v, n):  # n keys (some twice) whose largest is v
        k = uniform(rng, key_bits - 1, n)
        k[rng.choice(n, size=min(n, 3), replace=False)] = v
        return k

    def starting_with(v, n):  # n keys whose smallest is v
        k = uniform(rng, key_bits - 1, n) | np.uint64(1 << (key_bits - 1))
        k[rng.choice(n, size=min(n, 3), replace=False)] = v
        return k

    v = np.uint64(1 << (key_bits - 1))
    same_a, same_b, same_c = uniform(rng, key_bits, 5000), uniform(rng, key_bits, 64), uniform(rng, key_bits, 4096)
    lists = [
        ending_in(v, 4096), starting_with(v, 300),  # s ends on a wave border
        ending_in(v, 100), starting_with(v, 4097),
        ending_in(v, 100), np.zeros(0, dtype=np.uint64), starting_with(v, 100),
        np.array([v], dtype=np.uint64), np.array([v], dtype=np.uint64), np.array([v, v], dtype=np.uint64),
        same_a, same_a.copy(), same_b, same_b.copy(), same_b[::-1].copy(), same_c, same_c.copy(),
        np.zeros(0, dtype=np.uint64),
    ]
    lay = Layout(lists)
    want = lay.reference()
    for s in (0, 2, 4):
        nxt = s + 1 if len(want[s + 1]) else s + 2
        assert want[s][-1] == want[nxt][0] == v
    run(lay, key_bits, want=want)


# ---- parts, empty parts, gaps with foreign data ----
def cut(rng, n, parts, zero=()):
    """n keys over `parts` parts, the parts in `zero` empty"""
    live = [p for p in range(parts) if p not in zero]
    c = [0] * parts
    if live:
        at = np.sort(rng.integers(0, n + 1, size=len(live) - 1))
        for p, x in zip(live, np.diff(np.concatenate([[0], at, [n]]))):
            c[p] = int(x)
    assert sum(c) == (n if live else 0)
    return c


@pytest.mark.parametrize("key_bits", [64, 23])
@pytest.mark.parametrize("parts", [1, 2, 3, 8])
def test_parts_and_gaps(parts, key_bits):
    rng = np.random.default_rng(3000 + 10 * parts + key_bits)
    filler = 0x2A2A2A & ((1 << key_bits) - 1)
    last, mid = parts - 1, parts // 2
    splits = [
        cut(rng, 5000, parts),
        cut(rng, 700, parts, zero=(0,)) if parts > 1 else [0],                 # the first part empty
        cut(rng, 4200, parts, zero=(mid,)) if parts > 2 else cut(rng, 4200, parts),  # a middle part empty
        cut(rng, 900, parts, zero=(last,)) if parts > 1 else [900],            # the last part empty
        [1037] + [0] * (parts - 2) + [4000] if parts > 1 else [5037],          # a part ends inside wave 0, inside a round of 64 keys
        [0] * parts,                                                           # an empty list
        [4096 + 100] + [3] * (parts - 1),                                      # a part ends inside wave 1; parts of 3 keys
        [1] * parts,
        cut(rng, 64, parts, zero=(0, last)) if parts > 2 else cut(rng, 64, parts),
        [4096 // parts] * parts,
    ]
    lists = [uniform(rng, key_bits, sum(sp), filler) for sp in splits]
    lists[3][:40] = lists[3][40:80]  # duplicates, also across parts
    lists[4][1030:1045] = lists[4][0]
    gaps = [0, 1, 311, 0, 700, 1, 0, 5, 0, 250]
    lay = Layout(lists, parts=parts, splits=splits, gaps=gaps, filler=filler, cnt_stride=len(lists) + 5, tail_gap=129)
    assert (lay.keys == np.uint64(filler)).sum() >= sum(gaps) * parts
    want = lay.reference()
    assert all(filler not in w for w in want) and len(want[5]) == 0
    run(lay, key_bits, want=want)


# ---- max_waves is an upper bound ----
@pytest.mark.parametrize("key_bits", [56, 64, 9])
def test_max_waves_above_the_true_count(key_bits):
    """the histogram entries past the last wave hold stale totals from the second pass on: nothing may depend on them"""
    rng = np.random.default_rng(4000 + key_bits)
    lists = [uniform(rng, key_bits, n) for n in (5000, 0, 4096, 70, 9000, 0)]
    lists[0][:500] = lists[0][4500:]  # duplicates at any key width
    lists[4][4000:4200] = lists[4][8800:]
    lay = Layout(lists)
    want = lay.reference()
    true = lay.true_waves
    assert true == 2 + 1 + 1 + 3
    for mw in (true, true + 1, 3 * true):
        run(lay, key_bits, max_waves=mw, want=want)


def test_batches_without_keys():
    empty = np.zeros(0, dtype=np.uint64)
    run(Layout([empty] * 7, parts=2, splits=[[0, 0]] * 7, gaps=[3] * 7, filler=9), 64, max_waves=5)
    run(Layout([empty] * 7), 64, max_waves=0)
    run(Layout([empty] * 3), 0, max_waves=0)  # nothing to sort: no key width needed
    run(Layout([]), 64, max_waves=0)
    run(Layout([], tail_gap=10, filler=9), 33, max_waves=5)


# ---- many segments, long histogram tables ----
@pytest.mark.parametrize("n_segs", [1023, 1024, 1025, 5000])
def test_many_small_segments(n_segs):
    """the single-workgroup scan of the per-segment arrays gives each of its 1024 threads ceil((n_segs + 1) / 1024) entries"""
    rng = np.random.default_rng(5000 + n_segs)
    sizes = rng.integers(0, 41, size=n_segs)
    sizes[-1] = 40 if n_segs % 2 else 0
    lists = [uniform(rng, 12, int(n)) for n in sizes]  # 12 bits: duplicates inside and between the lists
    run(Layout(lists), 12)
    run(Layout(lists), 64, max_waves=n_segs + 7)


def test_more_than_1024_tiles_of_the_histogram_table():
    """20000 waves: 256 * 20000 / 4096 = 1250 tile sums, two per thread of the single-workgroup scan"""
    rng = np.random.default_rng(5100)
    n = 20000
    keys = uniform(rng, 17, n)
    lay = Layout([keys[i:i + 1] for i in range(n)])
    assert lay.true_waves == n
    run(lay, 17, max_waves=n)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_long_segment_among_3000_small_ones(where):
    rng = np.random.default_rng(5200)
    small = [uniform(rng, 48, int(n)) for n in rng.integers(0, 41, size=3000)]
    big = uniform(rng, 48, 50000)
    big[1000:3000] = big[:2000]
    at = {"first": 0, "middle": 1500, "last": 3000}[where]
    lists = small[:at] + [big] + small[at:]
    run(Layout(lists), 48, max_waves=3000 + 13)


# ---- refusals ----
def test_refusals_launch_nothing():
    """bad arguments are refused before anything is enqueued: the output buffers keep what they held"""
    import torch

    from kmcp_amd import lib
    dev = torch.device("cuda", 0)
    lay = Layout([np.arange(1, 101, dtype=np.uint64), np.arange(50, 60, dtype=np.uint64)])
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)  # noqa: E731
    t_keys, t_off, t_cnt = up(lay.keys, np.int64), up(lay.in_off, np.int64), up(lay.cnt.reshape(-1), np.int32)
    t_out = torch.full((8 * lay.part_stride,), -2, dtype=torch.int64, device=dev)
    t_koff = torch.full((lay.n_segs + 2,), -3, dtype=torch.int64, device=dev)
    t_zero = torch.zeros(lay.n_segs, dtype=torch.int64, device=dev)  # both lists at in_off 0

    def call(parts=1, key_bits=64, max_waves=2, keys=None, out=None, koff=None, out_cap=None, cnt_stride=None, off=None, part_stride=None):
        return lib.sort_segments_device(t_keys.data_ptr() if keys is None else keys, (t_off if off is None else off).data_ptr(), t_cnt.data_ptr(),
                                        lay.part_stride if part_stride is None else part_stride,
                                        lay.cnt_stride if cnt_stride is None else cnt_stride, parts, lay.n_segs, max_waves, key_bits,
                                        t_out.data_ptr() if out is None else out, t_out.numel() if out_cap is None else out_cap,
                                        t_koff.data_ptr() if koff is None else koff)

    for kw in (dict(parts=0), dict(parts=9), dict(key_bits=-1), dict(key_bits=65),
               dict(key_bits=0),  # with keys present: refused by the sort's launcher itself, before it enqueues anything
               dict(keys=0), dict(out=0), dict(koff=0), dict(out_cap=lay.part_stride - 1), dict(cnt_stride=1),
               dict(max_waves=1),                      # the lists need two waves
               dict(off=t_zero, part_stride=100)):     # overlapping lists: 110 raw keys in 100 words
        with pytest.raises(lib.KmcpGpuError) as e:
            call(**kw)
        assert e.value.code == -1, kw  # KMCPG_EINVAL
    torch.cuda.synchronize()
    assert bool((t_out == -2).all()) and bool((t_koff == -3).all())
    rec = call()
    assert rec["passes"] == 8 and rec["keys"] == 110
    assert t_koff.cpu().tolist() == [0, 100, 110, 110]
    assert t_out[:110].cpu().tolist() == list(range(1, 101)) + list(range(50, 60))
