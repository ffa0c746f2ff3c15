"""Sliding windows of long queries (kmcp-search --sliding-step / --sliding-window / --sliding-greedy, kmcpg_submit_windows), host side:
the window enumeration of `seqkit sliding -s S -W W [-g]` as INTEGRATION.md restates it — kmcpg_window_count / kmcpg_window_locate against
an independent walk of the rule — and the CLI's refusal of the combinations seqkit gives no meaning (pairs, -g / -G, --query-id), which
happens before any database or GPU is touched."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")


def windows_of(L, step, window, greedy):
    """the rule of INTEGRATION.md: starts 0, S, 2S, ...; e = i + W; past the end: greedy cuts at L and goes on while i < L, else stop"""
    out = []
    i = 0
    while True:
        e = i + window
        if e > L:
            if not greedy or i >= L:
                break
            e = L
        out.append((i, e))
        i += step
    return out


def _offs(lengths):
    o = np.zeros(len(lengths) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(lengths)
    return o


CASES = [  # (read lengths, step, window): reads shorter than W, S > W, S = W, S < W, W = 1, S = 1, empty reads
    ([10, 3, 0, 7, 12, 1], 2, 6),
    ([10, 3, 0, 7, 12, 1], 7, 4),
    ([10, 3, 0, 7, 12, 1], 5, 5),
    ([300, 299, 301, 1000, 2], 100, 300),
    ([1000, 150, 149, 151], 4, 150),
    ([10_000, 212, 211, 9_999], 1000, 212),
    ([17, 16, 15], 1, 1),
    ([17, 16, 15], 3, 1),
    ([0, 0], 3, 2),
]


@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("lengths,step,window", CASES)
def test_window_enumeration_matches_the_rule(lengths, step, window, greedy):
    from kmcp_amd import lib
    offs = _offs(lengths)
    want = [(r, i, e) for r, L in enumerate(lengths) for (i, e) in windows_of(L, step, window, greedy)]
    n, bases = lib.window_count(offs, step, window, greedy)
    assert n == len(want)
    assert bases == sum(e - i for _, i, e in want)
    read, start = lib.window_locate(offs, step, window, greedy)
    assert read.tolist() == [r for r, _, _ in want]
    assert start.tolist() == [i for _, i, _ in want]


@pytest.mark.parametrize("L,step,window,greedy,want", [
    (10, 2, 6, True, [(0, 6), (2, 8), (4, 10), (6, 10), (8, 10)]),  # S < W, greedy: cut windows kept while they start inside the read
    (10, 2, 6, False, [(0, 6), (2, 8), (4, 10)]),
    (10, 4, 3, False, [(0, 3), (4, 7)]),                            # S > W: gaps between windows
    (10, 4, 3, True, [(0, 3), (4, 7), (8, 10)]),
    (9, 3, 3, False, [(0, 3), (3, 6), (6, 9)]),                     # S = W: tiling
    (10, 3, 3, True, [(0, 3), (3, 6), (6, 9), (9, 10)]),
    (5, 2, 6, False, []),                                          # shorter than W: none without greedy, cut windows with it
    (5, 2, 6, True, [(0, 5), (2, 5), (4, 5)]),
])
def test_window_rule_by_hand(L, step, window, greedy, want):
    """the library's enumeration against windows written out by hand from the rule"""
    from kmcp_amd import lib
    offs = _offs([L])
    n, bases = lib.window_count(offs, step, window, greedy)
    read, start = lib.window_locate(offs, step, window, greedy)
    assert n == len(want) and bases == sum(e - i for i, e in want)
    assert start.tolist() == [i for i, _ in want] and read.tolist() == [0] * len(want)
    assert windows_of(L, step, window, greedy) == want


def test_window_locate_of_a_later_row_range():
    from kmcp_amd import lib
    import ctypes as C
    offs = _offs([1000, 150, 700])
    spec = lib.WindowSpec(4, 150, 0, 0)
    read_all, start_all = lib.window_locate(offs, 4, 150, False)
    read = np.zeros(7, dtype=np.uint32)
    start = np.zeros(7, dtype=np.uint64)
    L = lib.load()
    assert L.kmcpg_window_locate(offs.ctypes.data, 3, C.byref(spec), 210, 7, read.ctypes.data, start.ctypes.data) == 0
    assert read.tolist() == read_all[210:217].tolist() and start.tolist() == start_all[210:217].tolist()
    # past the last window, a zero step: refused
    assert L.kmcpg_window_locate(offs.ctypes.data, 3, C.byref(spec), len(read_all) - 3, 7, read.ctypes.data, start.ctypes.data) == -1
    n = C.c_uint64()
    for bad in (lib.WindowSpec(0, 150, 0, 0), lib.WindowSpec(4, 0, 0, 0), lib.WindowSpec(2**64 - 3, 150, 0, 0),  # zero / a negative step
                lib.WindowSpec(4, 2**64 - 1, 1, 0), lib.WindowSpec(4, 150, 2, 0), lib.WindowSpec(4, 150, 0, 7)):   # greedy 0/1, reserved 0
        assert L.kmcpg_window_count(offs.ctypes.data, 3, C.byref(bad), C.byref(n), None) == -1


def _cli(args, tmp_path):
    fq = tmp_path / "r.fa"
    fq.write_text(">a\nACGTACGTACGTACGTACGT\n")
    r = subprocess.run([CLI] + [a if a != "@" else str(fq) for a in args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("args,needle", [
    (["--sliding-step", "4", "--sliding-window", "10", "-1", "@", "-2", "@"], "paired-end"),
    (["--sliding-step", "4", "--sliding-window", "10", "-g", "@"], "-g/--query-whole-file"),
    (["--sliding-step", "4", "--sliding-window", "10", "-G", "@"], "-G/--use-filename"),
    (["--sliding-step", "4", "--sliding-window", "10", "--query-id", "x", "@"], "--query-id"),
    (["--sliding-step", "4", "@"], "needed together"),
    (["--sliding-window", "10", "--sliding-greedy", "@"], "needed together"),
    (["--sliding-step", "0", "--sliding-window", "10", "@"], "should be positive"),
    (["--sliding-step", "4", "--sliding-window", "0", "@"], "should be positive"),
    (["--sliding-step", "-3", "--sliding-window", "10", "@"], "should be positive"),
])
def test_cli_refuses_what_seqkit_sliding_cannot_mean(args, needle, tmp_path):
    """refused before the database is opened (the path given to -d does not even exist)"""
    rc, err = _cli(args + ["-d", str(tmp_path / "no_such_db")], tmp_path)
    assert rc != 0
    assert needle in err, err
    assert "sliding" in err, err


def test_cli_help_names_the_sliding_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--sliding-step", "--sliding-window", "--sliding-greedy", "_sliding:"):
        assert flag in r.stderr
