"""The sliding-window geometry of the library compiled alone (kmcp_amd/csrc/window_plan.hpp through tests/window_plan_check.cpp, g++ with
ASan/UBSan, no GPU): plan_windows (the pieces of a batch's windows), stage_windows (what a piece stages) and window_desc_at (what one thread
of k_window_desc computes), for (S, W) in {(1,1), (1,10), (4,10), (10,10), (13,10), (100,300)} with greedy on and off, budgets
{1, W, 2W+1, 1e9} and max_win {1, 3, 1<<22}, on reads of 0, 1, W-1, W, W+1, W+S-1, W+S and random lengths.

  the program itself    checks the whole grid (200 random lengths up to 5 000 per spec) against its own window-by-window walk
  this module           takes a smaller grid as numbers and recomputes every one of them from tests/test_sliding_cpu.py::windows_of:
                        the header's output is never the reference

Hard conditions: the pieces' slices name every window once and in order, n_win <= max_win, bases <= budget unless the piece is one window,
no empty piece, n_win and bases equal the recount.  Expected equality: the partition is that of the window-by-window greedy walk (a piece
closes when the next window would exceed either limit; a window that fits nowhere goes alone).  Per piece: src[w] is the window's first
base in the staged text, offs[w] the prefix of window bases, cpre the recount of chunks, wmax the longest window."""
import os
import subprocess

import pytest

from tests.test_sliding_cpu import windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("window_plan") / "window_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path,
                    os.path.join(ROOT, "tests", "window_plan_check.cpp")], check=True)
    return path


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.splitlines()[-1].startswith("ok: "), r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_the_whole_grid_against_the_window_by_window_walk(exe):
    last = run(exe).splitlines()[-1]
    assert last.startswith("ok: 144 cases, "), last  # 6 specs x greedy x 4 budgets x 3 max_win


def parse(out):
    """[(S, W, greedy, budget, max_win, k, chunk, lens, [piece])], piece = dict(n_win, bases, wmax, slices, copies, cpre, desc)"""
    cases = []
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        f = rest.split()
        if key == "case":
            cases.append([*map(int, f), None, []])
        elif key == "lens":
            cases[-1][7] = [int(x) for x in f]
        elif key == "piece":
            cases[-1][8].append(dict(n_win=int(f[0]), bases=int(f[1]), wmax=int(f[2])))
        elif key in ("slices", "copies", "desc"):
            cases[-1][8][-1][key] = [tuple(map(int, x.split(":"))) for x in f]
        elif key == "cpre":
            cases[-1][8][-1][key] = [int(x) for x in f]
    return cases


def test_every_number_of_a_small_grid_against_windows_of(exe):
    cases = parse(run(exe, "dump"))
    assert len(cases) == 144
    seen = set()
    for S, W, greedy, budget, max_win, k, chunk, lens, pieces in cases:
        what = f"S {S} W {W} greedy {greedy} budget {budget} max_win {max_win}"
        assert {0, 1, W - 1, W, W + 1, W + S - 1, W + S} <= set(lens), what
        offs = [0]
        for n in lens:
            offs.append(offs[-1] + n)
        wins = [(r, i, e) for r, n in enumerate(lens) for i, e in windows_of(n, S, W, bool(greedy))]  # the batch's windows in order
        # the greedy walk, window by window
        want, cur_n, cur_b = [], 0, 0
        for _, i, e in wins:
            if cur_n and (cur_n + 1 > max_win or cur_b + (e - i) > budget):
                want.append(cur_n)
                cur_n = cur_b = 0
            cur_n += 1
            cur_b += e - i
        if cur_n:
            want.append(cur_n)
        at = 0
        for pi, pc in enumerate(pieces):
            named = [(r, j * S) for r, j0, j1 in pc["slices"] for j in range(j0, j1)]
            mine = wins[at:at + len(named)]
            at += len(named)
            assert named and named == [(r, i) for r, i, _ in mine], (what, pi)  # every window once, in window order; no piece is empty
            sizes = [e - i for _, i, e in mine]
            assert pc["n_win"] == len(named) <= max_win and pc["bases"] == sum(sizes), (what, pi)
            assert pc["bases"] <= budget or len(named) == 1, (what, pi)
            assert pc["wmax"] == max(sizes), (what, pi)
            # the staged text is the copies one behind the other: src[w] is where the window's first base lands in it, the whole window
            # lies in that copy; offs[w] is the prefix of window bases
            assert len(pc["copies"]) == (len(named) if S >= W else len(pc["slices"])), (what, pi)
            starts, pos = [], 0
            for a, n in pc["copies"]:
                starts.append(pos)
                pos += n
            cp = [0]
            for a, n in pc["copies"]:
                cp.append(cp[-1] + (-(-(n - k + 1) // chunk) if n >= k else 0))
            assert pc["cpre"] == cp, (what, pi)
            q, prefix = 0, 0
            assert len(pc["desc"]) == len(named), (what, pi)
            for (src, off), (r, i, e) in zip(pc["desc"], mine):
                while q + 1 < len(starts) and starts[q + 1] <= src:
                    q += 1
                a, n = pc["copies"][q]
                assert starts[q] <= src and src + (e - i) <= starts[q] + n, (what, pi, src)
                assert a + (src - starts[q]) == offs[r] + i, (what, pi, src)
                assert off == prefix, (what, pi, off)
                prefix += e - i
            assert prefix == pc["bases"], (what, pi)  # = offs[n_win], which the last thread copies from vpre's end
            seen.add(("S>=W" if S >= W else "S<W", len(pc["copies"]) > 1, len(named) > 1))
        assert at == len(wins), what
        assert [pc["n_win"] for pc in pieces] == want, what  # the expected equality
    assert {x[0] for x in seen} == {"S>=W", "S<W"} and any(x[1] and x[2] for x in seen)
