"""The declared plan of test_gpu_k2_forms.py (k2_forms_plan.py) names every instantiation of the COBS kernel that
kmcp_amd/csrc/k2_cobs.hip can launch.  This checks the plan, not what happened to run: it needs no GPU, and holds under -k, -n and
in any order.  A form nobody tests is a red test here.  And the plan's own statement of the dispatch rules (lane_classes, expect) is
held against the rules themselves: kmcp_amd/csrc/k2_plan.hpp compiled for the host (tests/k2_forms_print.cpp) decides every case."""
import os
import re
import subprocess

import pytest

from tests import k2_forms_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_covers_every_instantiation():
    planned = set()
    for c in P.CASES:
        planned |= set(c.expect)
    missing = sorted(P.ALL_FORMS - planned)
    assert not missing, "no case of the plan expects: " + ", ".join(P.fmt(f) for f in missing)
    stray = sorted(planned - P.ALL_FORMS)
    assert not stray, "the plan expects forms the launchers do not have: " + ", ".join(P.fmt(f) for f in stray)
    assert len(P.ALL_FORMS) == 78


def test_override_only_forms_are_reached_by_their_override_alone():
    for form, why in P.OVERRIDE_ONLY.items():
        assert form in P.ALL_FORMS
        with_override = [c for c in P.CASES if form in c.expect]
        assert with_override and all(P.DB[c.db].open_env for c in with_override), (P.fmt(form), why)
    # the 4-row forms: by KMCPG_GROUP_ROWS=4, and by the default rule on the one index of 4 GiB
    for c in P.CASES:
        if any(f[5] == 4 for f in c.expect):
            assert c.env.get("KMCPG_GROUP_ROWS") == "4" or c.db == P.BIG.key, c.id
    assert any(c.db == P.BIG.key and c.expect == (("plain", 8, 0, 8, False, 4),) for c in P.CASES)


def test_case_ids_are_unique_and_layouts_consistent():
    ids = [c.id for c in P.CASES]
    assert len(ids) == len(set(ids))
    for l in P.LAYOUTS:
        assert l.cols % 8 != 0, l.name
        row = (l.cols + 7) // 8 * (l.blocks if l.step == 0 else 1)
        pitch = lambda a: 16 if row <= 16 else 32 if row <= 32 else 64 if row <= 64 else (row + a - 1) // a * a  # noqa: E731
        assert l.stride1 == pitch(64) and l.stridem == (pitch(128) if row > 128 else pitch(64)), l.name
        if l.step == 0:
            assert ((l.cols + 7) // 8) % 16 != 0, l.name  # segments of a fused group start off the 16-byte grid
    # every lane class on a layout of its own and on a fused one, with one and with several hash functions
    for nh in (1, 3):
        for fused in (False, True):
            seen = set()
            for d in P.DBS:
                if d.nh == nh and (P.LAYOUT[d.layout].step == 0) == fused:
                    seen |= set(P.lane_classes(P.stride_of(d), d.nh, d.open_env)[0])
            assert seen == set(P.LPRS), (nh, fused, seen)
    for batch, ns in P.BATCH_N.items():
        top = {8: 254, 10: 1022, 16: 65534, 24: 65535}[batch]
        assert max(ns) == top and P.planes_for(max(ns)) == batch
        assert 0 in ns and len(ns) % 4 != 0
    assert 255 in P.BATCH_N[10] and 1023 in P.BATCH_N[16] and 65535 in P.BATCH_N[24]
    # the last workgroup of every plain launch is part-filled: units = reads x slots of the lane class, 4 waves of 64 / lpr units each
    for d in P.DBS:
        classes, slots = P.lane_classes(P.stride_of(d), d.nh, d.open_env)
        groups = 1 if P.LAYOUT[d.layout].step == 0 else P.LAYOUT[d.layout].blocks
        for c in classes:
            for batch, ns in P.BATCH_N.items():
                assert (len(ns) * groups * slots[c]) % (4 * (64 // c)) != 0, (d.key, c, batch)


def test_launch_sites_match_the_parameter_sets():
    """the parameter sets ALL_FORMS is built from are the ones the switch statements of k2_cobs.hip dispatch on"""
    src = open(os.path.join(ROOT, "kmcp_amd", "csrc", "k2_cobs.hip")).read()
    ints = lambda pat: sorted(int(x) for x in re.findall(pat, src))  # noqa: E731  (every match: a case written twice shows)
    # plain: lanes x (planes, rows), both MULTI values at the one place that names the launch site
    assert ints(r"case (\d+): return launch_k2_plain_l<\1>\(") == list(P.LPRS)
    plain = sorted((int(p), int(g)) for p, g in re.findall(r"launch_k2_pieces<LPR, (\d+), false, (\d+)>\(", src))
    assert plain == sorted([(p, 8) for p in (8, 10, 16, 24)] + [(p, 4) for p in (8, 10)])
    for p in (8, 10, 16, 24):    # ... each under the case of its own plane count
        assert len(re.findall(r"case %d: return four \?[^;]*launch_k2_pieces<LPR, %d, false, 8>\(" % (p, p), src)) == 1
    # chunked: lanes, 16 planes, 8 rows
    assert ints(r"case (\d+): return launch_k2_pieces<\1, 16, true, 8>\(") == list(P.LPRS)
    assert len(re.findall(r"launch_k2_pieces<[^>]*true, \d+>\(", src)) == len(P.LPRS)
    # pair: 64 lanes + a narrower form, 16 planes
    assert ints(r"case (\d+): return launch_k2_pair_l<\1>\(") == [4, 8, 16, 32]
    assert sorted(re.findall(r"launch_k2_pair_form<64, LPRB, 16, (\w+)>\(", src)) == ["false", "true"]
    assert sorted(re.findall(r"launch_k2_form<LPR, NPL, (\w+), SPLIT, GR>\(", src)) == ["false", "true"]
    assert len(re.findall(r"launch_k2_form<", src)) == 2 and len(re.findall(r"launch_k2_pair_form<", src)) == 2  # those and no other call
    # one launch site per kernel template, each followed by its note
    assert len(re.findall(r"hipLaunchKernelGGL\(\(k2_cobs<", src)) == 1 and len(re.findall(r"hipLaunchKernelGGL\(\(k2_cobs_pair<", src)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(\(k2_cobs<LPR, NPL, MULTI, SPLIT, GR>\)[^\n]*\n  note_k2\(log, SPLIT \? 1 : 0, LPR, 0, NPL, MULTI, GR, nb\);", src)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(\(k2_cobs_pair<LPRA, LPRB, NPL, MULTI>\)[^\n]*\n  note_k2\(log, 2, LPRA, LPRB, NPL, MULTI, 8, nba \+ nbb\);", src)) == 1
    # the launchers decide nothing: no unit or grid arithmetic, no refusal by size, is left in the file
    for gone in ("K2_MAX_BLOCKS", "k2_blocks", "group_rows", "slot_major", "nslots", "std::min<uint64_t>"):
        assert gone not in src[src.index("static void note_k2("):src.index("__global__ void k_list_long(")].replace("r.group_rows = gr;", ""), gone


@pytest.fixture(scope="module")
def decided(tmp_path_factory):
    """case id -> (ask, [(lpr, slots of one group)], [forms in launch order]) as k2_row_parts / k2_ask_long / k2_plan decide"""
    exe = str(tmp_path_factory.mktemp("k2forms") / "k2_forms_print")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "k2_forms_print.cpp")], check=True)
    lines = []
    for c in P.CASES:
        db, ns = P.DB[c.db], P.BATCH_N[c.batch]
        lay, oenv = P.LAYOUT[db.layout], dict(db.open_env)
        groups = 1 if lay.step == 0 else lay.blocks
        split_min = int(c.env.get("KMCPG_SPLIT_MIN", P.SPLIT_DEFAULT))
        longs = [n for n in ns if n > split_min]         # what the device lists, where it is asked
        index_bytes = db.num_sigs * 128 if db is P.BIG else 0
        f = [c.id, P.stride_of(db), db.nh, groups, int(oenv.get("KMCPG_LPR8", 1)), int(oenv.get("KMCPG_LPR32", 1)), int(oenv.get("KMCPG_SPLIT_TILES", -1)),
             len(ns), max(ns), index_bytes, len(longs), max(longs, default=0),
             int("KMCPG_SPLIT_MIN" in c.env), split_min, int("KMCPG_SPLIT_CHUNK" in c.env), int(c.env.get("KMCPG_SPLIT_CHUNK", 0)), int(c.env.get("KMCPG_PRUNE", 1)),
             int("KMCPG_GROUP_ROWS" in c.env), int(c.env.get("KMCPG_GROUP_ROWS", 0)), int(c.env.get("KMCPG_PRUNE_EVERY", 1)), int(c.env.get("KMCPG_SLOT_MAJOR", 1)),
             int(c.env.get("KMCPG_PAIR", 1))]
        lines.append(" ".join(str(x) for x in f))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = {}
    for ln in r.stdout.splitlines():
        cid, ask, classes, forms = ln.split()
        cl = [tuple(int(x) for x in c.split(":")) for c in classes.split(",")]
        fm = []
        for f in ([] if forms == "-" else forms.split(",")):
            kind, lpr, lprb, npl, multi, gr = f.split("/")
            fm.append((kind, int(lpr), int(lprb), int(npl), bool(int(multi)), int(gr)))
        out[cid] = (bool(int(ask)), cl, fm)
    return out


def test_the_rule_cuts_the_lane_classes_the_plan_declares(decided):
    assert len(decided) == len(P.CASES)
    for c in P.CASES:
        db = P.DB[c.db]
        classes, slots = P.lane_classes(P.stride_of(db), db.nh, db.open_env)
        assert decided[c.id][1] == [(lpr, slots[lpr]) for lpr in classes], c.id


def test_the_rule_launches_the_forms_the_plan_declares(decided):
    n_big = 0
    for c in P.CASES:
        _, classes, forms = decided[c.id]
        assert tuple(sorted(forms)) == c.expect, (c.id, forms, c.expect)
        # launch order: the plain forms in class order (or the pair), then the chunked forms in class order
        order = [lpr for lpr, _ in classes]
        first = [f for f in forms if f[0] != "split"]
        assert forms == first + [f for f in forms if f[0] == "split"], c.id
        assert [f[1] for f in first] in (order, [64]) and [f[1] for f in forms if f[0] == "split"] in (order, []), c.id
        n_big += c.db == P.BIG.key
    assert n_big == 2  # the 4-row forms by the default rule: the index of 4 GiB and more
