"""The declared plan of test_gpu_k2_forms.py (k2_forms_plan.py) names every instantiation of the COBS kernel that
kmcp_amd/csrc/k2_cobs.hip can launch.  This checks the plan, not what happened to run: it needs no GPU, and holds under -k, -n and
in any order.  A form nobody tests is a red test here."""
import os
import re

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
    assert sorted(set(int(x) for x in re.findall(r"return launch_k2_l<(\d+)>", src))) == list(P.LPRS)
    assert sorted(set(int(x) for x in re.findall(r"launch_k2_t<LPR, (\d+)>", src))) == [8, 10, 16, 24]
    assert sorted(set(int(x) for x in re.findall(r"launch_k2_split_t<(\d+)>", src))) == list(P.LPRS)
    assert sorted(set(int(x) for x in re.findall(r"return launch_k2_pair_t<(\d+), 16>", src))) == [4, 8, 16, 32]
    # one launch site per kernel template, each followed by its note
    assert len(re.findall(r"hipLaunchKernelGGL\(\(k2_cobs<", src)) == 1 and len(re.findall(r"hipLaunchKernelGGL\(\(k2_cobs_pair<", src)) == 1
