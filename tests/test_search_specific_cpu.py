"""kmcp-search --specific-level: what is refused is refused before a file is opened or a GPU touched — status 255, the flag named, no
output file.  (None of these runs gets as far as a database: the -d directory and the input do not exist.)"""
import os
import subprocess

import pytest

from tests import filter_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxdump")
    return FC.write_taxdump(d / "dump"), FC.write_map(d / "map.tsv")


def refused(tmp_path, args, *words):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    out = tmp_path / "out.tsv"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    r = subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq"), "-o", str(out)] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input was looked at
    assert r.stdout == "" and not out.exists()


CASES = [
    (["-K"], "-K/--keep-unmatched"),
    (["--keep-unmatched"], "-K/--keep-unmatched"),
    (["--try-se"], "--try-se"),
    (["-n", "2"], "-n/--keep-top-scores"),
    (["--sliding-step", "100", "--sliding-window", "300"], "--sliding-"),
    (["--sliding-greedy"], "--sliding-"),
    (["--gpus", "2"], "--gpus/--gpu-ids"),
    (["--gpu-ids", "0,1"], "--gpus/--gpu-ids"),
    (["--gpu-passes", "2"], "--gpu-passes"),
    (["--gpu-passes", "0"], "--gpu-passes"),
]


@pytest.mark.parametrize("extra,word", CASES, ids=[" ".join(c[0]) for c in CASES])
@pytest.mark.parametrize("level", ["species", "strain"])
def test_flags_that_cannot_be_combined(tax, tmp_path, extra, word, level):
    dump, tmap = tax
    refused(tmp_path, ["--specific-level", level, "--taxid-map", tmap, "--taxdump", dump] + extra, word, "--specific-level")


def test_taxonomy_flags(tax, tmp_path):
    dump, tmap = tax
    refused(tmp_path, ["--specific-level", "species", "--taxid-map", tmap], "--taxdump is needed when --taxid-map given")
    refused(tmp_path, ["--specific-level", "strain", "--taxid-map", tmap], "--taxdump is needed when --taxid-map given")
    refused(tmp_path, ["--specific-level", "species", "--taxdump", dump], "--taxid-map is needed when --taxdump given")
    refused(tmp_path, ["--specific-level", "species"], "--taxid-map", "--taxdump", "are needed for --specific-level species")
    refused(tmp_path, ["--specific-level", "genus", "--taxid-map", tmap, "--taxdump", dump], "invalid value for --specific-level")
    refused(tmp_path, ["--taxid-map", tmap, "--taxdump", dump], "only used with --specific-level")
    # -T is --min-target-cov here: the long forms only
    refused(tmp_path, ["--specific-level", "species", "-T", tmap, "--taxdump", dump], "invalid argument", "min-target-cov")


def test_strain_level_needs_no_taxonomy_and_gets_as_far_as_the_input(tmp_path):
    """the accepted form is not refused by the flag checks: it fails later, on the input file that does not exist"""
    r = subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq"), "-o", str(tmp_path / "o.tsv"), "--specific-level", "Strain"],
                       capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert r.returncode == 255 and "no-such-reads.fq" in r.stderr and not (tmp_path / "o.tsv").exists()
