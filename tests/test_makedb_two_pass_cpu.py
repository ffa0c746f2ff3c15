"""kmcp-makedb --two-pass, what needs no GPU: the two flags are parsed (every spelling, the size suffixes of the other size flags),
--matrix-budget without --two-pass is refused with status 255 naming both flags, and --dry-run --two-pass prints what --dry-run prints
(nothing about the plan is known without sketching)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEDB = os.path.join(ROOT, "kmcp_amd", "kmcp-makedb")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from kmcp_amd import lib
    if not (os.path.exists(lib.LIB_PATH) and os.path.exists(MAKEDB)):
        g.build()
    return lib


def run(args):
    return subprocess.run([MAKEDB] + args, capture_output=True, text=True, timeout=120)


@pytest.fixture()
def fasta(tmp_path):
    fa = tmp_path / "g1.fa"
    fa.write_text(">a\n" + "ACGTTGCAACGGATCCATGA" * 40 + "\n>b\n" + "TTGACCAGTAGGCATCGATC" * 30 + "\n")
    return str(fa)


def test_matrix_budget_needs_two_pass(built, tmp_path, fasta):
    out = str(tmp_path / "o.kmcp")
    for spelling in (["--matrix-budget", "1G"], ["--matrix-budget=512M"]):
        for dry in ([], ["--dry-run"]):
            r = run(["-k", "21", "-O", out] + spelling + dry + [fasta])
            assert r.returncode == 255, (r.returncode, r.stderr)
            assert "--matrix-budget" in r.stderr and "--two-pass" in r.stderr, r.stderr
            assert not os.path.exists(out)


@pytest.mark.parametrize("args, word", [
    (["--two-pass", "--matrix-budget", "12x"], "invalid size"),
    (["--two-pass", "--matrix-budget", "0"], "--matrix-budget"),
    (["--two-pass", "--matrix-budget"], "flag needs an argument: --matrix-budget"),
    (["--two-pass", "--circular"], "--circular"),          # the refusals of one-pass mode stand
    (["--two-pass", "-s", "1000"], "--split-size"),
    (["--two-pass", "--two-pas"], "unknown flag: --two-pas\n"),  # the flag itself is known, a near miss is not
])
def test_two_pass_flag_refusals(built, tmp_path, fasta, args, word):
    out = str(tmp_path / "o.kmcp")
    r = run(["-k", "21", "-O", out, fasta] + args)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert word in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_dry_run_two_pass_prints_what_dry_run_prints(built, tmp_path, fasta):
    out = str(tmp_path / "o.kmcp")
    base = ["-k", "21", "-n", "3", "-l", "10", "-m", "0", "-O", out, "--dry-run", fasta]
    plain = run(base)
    assert plain.returncode == 0 and plain.stdout == "g1\t%d\t3\n" % (800 + 20 + 600), plain.stdout + plain.stderr
    for extra in (["--two-pass"], ["--two-pass", "--matrix-budget", "64M"], ["--matrix-budget=2g", "--two-pass"], ["--two-pass", "--matrix-budget", "1.5K"]):
        r = run(extra + base)
        assert r.returncode == 0, r.stderr
        assert r.stdout == plain.stdout and r.stderr == plain.stderr
    assert not os.path.exists(out)
    assert "--two-pass" in run(["--help"]).stdout and "--matrix-budget" in run(["--help"]).stdout
