"""CPU: miso_amd/filter_events.py against tests/_filter_ref.py (the reference's row test and vote restated) and against
sets written down by hand, on the hand-made tables of tests/golden/filter/."""
import os
import shutil
import subprocess
import sys

import pytest

import _filter_ref
from miso_amd import filter_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "filter")
REPS = [os.path.join(GOLD, "rep%d.miso_bf" % i) for i in (1, 2, 3)]
BOUNDARY = os.path.join(GOLD, "boundary.miso_bf")

# product keyword -> reference keyword
KW = {"num_total": "num_total", "num_inc": "num_inc", "num_exc": "num_exc", "num_sum": "num_sum",
      "delta_psi_filter": "delta_psi_filter", "bf_filter": "bf_filter", "apply_both_samples": "apply_both_samples"}


def lines_of(path):
    with open(path, "rb") as f:
        return f.read().splitlines(keepends=True)


def names_of(path):
    return [ln.split(b"\t")[0].decode() for ln in lines_of(path)[1:]]


def run_filter(files, out_dir, votes=0, same_direction=False, **kw):
    """multi_filter's outputs; every one checked to be the header + a verbatim subsequence of its input, and to hold
    exactly the rows _filter_ref selects."""
    done = filter_events.multi_filter(files, str(out_dir), vote_thresh=votes, votes_same_direction=same_direction,
                                      out=open(os.devnull, "w"), **kw)
    tables = [_filter_ref.read_table(f)[1] for f in files]
    want = _filter_ref.multi_filter(tables, vote_thresh=votes, same_direction=same_direction, **{KW[k]: v for k, v in kw.items()})
    got = []
    for (fname, n_kept, n_read), src, idx in zip(done, files, want):
        assert fname == os.path.join(str(out_dir), os.path.basename(src) + ".filtered")
        src_lines, out_lines = lines_of(src), lines_of(fname)
        assert out_lines[0] == src_lines[0]                                  # the header, byte for byte
        assert out_lines[1:] == [src_lines[1 + i] for i in idx]              # the reference's rows, verbatim, in input order
        assert (n_kept, n_read) == (len(idx), len(src_lines) - 1)
        got.append(names_of(fname))
    return got


ALL_BOUNDARY = names_of(BOUNDARY)


@pytest.mark.parametrize("kw, fails", [
    (dict(delta_psi_filter=0.20), ["dpsi_under", "dpsi_neg_under", "dpsi_zero"]),
    (dict(delta_psi_filter=-0.20), ["dpsi_under", "dpsi_neg_under", "dpsi_zero"]),       # |threshold|
    (dict(bf_filter=10), ["bf_under", "bf_neg_under"]),
    (dict(num_total=100), ["total_under", "neither_sample", "only_zero_class"]),
    (dict(num_total=100, apply_both_samples=True),
     ["total_under", "only_sample1", "only_sample2", "neither_sample", "only_zero_class"]),
    (dict(num_inc=10), ["inc_under", "neither_sample", "no_inc_class", "only_zero_class"]),
    (dict(num_exc=5), ["exc_under", "neither_sample", "no_exc_class", "only_zero_class"]),
    (dict(num_sum=20), ["sum_under", "neither_sample", "only_zero_class"]),
    (dict(), []),
])
def test_every_threshold_at_under_and_over_its_boundary(tmp_path, kw, fails):
    (got,) = run_filter([BOUNDARY], tmp_path, **kw)
    assert got == [n for n in ALL_BOUNDARY if n not in fails]


def test_all_thresholds_together(tmp_path):
    (got,) = run_filter([BOUNDARY], tmp_path, delta_psi_filter=0.20, bf_filter=10, num_total=100, num_inc=10, num_exc=5,
                        num_sum=20)
    assert "dpsi_at" in got and "dpsi_neg_at" in got and "bf_neg_at" in got and "bf_cap" in got
    assert all(n.endswith(("_at", "_over")) or n in ("bf_cap", "only_sample1", "only_sample2") for n in got), got


def test_counts_lacking_a_class():
    assert filter_events.get_counts("(0,0):50,(1,0):120") == (120, 0, 0)
    assert filter_events.get_counts("(0,1):120,(1,1):12") == (0, 120, 12)
    assert filter_events.get_counts("(0,0):500") == (0, 0, 0)
    assert filter_events.get_counts("(0,0):3,(0,1):4,(1,0):6,(1,1):10") == (6, 4, 10)


PASS = {1: ["ev_all_up", "ev_two_up", "ev_one", "ev_mixed", "ev_only_in_1_and_2"],
        2: ["ev_mixed", "ev_all_up", "ev_two_up", "ev_zero", "ev_only_in_1_and_2", "ev_only_in_2"],
        3: ["ev_all_up", "ev_mixed", "ev_zero", "ev_only_in_3"]}
KEPT = {0: None, 1: None, 2: {"ev_all_up", "ev_two_up", "ev_mixed", "ev_zero", "ev_only_in_1_and_2"},
        3: {"ev_all_up", "ev_mixed"}, 4: set()}


@pytest.mark.parametrize("votes", [0, 1, 2, 3, 4])
def test_votes_over_three_replicates(tmp_path, votes):
    got = run_filter(REPS, tmp_path, votes=votes, delta_psi_filter=0.10, bf_filter=5)
    for i, names in zip((1, 2, 3), got):
        assert names == [n for n in PASS[i] if KEPT[votes] is None or n in KEPT[votes]]


def test_one_file_ignores_votes(tmp_path):
    (got,) = run_filter([REPS[0]], tmp_path, votes=3, delta_psi_filter=0.10, bf_filter=5)
    assert got == PASS[1]


def test_votes_same_direction(tmp_path):
    got = run_filter(REPS, tmp_path / "a", votes=2, same_direction=True, delta_psi_filter=0.10, bf_filter=5)
    kept = {"ev_all_up", "ev_two_up", "ev_mixed", "ev_only_in_1_and_2"}           # ev_zero: one up, one down
    assert [set(g) for g in got] == [set(PASS[i]) & kept for i in (1, 2, 3)]
    got = run_filter(REPS, tmp_path / "b", votes=3, same_direction=True, delta_psi_filter=0.10, bf_filter=5)
    assert [set(g) for g in got] == [{"ev_all_up"}] * 3                            # ev_mixed: up, down, down
    # no delta-psi threshold: ev_zero passes in all three files with diff 0.00, 0.15, -0.12 -- no two of one sign
    got = run_filter(REPS, tmp_path / "c", votes=2, same_direction=True, bf_filter=5)
    assert all("ev_zero" not in g for g in got)
    got = run_filter(REPS, tmp_path / "d", votes=2, bf_filter=5)
    assert all("ev_zero" in g for g in got)
    got = run_filter(REPS, tmp_path / "e", votes=1, same_direction=True, bf_filter=5)
    assert "ev_zero" in got[1] and "ev_zero" in got[2] and "ev_zero" in got[0]


def cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "miso_amd.filter_events"] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=120)


def test_cli_writes_the_reference_s_summary_line_and_ignores_control(tmp_path):
    r = cli(["--filter"] + REPS + ["--control", BOUNDARY, "--votes", "2", "--delta-psi", "0.1", "--bayes-factor", "5",
                                   "--output-dir", str(tmp_path)])
    assert r.returncode == 0, r.stdout
    assert "--control is ignored" in r.stdout
    assert "4/7 events pass the filter (57.14 percent)." in r.stdout
    assert "5/8 events pass the filter (62.50 percent)." in r.stdout
    assert "3/6 events pass the filter (50.00 percent)." in r.stdout
    assert names_of(str(tmp_path / "rep3.miso_bf.filtered")) == ["ev_all_up", "ev_mixed", "ev_zero"]
    assert sorted(os.listdir(str(tmp_path))) == ["rep%d.miso_bf.filtered" % i for i in (1, 2, 3)]
    # "0.50" stays "0.50", the isoform names keep their quotes: the rows are not re-formatted
    kept = lines_of(str(tmp_path / "rep1.miso_bf.filtered"))[1]
    assert b"\t0.50\t" in kept and b"'ev.A.up_ev.A.se_ev.A.dn','ev.A.up_ev.A.dn'" in kept


def test_a_three_isoform_row_ends_the_run_with_status_1_and_no_output(tmp_path):
    out = tmp_path / "out"
    r = cli(["--filter", REPS[0], os.path.join(GOLD, "three_isoforms.miso_bf"), "--output-dir", str(out)])
    assert r.returncode == 1, r.stdout
    assert "only defined for MISO output on two-isoform alternative events" in r.stdout
    assert "Found a non-two isoform event: three" in r.stdout
    assert not out.exists() or os.listdir(str(out)) == []
    with pytest.raises(filter_events.NotTwoIsoforms):
        filter_events.multi_filter([os.path.join(GOLD, "three_isoforms.miso_bf")], str(out))
    assert not out.exists() or os.listdir(str(out)) == []
    assert filter_events.num_isoforms("'a','b'") == 2 and filter_events.num_isoforms("'a_1','b,2','c'") == 3
    assert filter_events.num_isoforms("'only'") == 1


def test_delta_psi_above_one_is_an_error(tmp_path):
    with pytest.raises(ValueError, match="delta psi"):
        filter_events.multi_filter([REPS[0]], str(tmp_path / "o"), delta_psi_filter=1.01)
    with pytest.raises(ValueError, match="delta psi"):
        filter_events.multi_filter([REPS[0]], str(tmp_path / "o"), delta_psi_filter=-1.5)
    assert not (tmp_path / "o").exists()
    filter_events.multi_filter([REPS[0]], str(tmp_path / "ok"), delta_psi_filter=1.0, out=open(os.devnull, "w"))
    r = cli(["--filter", REPS[0], "--delta-psi", "2", "--output-dir", str(tmp_path / "o")])
    assert r.returncode not in (0, 1) and "delta psi" in r.stdout


def test_duplicate_base_names_are_an_error(tmp_path):
    other = tmp_path / "elsewhere"
    other.mkdir()
    shutil.copy(REPS[1], str(other / "rep1.miso_bf"))
    with pytest.raises(ValueError, match="rep1.miso_bf"):
        filter_events.multi_filter([REPS[0], str(other / "rep1.miso_bf")], str(tmp_path / "o"))
    assert not (tmp_path / "o").exists()


def test_an_empty_table(tmp_path, capsys):
    empty = os.path.join(GOLD, "empty.miso_bf")
    done = filter_events.multi_filter([empty], str(tmp_path))
    assert done == [(str(tmp_path / "empty.miso_bf.filtered"), 0, 0)]
    assert "0/0 events pass the filter (0.00 percent)." in capsys.readouterr().out
    assert lines_of(done[0][0]) == lines_of(empty)
    got = run_filter([empty] + REPS[:2], tmp_path / "with", votes=1, delta_psi_filter=0.10, bf_filter=5)
    assert got[0] == [] and got[1] == PASS[1]


def test_the_module_runs_on_the_host_alone():
    """filter_events neither imports capi nor loads the device library."""
    code = ("import sys, miso_amd.filter_events as f; from miso_amd import capi; "
            "assert capi._lib is None; assert 'capi' not in vars(f)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
