"""GPU: every pair of two sample groups in one pass (capi.compare_groups, compare_groups_kernel) against the pairwise call,
bit for bit; samples_utils.output_group_comparisons against output_samples_comparison, byte for byte, on trees with
missing events, shape disagreements, an event outside the device decoder's grammar and a packed tree; and
`--compare-groups` followed by filter_events."""
import os
import shutil

import numpy as np
import pytest

import _filter_ref
from _compare_columns import columns
from _compare_ref import bayes_factor
from miso_amd import capi, filter_events, miso_pack, samples_utils
from test_gpu_compare import BF_RTOL
from test_gpu_miso_text import write_two_sample_trees

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 6)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def planted(S, rng):
    u = rng.random(S)
    step = (1 + np.arange(S) % 3) * 2.0 ** -40
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    return {"planted identical samples": (u, u.copy()),                                   # constant delta
            "planted mad under 0.009": (0.25 + sign * (0.009 - step), np.full(S, 0.25)),
            "planted mad over 0.009": (0.25 + sign * (0.009 + step), np.full(S, 0.25)),
            "planted far apart": (0.99 + 0.01 * rng.random(S), 0.01 * rng.random(S))}     # density 0 -> 1e12


def groups_of(S, n1, n2, seed):
    """(samples1, samples2, cases): samplesN[i] = the events' arrays [S, K] of sample i of group N.  Isoform k of event e
    holds column pair cases[e][k] = (name, u, v): sample i of group 1 has u rotated by i, sample j of group 2 v rotated by
    j, so the pairs (i, i) keep what the pair's name says and the others see other differences."""
    rng = np.random.default_rng(seed)
    col = dict(columns(S, rng))
    col.update(planted(S, rng))
    pairs = [(n,) + tuple(np.asarray(x, dtype=np.float64) for x in uv) for n, uv in col.items()]
    cases, p = [], 0
    for K in KS:
        for _ in range(-(-len(pairs) // K)):
            cases.append([pairs[(p + k) % len(pairs)] for k in range(K)])
            p += K
    def sample(which, r):
        return [np.stack([np.roll(c[which], r) for c in ev], axis=1) for ev in cases]
    return [sample(1, i) for i in range(n1)], [sample(2, j) for j in range(n2)], cases


def check_against_pairwise(b1, b2, arrays1, arrays2, smoothing=0.3, staging="auto", reference=True):
    n_events = len(arrays1[0])
    g = capi.compare_groups(b1, b2, smoothing, staging=staging)
    n_ref = 0
    for i in range(len(b1)):
        for j in range(len(b2)):
            b1[i].compare(b2[j], smoothing)
            for e in range(n_events):
                want, got = b1[i].comparison(e), g.comparison(i, j, e)
                for q in range(4):
                    assert bits(got[q]).tolist() == bits(want[q]).tolist(), (i, j, e, q, got[q], want[q])
                if not reference:
                    continue
                for k in range(arrays1[i][e].shape[1]):
                    bf = got[2][k]
                    if np.isfinite(bf) and 0.0 < bf < 1e12:
                        with np.errstate(all="ignore"):
                            ebf, _ = bayes_factor(arrays1[i][e][:, k], arrays2[j][e][:, k], smoothing)
                        if np.isfinite(ebf) and 0.0 < ebf < 1e12:
                            assert abs(bf - ebf) <= BF_RTOL * ebf, (i, j, e, k, bf, ebf)
                            n_ref += 1
    return g, n_ref


@pytest.mark.parametrize("S", [2, 255, 2700, 8192, 8193, 9000])
@pytest.mark.parametrize("n1, n2", [(3, 2), (1, 1), (4, 4)])
def test_every_pair_has_the_pairwise_call_s_bits(n1, n2, S):
    a1, a2, cases = groups_of(S, n1, n2, seed=1000 * n1 + S)
    b1, b2 = [capi.SamplesBatch(a) for a in a1], [capi.SamplesBatch(a) for a in a2]
    g, n_ref = check_against_pairwise(b1, b2, a1, a2)
    assert n_ref > 0 or S <= 3
    # the planted branches are what they claim, in the pair (0, 0)
    for e, ev in enumerate(cases):
        for k, (name, _, _) in enumerate(ev):
            _, _, bf, dens = g.comparison(0, 0, e)
            if name in ("planted identical samples", "planted mad under 0.009"):
                assert bf[k] == 0.0 and np.isposinf(dens[k]), name
            elif name == "planted mad over 0.009" and S > 3:
                assert bf[k] > 0.0 and np.isfinite(dens[k]), name
            elif name == "planted far apart":
                assert bf[k] == 1e12 and dens[k] == 0.0, name
    if (n1, n2) == (3, 2) and S in (2700, 9000):
        for smoothing in (0.5,):
            check_against_pairwise(b1, b2, a1, a2, smoothing=smoothing)
        for staging in ("both", "smaller", "none"):         # S = 9000: three columns are 216 KB -- `both` cannot fit
            if staging == "both" and S == 9000:
                with pytest.raises(capi.InternalError, match="does not fit"):
                    capi.compare_groups(b1, b2, staging=staging)
            else:
                check_against_pairwise(b1, b2, a1, a2, staging=staging, reference=False)


@pytest.mark.parametrize("n1, n2", [(4, 4), (6, 2), (7, 6)])
def test_more_columns_than_fit_in_lds(n1, n2):
    """Eight samples of 4000 rows are 256 KB of columns (LDS: 160 KiB): the smaller group alone, or nothing, is staged and
    the rest comes from global memory -- the same bits, no error."""
    S = 4000
    a1, a2, _ = groups_of(S, n1, n2, seed=77 + n1)
    b1, b2 = [capi.SamplesBatch(a) for a in a1], [capi.SamplesBatch(a) for a in a2]
    check_against_pairwise(b1, b2, a1, a2, reference=(n1, n2) == (4, 4))


def test_errors_name_the_group_and_the_index():
    rng = np.random.default_rng(3)
    def batch(n=3, K=2, S=50):
        return capi.SamplesBatch([rng.random((S, K)) for _ in range(n)])
    good = [batch(), batch()]
    with pytest.raises(capi.InternalError, match=r"group 2 batch 1: .*differ in events"):
        capi.compare_groups(good, [batch(), batch(n=2)])
    with pytest.raises(capi.InternalError, match=r"group 1 batch 1: .*differ in isoforms"):
        capi.compare_groups([batch(), batch(K=3)], good)
    with pytest.raises(capi.InternalError, match=r"group 2 batch 0: .*samples per event"):
        capi.compare_groups(good, [batch(S=60)])
    empty = capi.Batch(36, iters=50, burn=10, lag=1, chains=1)          # never filled
    with pytest.raises(capi.InternalError, match=r"group 1 batch 2: batch not launched"):
        capi.compare_groups(good + [empty], good)
    with pytest.raises(capi.InternalError, match="at least one batch"):
        capi.compare_groups([], good)
    with pytest.raises(capi.InternalError, match="smoothing"):
        capi.compare_groups(good, good, smoothing=0.0)
    with pytest.raises(capi.InternalError, match="Too few samples"):
        capi.compare_groups([batch(S=1)], [batch(S=1)])
    # (a batch on another device needs a second GPU: on a single-GPU machine this one message stays untested)
    if capi.device_count() > 1:
        other = capi.SamplesBatch([rng.random((50, 2)) for _ in range(3)], device=1)
        with pytest.raises(capi.InternalError, match=r"group 2 batch 1: .*different devices"):
            capi.compare_groups(good, [batch(), other])
    g = capi.compare_groups(good, good)                                   # and the batches are still good for a call
    with pytest.raises(IndexError):
        g.comparison(0, 0, 3)


# ---- trees ----
LABELS = (["ctl1", "ctl2"], ["kd1", "kd2"])


def event_path(tree, name):
    return os.path.join(tree, "chr%d" % (int(name[2:]) % 3), name + ".miso")


def rewrite_rows(path, rows):
    lines = open(path).read().splitlines(keepends=True)
    open(path, "w").write("".join(lines[:2] + rows(lines[2:])))


def four_trees(tmp_path):
    """2 + 2 sample trees: write_two_sample_trees' ctl / kd, and a second replicate of each with every event's sample rows
    rotated (other pairings, so other Bayes factors)."""
    first = write_two_sample_trees(tmp_path / "rep1")
    trees = [[first[0]], [first[1]]]
    for g, (src, shift) in enumerate(zip(first, (7, 13))):
        dst = str(tmp_path / "rep2" / os.path.basename(src))
        shutil.copytree(src, dst)
        for e in range(72):
            rewrite_rows(event_path(dst, "ev%03d" % e), lambda rows: rows[shift:] + rows[:shift])
        trees[g].append(dst)
    return trees


def body_bytes(tree):
    total = 0
    for base, _, files in os.walk(tree):
        for f in files:
            if f.endswith(".miso"):
                data = open(os.path.join(base, f), "rb").read()
                total += len(data) - (data.index(b"\n", data.index(b"\n") + 1) + 1)
    return total


def pairwise_tables(trees, out_dir, decoder):
    tables = {}
    for i, d1 in enumerate(trees[0]):
        for j, d2 in enumerate(trees[1]):
            path, n = samples_utils.output_samples_comparison(d1, d2, out_dir, sample_labels=(LABELS[0][i], LABELS[1][j]),
                                                              decoder=decoder)
            tables[i, j] = (open(path, "rb").read(), n, os.path.relpath(path, out_dir))
    return tables


def group_tables(trees, out_dir, decoder):
    done = samples_utils.output_group_comparisons(trees[0], trees[1], out_dir, LABELS[0], LABELS[1], decoder=decoder)
    tables = {}
    for (path, n), (i, j) in zip(done, [(i, j) for i in range(len(trees[0])) for j in range(len(trees[1]))]):
        tables[i, j] = (open(path, "rb").read(), n, os.path.relpath(path, out_dir))
    return tables, dict(samples_utils.last_decode_stats)


def plant(trees):
    os.remove(event_path(trees[0][0], "ev010"))                                    # missing from one sample each
    os.remove(event_path(trees[1][1], "ev020"))
    rewrite_rows(event_path(trees[0][1], "ev030"), lambda rows: rows[:-10])         # another S in one sample
    def exponents(rows):
        out = []
        for ln in rows:
            psi, score = ln.rstrip("\n").split("\t")
            out.append("%s\t%s\n" % (",".join("%.4e" % float(v) for v in psi.split(",")), score))
        return out
    rewrite_rows(event_path(trees[1][0], "ev007"), exponents)                       # outside the device decoder's grammar


def test_group_tables_are_the_pairwise_tables_byte_for_byte(tmp_path, capsys):
    trees = four_trees(tmp_path)
    # nothing planted: every event takes the group route and every tree's text goes to the device once
    clean, st = group_tables(trees, str(tmp_path / "clean"), "device")
    assert st["text_bytes"] == sum(body_bytes(t) for g in trees for t in g)
    assert (st["samples"], st["pairs"], st["group_events"]) == (4, 4, 72)
    assert st["fallback_events"] == [] and st["pair_route_events"] == []
    assert all(n == 72 for _, n, _ in clean.values())
    assert len({t[0] for t in clean.values()}) == 4                                # four different tables
    want = pairwise_tables(trees, str(tmp_path / "clean_pairwise"), "device")
    assert clean == want

    plant(trees)
    e2e = [[str(tmp_path / "e2e" / LABELS[g][i]) for i in range(2)] for g in range(2)]
    for g in range(2):                                                             # (kept for the end-to-end test below)
        for src, dst in zip(trees[g], e2e[g]):
            shutil.copytree(src, dst)
    assert miso_pack.main(["--pack", trees[1][1]]) == 0                            # one tree packed to .miso_db
    assert all(f.endswith(".miso_db") for f in os.listdir(trees[1][1]))
    capsys.readouterr()
    tables = {}
    for decoder in ("device", "host"):
        want = pairwise_tables(trees, str(tmp_path / "pairwise" / decoder), decoder)
        skipped_pairwise = capsys.readouterr().out.count("Skipping ev030:")
        got, st = group_tables(trees, str(tmp_path / "group" / decoder), decoder)
        skipped_group = capsys.readouterr().out.count("Skipping ev030:")
        assert got == want, [p for p in want if got[p] != want[p]]
        assert skipped_group == skipped_pairwise == 2                              # the two pairs of ctl2
        assert [n for _, n, _ in (got[p] for p in sorted(got))] == [71, 70, 71, 70]
        assert st["decoder"] == decoder and (st["samples"], st["pairs"]) == (4, 4)
        assert st["pair_route_events"] == ["ev030"]
        if decoder == "device":
            # a fallback cannot hide a broken device path: everything but the two planted events went through the kernel
            assert st["fallback_events"] == ["ev007"]
            assert st["group_events"] == 70 and st["compare_kernel_ms"] > 0
        else:
            assert st["fallback_events"] == [] and st["group_events"] == 71        # (the host parser reads exponents)
        tables[decoder] = got
    assert tables["device"] == tables["host"]

    # end to end: --compare-groups, then filter_events with the replicate vote.  filter_events is defined for two-isoform
    # events only (a three-isoform row ends it, tests/test_filter_events.py), so these trees keep the K = 2 events
    for g in range(2):
        for tree in e2e[g]:
            for e in range(72):
                if e % 3 != 0 and os.path.exists(event_path(tree, "ev%03d" % e)):
                    os.remove(event_path(tree, "ev%03d" % e))
    out = str(tmp_path / "e2e_out")
    assert samples_utils.main(["--compare-groups", ",".join(e2e[0]), ",".join(e2e[1]), out]) == 0
    files = [os.path.join(out, n, "bayes-factors", n + ".miso_bf") for n in
             ("%s_vs_%s" % (a, c) for a in LABELS[0] for c in LABELS[1])]
    assert all(os.path.isfile(f) for f in files)
    filtered = str(tmp_path / "filtered")
    assert filter_events.main(["--filter"] + files + ["--votes", "2", "--delta-psi", "0.1", "--bayes-factor", "5",
                                                      "--output-dir", filtered]) == 0
    rows = [_filter_ref.read_table(f)[1] for f in files]
    keep = _filter_ref.multi_filter(rows, vote_thresh=2, delta_psi_filter=0.1, bf_filter=5)
    for f, idx in zip(files, keep):
        src = open(f, "rb").read().splitlines(keepends=True)
        got = open(os.path.join(filtered, os.path.basename(f) + ".filtered"), "rb").read().splitlines(keepends=True)
        assert got == [src[0]] + [src[1 + i] for i in idx]
    keep0 = _filter_ref.multi_filter(rows, vote_thresh=0, delta_psi_filter=0.1, bf_filter=5)
    keep4 = _filter_ref.multi_filter(rows, vote_thresh=4, delta_psi_filter=0.1, bf_filter=5)
    print("end to end: kept", [len(k) for k in keep], "of", [len(r) for r in rows], "before the vote", [len(k) for k in keep0],
          "with four votes", [len(k) for k in keep4])
    # the real tables exercise the thresholds and the vote: rows kept, rows dropped, and events that pass in some of the
    # four tables only, so that the number of votes asked for decides what is kept
    assert all(0 < len(k) < len(r) for k, r in zip(keep, rows))
    assert all(set(k4) <= set(k) <= set(k0) for k4, k, k0 in zip(keep4, keep, keep0))
    assert keep4 != keep
