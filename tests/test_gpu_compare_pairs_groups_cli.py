"""GPU: `samples_utils --compare-groups G1 G2 OUT --delta-posterior` end to end on 2 + 2 sample trees (those of
tests/test_gpu_compare_groups.py: an event missing from one replicate, one whose rows were cut in one sample, one outside
the device decoder's grammar, one tree packed).  The pairwise `.miso_dpsi` are the `--compare-samples --delta-posterior`
runs' byte for byte, the `.miso_bf` those of a run without the flag, and the pooled `.miso_group_dpsi` is the restatement
(tests/_group_pairs_ref.py on the parsed `.miso` files) as compare.dpsi_fields formats it."""
import os
import shutil

import pytest

import _group_pairs_ref as GR
from _summary_ref import tree_mean
from miso_amd import compare, miso_pack, samples_utils
from test_gpu_compare_groups import LABELS, event_path, four_trees, plant

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.1, 0.25)
PAIRS = [(i, j) for i in range(2) for j in range(2)]


def files_under(top):
    out = {}
    for d, _, files in os.walk(top):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), top)] = open(os.path.join(d, f), "rb").read()
    return out


def pair_paths(out_dir, ext):
    return [os.path.join(out_dir, n, "bayes-factors", n + ext) for n in
            ("%s_vs_%s" % (LABELS[0][i], LABELS[1][j]) for i, j in PAIRS)]


def expected_group_rows(trees, thresholds, level=0.95):
    """the pooled table's rows from the unpacked trees' `.miso` files: {event: fields}"""
    have = [[{} for _ in g] for g in trees]
    for g in range(2):
        for r, tree in enumerate(trees[g]):
            for e in range(72):
                p = event_path(tree, "ev%03d" % e)
                if os.path.exists(p):
                    have[g][r]["ev%03d" % e] = samples_utils.parse_miso_file(p)
    rows = {}
    for name in sorted(set().union(*have[0]) & set().union(*have[1])):
        reps = [[h[name] for h in have[g] if name in h] for g in range(2)]
        head = [name, "%d" % len(reps[0]), "%d" % len(reps[1])]
        hdr = reps[0][0][2]
        tail = [hdr.get(k, "NA") for k in ("isoforms", "chrom", "strand", "mRNA_starts", "mRNA_ends")]
        if len({x[1].shape for x in reps[0] + reps[1]}) > 1:
            rows[name] = head + ["NA"] * (3 + 5 + len(thresholds)) + tail
            continue
        K = reps[0][0][1].shape[1]
        ref = [GR.brute([x[1][:, k] for x in reps[0]], [x[1][:, k] for x in reps[1]], level, thresholds) for k in range(K)]
        pairs = ([x[0] for x in ref], [x[1] for x in ref], [x[2] for x in ref], [x[3] for x in ref], [x[4] for x in ref],
                 [x[5] for x in ref], [x[6] for x in ref], ref[0][7])
        m = [compare.group_mean([[tree_mean(x[1][:, k]) for k in range(K)] for x in reps[g]]) for g in range(2)]
        ks = [0] if K == 2 else range(K)
        means = [",".join("%.4f" % m[g][k] for k in ks) for g in range(2)] + [",".join("%.4f" % (m[0][k] - m[1][k]) for k in ks)]
        rows[name] = head + means + compare.dpsi_fields(pairs, len(thresholds)) + tail
    return rows


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pairs_groups_cli")
    trees = four_trees(tmp)
    plant(trees)
    unpacked = [[str(tmp / "kept" / LABELS[g][r]) for r in range(2)] for g in range(2)]
    for g in range(2):
        for src, dst in zip(trees[g], unpacked[g]):
            shutil.copytree(src, dst)
    return tmp, trees, unpacked


def group_run(trees, out_dir, decoder, delta=True, names=None):
    done = samples_utils.output_group_comparisons(trees[0], trees[1], out_dir, LABELS[0], LABELS[1], decoder=decoder,
                                                  delta_thresholds=THRESHOLDS if delta else None, group_names=names)
    return done, dict(samples_utils.last_decode_stats)


def test_tables_of_a_group_run(runs, capsys):
    tmp, trees, unpacked = runs
    out = str(tmp / "group")
    capsys.readouterr()
    done, st = group_run(trees, out, "device")
    said = capsys.readouterr().out
    # one notice per call and cause: ev030's rows were cut in one sample
    assert said.count("No pooled delta psi for events whose samples differ") == 1 and "ev030" in said
    assert said.count("No pooled delta psi") == 1
    assert st["fallback_events"] == ["ev007"] and st["pair_route_events"] == ["ev030"] and st["pairs_groups_kernel_ms"] > 0
    table = os.path.join(out, "group1_vs_group2", "delta-psi", "group1_vs_group2.miso_group_dpsi")
    assert done[-1] == (table, 72) and [p for p, _ in done[:4]] == pair_paths(out, ".miso_bf")

    # the `.miso_bf` are those of a run without the flag, which writes nothing else
    plain_out = str(tmp / "plain")
    plain, _ = group_run(trees, plain_out, "device", delta=False)
    assert len(plain) == 4
    got, want = files_under(out), files_under(plain_out)
    assert all(f.endswith(".miso_bf") for f in want) and len(want) == 4
    assert {f: d for f, d in got.items() if f.endswith(".miso_bf")} == want
    assert sorted(f for f in got if not f.endswith(".miso_bf")) == sorted(
        [os.path.relpath(p, out) for p in pair_paths(out, ".miso_dpsi")] + [os.path.relpath(table, out)])

    # the pairwise `.miso_dpsi` are the four --compare-samples --delta-posterior runs', byte for byte
    pw = str(tmp / "pairwise")
    for i, j in PAIRS:
        samples_utils.output_samples_comparison(trees[0][i], trees[1][j], pw, sample_labels=(LABELS[0][i], LABELS[1][j]),
                                                decoder="device", delta_thresholds=THRESHOLDS)
    assert files_under(pw) == {f: d for f, d in got.items() if f != os.path.relpath(table, out)}

    # the pooled table against the restatement
    lines = [ln.split("\t") for ln in open(table).read().splitlines()]
    assert lines[0] == compare.group_dpsi_header_fields(THRESHOLDS)
    want_rows = expected_group_rows(unpacked, THRESHOLDS)
    assert [ln[0] for ln in lines[1:]] == sorted(want_rows) and len(want_rows) == 72
    for ln in lines[1:]:
        assert ln == want_rows[ln[0]], (ln, want_rows[ln[0]])
    by_name = {ln[0]: ln for ln in lines[1:]}
    assert by_name["ev010"][1:3] == ["1", "2"] and by_name["ev020"][1:3] == ["2", "1"]      # missing from one replicate
    assert by_name["ev030"][1:3] == ["2", "2"] and set(by_name["ev030"][3:13]) == {"NA"}     # the pair route: NA
    assert by_name["ev007"][1:3] == ["2", "2"] and "NA" not in by_name["ev007"][3:13]        # the fallback: still pooled
    assert "," in by_name["ev001"][6] and "," not in by_name["ev000"][6]                    # three isoforms, two


def test_packed_trees_the_host_decoder_and_the_command_line(runs, capsys):
    tmp, trees, unpacked = runs
    table = lambda out, a="group1", b="group2": open(os.path.join(out, "%s_vs_%s" % (a, b), "delta-psi",  # noqa: E731
                                                                  "%s_vs_%s.miso_group_dpsi" % (a, b)), "rb").read()
    group_run(unpacked, str(tmp / "unpacked_device"), "device")
    want = table(str(tmp / "unpacked_device"))
    want_all = files_under(str(tmp / "unpacked_device"))
    group_run(unpacked, str(tmp / "unpacked_host"), "host")
    assert files_under(str(tmp / "unpacked_host")) == want_all
    packed = [[str(tmp / "packed" / LABELS[g][r]) for r in range(2)] for g in range(2)]
    for g in range(2):
        for src, dst in zip(unpacked[g], packed[g]):
            shutil.copytree(src, dst)
    assert miso_pack.main(["--pack", packed[1][1]]) == 0 and miso_pack.main(["--pack", packed[0][0]]) == 0
    assert all(f.endswith(".miso_db") for f in os.listdir(packed[1][1]))
    for decoder in ("device", "host"):
        group_run(packed, str(tmp / ("packed_" + decoder)), decoder)
        assert files_under(str(tmp / ("packed_" + decoder))) == want_all, decoder
    # the command line, with names and thresholds of its own
    out = str(tmp / "cli")
    capsys.readouterr()
    assert samples_utils.main(["--compare-groups", ",".join(packed[0]), ",".join(packed[1]), out, "--delta-posterior",
                               "--delta-psi-thresholds"] + ["%g" % t for t in THRESHOLDS] + ["--group-names", "ctl", "kd"]) == 0
    assert "ctl_vs_kd.miso_group_dpsi" in capsys.readouterr().out
    assert table(out, "ctl", "kd") == want
    assert all(os.path.isfile(p) for p in pair_paths(out, ".miso_dpsi"))
