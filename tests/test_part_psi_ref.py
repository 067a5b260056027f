"""CPU: part-level psi without a device (miso_amd/part_psi.py): the parts of a gene as isoform groups, the
tables' columns, the restatement the GPU tests compare against (tests/_part_psi_ref.py) on cases worked by hand, the
argument errors of the new options, and MISO_ENODEVICE from both calls where there is no device."""
import ctypes as C

import numpy as np
import pytest

import _pairs_ref as PR
import _part_psi_ref as GR
from _summary_ref import summarize as column_summary
from miso_amd import capi, compare, gene_utils, part_psi, samples_utils


def four_isoform_gene():
    """A in every isoform, D in none, B and B2 with the same coordinates, C in two"""
    parts = [gene_utils.Exon(1, 100, "A"), gene_utils.Exon(201, 300, "B"), gene_utils.Exon(401, 500, "C"),
             gene_utils.Exon(601, 700, "D"), gene_utils.Exon(201, 300, "B2")]
    return gene_utils.Gene([["A", "B", "C"], ["A", "C"], ["A", "B2"], ["A"]], parts, chrom="chr7", label="G4", strand="-")


def test_gene_part_groups():
    got = part_psi.gene_part_groups(four_isoform_gene())
    assert [tuple(g) for g in got] == [("B", 201, 300, 0b0101, [0, 2]), ("C", 401, 500, 0b0011, [0, 1])]
    # the skipped exon of a two-isoform event: isoform 0 alone
    se = gene_utils.se_event_to_gene(100, 50, 100, "chr1", label="se")
    assert [tuple(g) for g in part_psi.gene_part_groups(se)] == [("B", 100, 149, 0b01, [0])]
    # one isoform: every part is in every isoform
    one = gene_utils.Gene([["A"]], [gene_utils.Exon(1, 10, "A")], chrom="c")
    assert part_psi.gene_part_groups(one) == []
    wide = gene_utils.Gene([["A"]] * 64 + [["A", "B"]], [gene_utils.Exon(1, 10, "A"), gene_utils.Exon(20, 30, "B")], chrom="c")
    with pytest.raises(ValueError, match="64 at most"):
        part_psi.gene_part_groups(wide)
    bit63 = gene_utils.Gene([["A"]] * 63 + [["A", "B"]], [gene_utils.Exon(1, 10, "A"), gene_utils.Exon(20, 30, "B")], chrom="c")
    assert part_psi.gene_part_groups(bit63)[0].mask == 1 << 63


def test_event_groups_send_every_mask_once(capsys):
    g4 = four_isoform_gene()
    twice = gene_utils.Gene([["A", "B"], ["A", "B2"], ["A"]],
                            [gene_utils.Exon(1, 9, "A"), gene_utils.Exon(20, 29, "B"), gene_utils.Exon(40, 49, "B2")], chrom="c")
    wide = gene_utils.Gene([["A"]] * 64 + [["A", "B"]], [gene_utils.Exon(1, 10, "A"), gene_utils.Exon(20, 30, "B")], chrom="c",
                           label="W")
    one = gene_utils.Gene([["A"]], [gene_utils.Exon(1, 10, "A")], chrom="c")
    same_mask = gene_utils.Gene([["A", "B", "C"], ["A"]],
                                [gene_utils.Exon(1, 9, "A"), gene_utils.Exon(20, 29, "B"), gene_utils.Exon(40, 49, "C")], chrom="c")
    groups, places = part_psi.event_groups([g4, None, wide, one, twice, same_mask, wide], part_psi._Skipped())
    assert groups == [(0, 0b0101), (0, 0b0011), (4, 0b001), (4, 0b010), (5, 0b01)]
    assert [[(pg.label, g) for pg, g in mine] for mine in places] == \
        [[("B", 0), ("C", 1)], [], [], [], [("B", 2), ("B2", 3)], [("B", 4), ("C", 4)], []]
    err = capsys.readouterr().err
    assert err.count("more than 64 isoforms") == 1 and "W has 65" in err


def test_writers(tmp_path):
    g4 = four_isoform_gene()
    pgs = part_psi.gene_part_groups(g4)
    head = [part_psi._head("ev1", g4, pg) for pg in pgs]
    assert head[0] == ["ev1", "B", "chr7:201-300:-", "0,2", "4"]
    nan = float("nan")
    f = tmp_path / "sub" / "x.miso_part_summary"
    assert part_psi.write_part_summary(str(f), [(head[0], (0.12345, 0.005, 0.995)), (head[1], (nan, nan, nan))]) == 2
    lines = f.read_text().split("\n")
    assert lines[0].split("\t") == ["event_name", "part", "part_coords", "isoforms_with_part", "num_isoforms",
                                    "miso_posterior_mean", "ci_low", "ci_high"]
    assert lines[1] == "ev1\tB\tchr7:201-300:-\t0,2\t4\t0.12\t0.01\t0.99"          # ("%.2f", as the summary's)
    assert lines[2] == "ev1\tC\tchr7:401-500:-\t0,1\t4\tNA\tNA\tNA" and lines[3] == ""
    d = tmp_path / "y.miso_part_dpsi"
    pairs = (0.25, -0.5, 0.75, 30, 10, [8, 4], True, 40)
    bad = (nan, nan, nan, 0, 0, [0, 0], False, 40)
    part_psi.write_part_dpsi(str(d), [(head[0], (0.5, 0.25, 0.75), (0.25, 0.125, 0.5), pairs),
                                      (head[1], (nan,) * 3, (0.25, 0.125, 0.5), bad)], (0.1, 0.2))
    lines = d.read_text().split("\n")
    assert lines[0].split("\t") == (["event_name", "part", "part_coords", "isoforms_with_part", "num_isoforms",
                                     "sample1_posterior_mean", "sample1_ci_low", "sample1_ci_high",
                                     "sample2_posterior_mean", "sample2_ci_low", "sample2_ci_high"]
                                    + compare.DPSI_FIELDS + ["prob_abs_diff_ge_0.1", "prob_abs_diff_ge_0.2"])
    assert lines[0].split("\t")[11:] == compare.dpsi_header_fields((0.1, 0.2))[len(compare.HEADER_FIELDS):]
    assert lines[1].split("\t")[5:] == ["0.50", "0.25", "0.75", "0.25", "0.12", "0.50",
                                        "0.2500", "-0.5000", "0.7500", "0.7500", "0.2500", "0.2000", "0.1000"]
    assert lines[2].split("\t")[5:] == ["NA"] * 3 + ["0.25", "0.12", "0.50"] + ["NA"] * 7
    # the statistics columns are compare.py's, formatted as it formats a column
    as_dpsi = compare.dpsi_fields(([0.25, 0], [-0.5, 0], [0.75, 0], [30, 0], [10, 0], [[8, 4], [0, 0]], [True, True], 40), 2)
    assert lines[1].split("\t")[11:] == as_dpsi
    with pytest.raises(ValueError, match="delta psi threshold"):
        part_psi.write_part_dpsi(str(d), [], (0.1, 1.5))


def test_the_restatement_on_columns_worked_by_hand():
    x = np.array([[0.1, 0.2, 0.7], [0.3, 0.3, 0.4], [-0.0, 0.0, 1.0], [0.12345, 0.00005, 0.8765]])
    assert GR.members(0b101) == [0, 2] and GR.mask_of([0, 2]) == 0b101
    assert GR.group_column(x, 0b101).tolist() == [(0.0 + 0.1) + 0.7, (0.0 + 0.3) + 0.4, 1.0, (0.0 + 0.12345) + 0.8765]
    assert PR.bits(GR.group_column(x, 0b011))[2] == 0                      # -0.0 + 0.0 stored as +0.0
    assert PR.bits(GR.group_column(x, 0b001))[2] == 0
    # as text: 0.12345 prints 0.1235 (the double lies above the tie), 0.00005 prints 0.0001 (likewise)
    assert GR.group_column(x, 0b011, as_text=True)[3] == (0.0 + 0.1235) + 0.0001
    # the sum is left to right over ascending isoforms, not numpy's own order
    y = np.array([[1e16, 1.0, -1e16, 1.0]])
    assert GR.group_column(y, 0b1111)[0] == ((1e16 + 1.0) - 1e16) + 1.0 == 1.0
    # a value that is not finite, in the mask and outside it
    z = np.array([[0.5, np.nan], [0.25, 0.5]] * 40)
    assert all(v != v for v in GR.summarize(z, 0b10)) and all(v != v for v in GR.summarize(z, 0b11))
    assert GR.summarize(z, 0b01) == (0.375, 0.25, 0.5)
    assert PR.same(GR.compare(z, z, 0b10, 0.95, (0.1,)), PR._not_finite(1, 6400))
    # a single bit is the column itself: _summary_ref's numbers, _pairs_ref's numbers
    rng = np.random.default_rng(0)
    s1, s2 = rng.dirichlet(np.ones(3), 257), rng.dirichlet(np.ones(3), 97)
    m, lo, hi = column_summary(s1.T, 0.95)
    for k in range(3):
        assert GR.same3(GR.summarize(s1, 1 << k), (m[k], lo[k], hi[k]))
        assert PR.same(GR.compare(s1, s2, 1 << k, 0.9, (0.1, 0.2)), PR.brute(s1[:, k], s2[:, k], 0.9, (0.1, 0.2)))
    # all bits of a simplex: one, up to the adds' rounding; the difference of two such columns is about zero
    tot = GR.summarize(s1, 0b111)
    assert all(abs(v - 1.0) < 1e-15 for v in tot)
    with pytest.raises(AssertionError):
        GR.strict_ranks(59, 0.95)
    assert GR.strict_ranks(60, 0.95) == (1, 58)


def test_argument_errors(capsys, tmp_path):
    for argv in (["--summarize-parts", str(tmp_path), str(tmp_path / "no_index"), str(tmp_path / "out")],
                 ["--compare-parts", str(tmp_path), str(tmp_path), str(tmp_path / "no_index"), str(tmp_path / "out")]):
        with pytest.raises(SystemExit) as err:
            samples_utils.main(argv)
        assert err.value.code == 2 and "no index directory" in capsys.readouterr().err
    for argv, msg in ((["--summarize-parts", "a", "b"], "expected 3 arguments"),
                      (["--compare-parts", "a", "b", "c"], "expected 4 arguments"),
                      (["--compare-parts", str(tmp_path), str(tmp_path), str(tmp_path), str(tmp_path), "--delta-psi-thresholds",
                        "0.1", "1.5"], "outside (0, 1)"),
                      (["--summarize-parts", str(tmp_path), str(tmp_path), str(tmp_path), "--delta-psi-thresholds", "0.1"],
                       "--delta-psi-thresholds goes with")):
        with pytest.raises(SystemExit) as err:
            samples_utils.main(argv)
        assert err.value.code == 2 and msg in capsys.readouterr().err, argv
    assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="64 bits"):
        capi._group_arrays([(0, 1 << 64)])
    with pytest.raises(ValueError, match="64 bits"):
        capi._group_arrays([(0, -1)])
    ev, mask = capi._group_arrays([(3, 1 << 63), (0, 5)])
    assert ev.dtype == np.int32 and mask.dtype == np.uint64 and mask.tolist() == [1 << 63, 5]


def test_run_options_are_refused_before_any_work(capsys, tmp_path):
    """plain argparse paths of `miso --run --part-psi` and `run_miso --part-psi-file(s)`: no device needed"""
    from miso_amd import miso as miso_cli, run_miso
    from miso_amd.settings import Settings
    try:
        for text, msg in (("[sampler]\nburn_in = 0\nlag = 1\nnum_iters = 5000\nnum_chains = 2\n", "8192 samples per event at most"),
                          ("[sampler]\nburn_in = 0\nlag = 1\nnum_iters = 20\nnum_chains = 2\n", "more samples for a credible interval")):
            settings = tmp_path / "settings.txt"
            settings.write_text(text)
            for main, argv in ((miso_cli.main, ["--run", "idx", "bam", "--output-dir", str(tmp_path / "out"), "--read-len", "36",
                                                "--part-psi"]),
                               (run_miso.main, ["--compute-genes-from-file", "g", "bam", str(tmp_path / "out"), "--read-len", "36",
                                                "--part-psi-file", "f"]),
                               (run_miso.main, ["--compare-genes-from-file", "g", "b1", "b2", "o1", "o2", "bf", "--read-len", "36",
                                                "--part-psi-files", "f1", "f2", "fd"])):
                with pytest.raises(SystemExit) as err:
                    main(argv + ["--settings-filename", str(settings)])
                assert err.value.code == 2 and msg in capsys.readouterr().err, argv
        ok = tmp_path / "ok.txt"
        ok.write_text("[sampler]\nburn_in = 200\nlag = 4\nnum_iters = 1000\nnum_chains = 2\n")
        for argv, msg in ((["--compare-genes-from-file", "g", "b1", "b2", "o1", "o2", "bf", "--read-len", "36", "--part-psi-file", "f"],
                           "--part-psi-file goes with --compute-genes-from-file"),
                          (["--compute-genes-from-file", "g", "bam", "o", "--read-len", "36", "--part-psi-files", "a", "b", "c"],
                           "--part-psi-files goes with --compare-genes-from-file"),
                          (["--compare-genes-from-file", "g", "b1", "b2", "o1", "o2", "bf", "--read-len", "36", "--part-psi-files", "a"],
                           "expected 3 arguments")):
            with pytest.raises(SystemExit) as err:
                run_miso.main(argv + ["--settings-filename", str(ok)])
            assert err.value.code == 2 and msg in capsys.readouterr().err, argv
        with pytest.raises(SystemExit) as err:       # thresholds go with --part-psi only beside --compare
            miso_cli.main(["--run", "idx", "bam", "--output-dir", str(tmp_path / "out"), "--read-len", "36", "--part-psi",
                           "--delta-psi-thresholds", "0.1", "--settings-filename", str(ok)])
        assert err.value.code == 2 and "--delta-psi-thresholds goes with" in capsys.readouterr().err
        assert not (tmp_path / "out").exists()
    finally:
        Settings.load(None)
    assert part_psi.samples_refusal(400) is None and part_psi.samples_refusal(8192) is None and part_psi.samples_refusal(60) is None
    assert "8192" in part_psi.samples_refusal(8193) and "credible interval" in part_psi.samples_refusal(59)


def test_sort_table_orders_events_and_keeps_part_order(tmp_path):
    f = tmp_path / "t"
    f.write_text("event_name\tpart\nG3\tB\nG3\tA\nENS1\tz\nG10\tq\nENS1\ta\n")
    part_psi.sort_table(str(f))
    assert f.read_text() == "event_name\tpart\nENS1\tz\nENS1\ta\nG10\tq\nG3\tB\nG3\tA\n"
    f.write_text("event_name\tpart\n")
    assert open(part_psi.sort_table(str(f))).read() == "event_name\tpart\n"


def test_the_calls_have_no_cpu_path():
    if capi.device_count() > 0:       # (with a device the calls run: tests/test_gpu_part_psi.py)
        return
    b = capi.Batch(36, iters=40, burn=10, lag=1, chains=2)
    with pytest.raises(capi.InternalError, match="no HIP device"):
        b.summarize_isoform_groups([(0, 1)])
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.compare_pairs_isoform_groups(b, b, [(0, 1)])
    L = capi.lib()
    L.miso_batch_summarize_isoform_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int,
                                                      C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
    assert L.miso_batch_summarize_isoform_groups(b.handle, None, None, 0, 0.95, 0, None, 0, None) == capi.MISO_ENODEVICE
    L.miso_batch_compare_pairs_isoform_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double,
                                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                                          C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    assert L.miso_batch_compare_pairs_isoform_groups(b.handle, b.handle, None, None, 0, 0.95, None, 0, 0, None, 0, None,
                                                     None) == capi.MISO_ENODEVICE
