"""CPU: the host side of miso_amd/sashimi_plot.py -- settings, event lookup, scaling and compression, the `.miso` lookup,
the posterior panel, and the two plots that need no alignment file."""
import math
import os
import shutil

import matplotlib
import numpy as np
import pytest

import _sashimi_ref as ref
from miso_amd import compare, index_gff, miso_pack, pe_utils
from miso_amd import sashimi_plot as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sashimi")
EVENT = "chr17:45816186:45816265:-@chr17:45815912:45815950:-@chr17:45814875:45814965:-"
SAMPLES = ["heartWT1", "heartWT2", "heartKOa", "heartKOb"]


def test_backend_needs_no_display():
    assert matplotlib.get_backend().lower() == "pdf"


# ---- settings ----
ALL_KINDS = """[data]
bam_prefix = /data/bams
miso_prefix = /data/miso
bam_files = [
    "a.bam",
    "sub/b.bam"]
miso_files = ["a", "b"]
[plotting]
fig_width = 7
fig_height = 5
intron_scale = 30
exon_scale = 4
logged = False
font_size = 6
ymax = 150
nyticks = 3
nxticks = 5
show_posteriors = yes
number_junctions = 0
resolution = .5
posterior_bins = 40
gene_posterior_ratio = 5
colors = ["#CC0011", "#FF8800"]
coverages = [6830944, 14039751]
bar_color = "b"
bf_thresholds = [0, 1.0, 2, 5]
some_text = left as it is
"""


def write(tmp_path, text, name="settings.txt"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_settings_every_kind(tmp_path):
    s = sp.parse_plot_settings(write(tmp_path, ALL_KINDS))
    assert s["fig_width"] == 7.0 and isinstance(s["fig_width"], float) and isinstance(s["font_size"], float)
    assert s["ymax"] == 150.0 and s["exon_scale"] == 4.0 and s["resolution"] == 0.5
    assert s["nxticks"] == 5 and isinstance(s["nxticks"], int) and s["posterior_bins"] == 40
    assert s["logged"] is False and s["show_posteriors"] is True and s["number_junctions"] is False
    assert s["bam_files"] == [os.path.join("/data/bams", "a.bam"), os.path.join("/data/bams", "sub/b.bam")]
    assert s["sample_labels"] == ["a.bam", "b.bam"]                  # the BAM basenames by default
    assert s["miso_files"] == ["a", "b"] and s["miso_prefix"] == "/data/miso"
    assert s["colors"] == ["#CC0011", "#FF8800"]
    assert s["coverages"] == [6830944 / 1e6, 14039751 / 1e6]
    assert s["bar_color"] == "b" and s["bf_thresholds"] == [0, 1, 2, 5]
    assert all(isinstance(t, int) for t in s["bf_thresholds"])
    assert s["some_text"] == "left as it is"
    assert s["reverse_minus"] is False and s["insert_len_bins"] == 25       # untouched defaults
    assert sp.parse_plot_settings(write(tmp_path, ALL_KINDS), no_posteriors=True)["show_posteriors"] is False


def test_settings_defaults(tmp_path):
    d = sp.get_default_settings()
    assert d == {"intron_scale": 30, "exon_scale": 1, "logged": False, "ymax": None, "show_posteriors": True,
                 "number_junctions": True, "posterior_bins": 40, "gene_posterior_ratio": 5, "resolution": .5,
                 "fig_width": 8.5, "fig_height": 11, "bar_posteriors": False, "junction_log_base": 10.,
                 "reverse_minus": False, "bf_dist_bins": 20, "font_size": 6, "insert_len_bins": 25,
                 "bf_thresholds": [0, 1, 2, 5, 10, 20], "nyticks": 3, "nxticks": 4, "show_ylabel": True,
                 "show_xlabel": True, "sans_serif": False, "bar_color": "k"}
    s = sp.parse_plot_settings(write(tmp_path, '[data]\nbam_files = ["x.bam", "y.bam"]\n'))
    assert s["colors"] == [None, None] and s["coverages"] == [1, 1] and s["miso_files"] == []
    assert s["sample_labels"] == ["x.bam", "y.bam"]
    assert {k: v for k, v in s.items() if k in d} == d


@pytest.mark.parametrize("text, message", [
    ('[data]\nbam_files = ["x.bam", "y.bam"]\nsample_labels = ["x"]\n', "Provided 1 labels, 2 BAMs, 2 colors"),
    ('[data]\nbam_files = ["x.bam", "y.bam"]\n[plotting]\ncolors = ["r"]\n', "Provided 2 labels, 2 BAMs, 1 colors"),
    ('[data]\nbam_files = ["x.bam", "y.bam"]\n[plotting]\ncoverages = [1, 2, 3]\n', "Must provide a coverage value"),
])
def test_settings_count_mismatch_exits(tmp_path, capsys, text, message):
    with pytest.raises(SystemExit) as e:
        sp.parse_plot_settings(write(tmp_path, text))
    assert e.value.code == 1 and message in capsys.readouterr().out


# ---- event lookup ----
@pytest.fixture(scope="module")
def index_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("index"))
    index_gff.index_gff(os.path.join(GOLDEN, "events.gff"), d)
    return d


def test_event_lookup(index_dir, tmp_path):
    tx_start, tx_end, exon_starts, exon_ends, gene_obj, mRNAs, strand, chrom = \
        sp.parse_gene(sp.find_event(EVENT, index_dir), EVENT)
    assert (tx_start, tx_end, strand, chrom) == (45814875, 45816265, "-", "chr17")
    assert mRNAs == [[[45816186, 45816265], [45814875, 45814965]],
                     [[45816186, 45816265], [45815912, 45815950], [45814875, 45814965]]]
    assert sorted(zip(exon_starts, exon_ends)) == sorted([(45816186, 45816265), (45815912, 45815950),
                                                          (45814875, 45814965)] + [(45816186, 45816265),
                                                                                   (45814875, 45814965)])
    with pytest.raises(Exception, match="no_such_event"):
        sp.find_event("no_such_event", index_dir)
    settings = write(tmp_path, '[data]\nbam_files = []\n')
    for args in ((EVENT, index_dir, str(tmp_path / "missing.txt")), (EVENT, str(tmp_path / "no_index"), settings)):
        with pytest.raises(SystemExit) as e:
            sp.plot_event(*args, str(tmp_path / "out"))
        assert e.value.code == 1
    with pytest.raises(Exception, match="no_such_event"):
        sp.plot_event("no_such_event", index_dir, settings, str(tmp_path / "out"))


def test_event_list_file(tmp_path):
    p = write(tmp_path, "# picked by hand\n\nev1\n  ev2  \n#ev3\n\nev1\n", "events.txt")
    assert sp.read_event_list(p) == ["ev1", "ev2", "ev1"]


# ---- scaling and compression against the literal restatement of tests/_sashimi_ref.py ----
@pytest.mark.parametrize("exon_scale", [1, 4])
@pytest.mark.parametrize("strand, reverse_minus", [("+", False), ("-", False), ("-", True)])
def test_scaling_and_compression(index_dir, strand, reverse_minus, exon_scale):
    tx_start, tx_end, exon_starts, exon_ends, _, _, _, _ = sp.parse_gene(sp.find_event(EVENT, index_dir), EVENT)
    args = (tx_start, tx_end, strand, exon_starts, exon_ends, 30, exon_scale, reverse_minus)
    coords, back = sp.get_scaling(*args)
    want_coords, want_back = ref.scaling(*args)
    assert coords.dtype == np.float32 and len(coords) == tx_end - tx_start + 1
    assert coords.tobytes() == want_coords.tobytes() and back == want_back
    assert (coords[0] == 0) == (strand == "+" or not reverse_minus) and (coords[-1] == 0) == (strand == "-" and reverse_minus)
    rng = np.random.RandomState(3)
    wiggle = rng.randint(0, 50, len(coords)) / 48.0
    xs, ys = sp.compress_density(coords, wiggle, .5)
    want_xs, want_ys = ref.compression(want_coords, wiggle, .5)
    assert [float(x) for x in xs] == [float(x) for x in want_xs] and len(xs) > 50
    assert all(type(x) is np.float32 for x in xs)
    np.testing.assert_allclose(ys, want_ys, rtol=1e-14, atol=0)
    if not (strand == "-" and reverse_minus):
        # the value at the index that closes a bin belongs to that bin; the open bin at the end is dropped
        first_close = next(i for i in range(len(coords)) if abs(np.float32(coords[i]) - coords[0]) > .5)
        assert ys[0] == pytest.approx(np.mean(wiggle[:first_close + 1]), rel=1e-14)
        assert xs[1] == coords[first_close]


def test_exon_scale_4_sits_on_the_resolution():
    """With exon_scale 4 and resolution .5 two steps of 1/4 are exactly the resolution: inside an exon a bin closes at
    the third step (`>` is strict), so three bases make a bin."""
    coords, _ = sp.get_scaling(1, 40, "+", [1], [41], 30, 4, False)
    xs, ys = sp.compress_density(coords, np.arange(40.0), .5)
    assert [float(x) for x in xs[:3]] == [0.0, 0.75, 1.5]
    assert ys[:2] == [1.5, 5.0]                     # the values 0..3, then 4..6: the closing index stays in the bin


# ---- .miso lookup ----
def miso_tree(tmp_path, layout):
    """A miso_prefix with one sample per layout name."""
    src = os.path.join(GOLDEN, "miso-data", "heartWT1", "chr17", EVENT + ".miso")
    prefix = tmp_path / "miso"
    for sample, how in layout.items():
        d = prefix / sample
        d.mkdir(parents=True)
        if how == "chrom":
            (d / "chr17").mkdir()
            shutil.copy(src, str(d / "chr17" / (EVENT + ".miso")))
        elif how == "nested":
            (d / "run1" / "chr17").mkdir(parents=True)
            shutil.copy(src, str(d / "run1" / "chr17" / (EVENT + ".miso")))
        elif how == "top":
            shutil.copy(src, str(d / (EVENT + ".miso")))
        elif how == "db":
            (d / "chr17").mkdir()
            shutil.copy(src, str(d / "chr17" / (EVENT + ".miso")))
            assert miso_pack.pack_dirs([str(d)]) == 0 and not (d / "chr17").exists()
        elif how == "other":
            (d / "chr17").mkdir()
            shutil.copy(src, str(d / "chr17" / "another_event.miso"))
    return str(prefix)


def test_miso_lookup(tmp_path, capsys):
    layout = {"s_chrom": "chrom", "s_nested": "nested", "s_top": "top", "s_db": "db", "s_other": "other",
              "s_empty": "empty"}
    prefix = miso_tree(tmp_path, layout)
    settings = {"miso_prefix": prefix, "miso_files": list(layout)}
    got = sp.get_miso_output_files(EVENT, "chr17", settings)
    assert got[0] == os.path.join(prefix, "s_chrom", "chr17", EVENT + ".miso")
    assert got[1] == os.path.join(prefix, "s_nested", "run1", "chr17", EVENT + ".miso")
    assert got[2] == os.path.join(prefix, "s_top", EVENT + ".miso")
    assert got[3] == os.path.join(prefix, "s_db", "chr17.miso_db") + "::" + EVENT
    assert got[4] == "" and got[5] == ""
    out = capsys.readouterr().out
    assert out.count("Could not find MISO output files for sample") == 2 and "sample s_other" in out
    want = sp.load_psis(os.path.join(GOLDEN, "miso-data", "heartWT1", "chr17", EVENT + ".miso"))
    assert len(want) == 360
    for source in got[:4]:
        assert sp.load_psis(source) == want
    assert sp.get_miso_output_files(EVENT, "chr17", {"miso_prefix": prefix}) == []


# ---- the posterior panel ----
def parsed_column(sample):
    rows = [l for l in open(os.path.join(GOLDEN, "miso-data", sample, "chr17", EVENT + ".miso")).read().splitlines()
            if not l.startswith("#") and not l.startswith("sampled")]
    return np.array([float(r.split("\t")[0].split(",")[0]) for r in rows])


def py2_round(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


@pytest.mark.parametrize("sample, near", zip(SAMPLES, [0.79, 0.76, 0.25, 0.25]))
def test_posterior_panel(sample, near):
    import matplotlib.pyplot as plt
    col = parsed_column(sample)
    n = len(col)
    ordered = np.sort(col)
    want = (np.mean(col), ordered[py2_round(0.025 * n) - 1], ordered[py2_round(0.975 * n) - 1])
    assert abs(want[0] - near) < 0.006
    source = os.path.join(GOLDEN, "miso-data", sample, "chr17", EVENT + ".miso")
    fig = plt.figure()
    ax = fig.add_subplot(1, 1, 1)
    got = sp.plot_posterior_single(source, ax, 40)
    assert got[0] == pytest.approx(want[0], rel=1e-15) and got[1:] == want[1:]
    heights, _ = np.histogram(col, np.linspace(0, 1, 40), density=True)
    bars = [p for p in ax.patches if hasattr(p, "get_height")]
    assert len(bars) == 39
    np.testing.assert_allclose([b.get_height() for b in bars], heights, rtol=1e-12)
    assert ax.get_ylim() == pytest.approx((-.75 * max(heights), 1.5 * max(heights)))
    lines = sorted(l.get_xdata()[0] for l in ax.lines)
    assert lines == pytest.approx(sorted(want))
    assert ax.get_xlim() == (0, 1) and ax.texts[0].get_text() == "$\\Psi$ = %.2f\n[%.2f, %.2f]" % want
    plt.close(fig)
    # the bar form: the mean with the interval as its error bar
    fig = plt.figure()
    ax = fig.add_subplot(1, 1, 1)
    assert sp.plot_posterior_single(source, ax, 40, bar_posterior=True)[1:] == want[1:]
    assert not [p for p in ax.patches if hasattr(p, "get_height")] and ax.get_yticks().size == 0
    plt.close(fig)


def test_python2_rounding_of_the_interval():
    # 0.025 * 100 = 2.5: Python 2 rounds to 3, Python 3's round() to 2
    psis = [i / 100.0 for i in range(100)]
    assert sp.posterior_summary(psis)[1:] == (0.02, 0.97)
    assert sp.py2_round(2.5) == 3 and sp.py2_round(3.5) == 4 and round(2.5) == 2


# ---- the plots that need no alignment file ----
def test_plot_insert_len(tmp_path):
    import matplotlib.pyplot as plt
    rng = np.random.RandomState(1)
    dists = {"chr1:%d-%d" % (k * 1000, k * 1000 + 900): rng.normal(250, 20, 80).astype(np.int64) for k in range(5)}
    name = "sample.bam.insert_len"
    pe_utils.summarize_insert_len_dist(dists, str(tmp_path / name))
    settings = write(tmp_path, "[plotting]\ninsert_len_bins = 12\nfig_width = 4\nfig_height = 4\n")
    out = tmp_path / "plots"
    assert sp.main(["--plot-insert-len", str(tmp_path / name), settings, "--output-dir", str(out)]) == 0
    assert (out / (name + ".pdf")).read_bytes().startswith(b"%PDF")
    fig = sp.plot_insert_len(str(tmp_path / name), settings, str(out))
    inserts, _ = pe_utils.load_insert_len(str(tmp_path / name))
    ax = fig.axes[0]
    assert len(ax.patches) == 12 and sum(p.get_height() for p in ax.patches) == len(inserts)
    assert ax.get_title() == "%s (%d read-pairs)" % (name, len(inserts))
    plt.close(fig)


def test_plot_bf_dist(tmp_path, capsys):
    import matplotlib.pyplot as plt
    head = {"isoforms": "'a','b'", "counts": "(0,1):5", "assigned_counts": "0:3,1:2", "chrom": "chr1", "strand": "+",
            "mRNA_starts": "1,1", "mRNA_ends": "9,9"}
    bfs = [0.3, 1.5, 4.0, 12.0, 30.0, 1e14, -2.0]
    rows = [("ev%d" % k, ([0.6, 0.4], [0.5, 0.3], [0.7, 0.5]), ([0.3, 0.7], [0.2, 0.6], [0.4, 0.8]), [bf, bf], head, head)
            for k, bf in enumerate(bfs)]
    three = ([0.5, 0.3, 0.2], [0.4, 0.2, 0.1], [0.6, 0.4, 0.3])
    rows.append(("multi", three, three, [3.0, 4.0, 5.0], head, head))
    name = "a_vs_b.miso_bf"
    assert compare.write_comparison(str(tmp_path / name), rows) == 8
    settings = write(tmp_path, '[plotting]\nbar_color = "b"\nbf_thresholds = [0, 1, 2, 5, 10, 20]\n')
    out = tmp_path / "plots"
    assert sp.main(["--plot-bf-dist", str(tmp_path / name), settings, "--output-dir", str(out)]) == 0
    assert (out / (name + ".pdf")).read_bytes().startswith(b"%PDF")
    text = capsys.readouterr().out
    assert text.count("is a multi-isoform event, skipping...") == 1 and "Loaded 7 event comparisons." in text
    fig = sp.plot_bf_dist(str(tmp_path / name), settings, str(out))
    ax = fig.axes[0]
    assert ax.get_title() == "Bayes factor distributions\n(using 6/7 events)"        # -2 is below every threshold
    assert [p.get_height() for p in ax.patches] == [6, 5, 4, 3, 3, 2] and ax.get_yscale() == "log"
    plt.close(fig)


def test_no_option_greets_and_fails(capsys):
    assert sp.main([]) == 1 and "Sashimi plot" in capsys.readouterr().out
    assert sp.main(["--plot-bf-dist", "x.miso_bf", "s.txt"]) == 1 and "need --output-dir" in capsys.readouterr().out
