"""GPU: sashimi_plot end to end on the reference's own example (tests/golden/sashimi: four BAM files, one skipped-exon
event, its four `.miso` files) with the reference's settings values; what is drawn is read back from the Figure and
compared with the checkers (tests/_density_ref.py, tests/_sashimi_ref.py)."""
import math
import os
from fractions import Fraction

import matplotlib.pyplot as plt
import numpy as np
import pytest
from matplotlib.collections import PolyCollection
from matplotlib.patches import PathPatch

import _density_ref as dref
import _sashimi_ref as sref
from miso_amd import capi, index_gff
from miso_amd import sashimi_plot as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sashimi")
EVENT = "chr17:45816186:45816265:-@chr17:45815912:45815950:-@chr17:45814875:45814965:-"
TX_START, TX_END = 45814875, 45816265
SAMPLES = ["heartWT1", "heartWT2", "heartKOa", "heartKOb"]
COVERAGES = [6830944, 14039751, 4449737, 6720151]
SITES = [(45814965, 45815912), (45814965, 45816186), (45815950, 45816186)]
COUNTS = {"heartWT1": [8, 1, 13], "heartWT2": [31, 7, 25], "heartKOa": [4, 11, 1], "heartKOb": [5, 12, 3]}

SETTINGS = """[data]
bam_prefix = %(golden)s/bam-data/
miso_prefix = %(golden)s/miso-data/
bam_files = [
    "heartWT1.sorted.bam",
    "heartWT2.sorted.bam",
    "heartKOa.sorted.bam",
    "heartKOb.sorted.bam"]
miso_files = ["heartWT1", "heartWT2", "heartKOa", "heartKOb"]
[plotting]
fig_width = 7
fig_height = 5
intron_scale = 30
exon_scale = 4
logged = False
font_size = 6
bar_posteriors = False
ymax = 150
nyticks = 3
nxticks = 4
show_ylabel = True
show_xlabel = True
show_posteriors = True
number_junctions = True
resolution = .5
posterior_bins = 40
gene_posterior_ratio = 5
colors = ["#CC0011", "#CC0011", "#FF8800", "#FF8800"]
coverages = [6830944, 14039751, 4449737, 6720151]
bar_color = "b"
bf_thresholds = [0, 1, 2, 5, 10, 20]
""" % {"golden": GOLDEN}


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("sashimi")
    index_dir = str(d / "index")
    index_gff.index_gff(os.path.join(GOLDEN, "events.gff"), index_dir)
    settings = d / "settings.txt"
    settings.write_text(SETTINGS)
    return index_dir, str(settings), d


def axes_named(fig, prefix):
    return [ax for ax in fig.axes if ax.get_label().startswith(prefix)]


def drawn(ax):
    """(x, y) of the filled polygon's upper edge, [(vertices, line width)] of the arcs, the junction labels."""
    polys = [c for c in ax.collections if isinstance(c, PolyCollection)]
    assert len(polys) == 1
    v = polys[0].get_paths()[0].vertices
    n = (len(v) - 3) // 2                      # first point on y2, n points on y1, last on y2, n back along y2, closing
    arcs = [(p.get_path().vertices.copy(), p.get_linewidth()) for p in ax.patches if isinstance(p, PathPatch)]
    labels = [t.get_text() for t in ax.texts if t.get_text().isdigit()]
    return v[1:n + 1, 0].copy(), v[1:n + 1, 1].copy(), arcs, labels


def expected_series(sample, coverage):
    """The checker's compressed series from its exact densities: float32 x, exact rational y, and per bin (largest number
    of distinct qlen at a base, bases in the bin)."""
    sam = dref.bam_to_sam(os.path.join(GOLDEN, "bam-data", sample + ".sorted.bam"))
    (region,), _ = dref.regions(sam, [("chr17", TX_START, TX_END)])
    gff = [l.split("\t") for l in open(os.path.join(GOLDEN, "events.gff")).read().splitlines()]
    exons = [(int(f[3]), int(f[4])) for f in gff if f[2] == "exon"]
    coords, _ = sref.scaling(TX_START, TX_END, "-", [s for s, _ in exons], [e for _, e in exons], 30, 4.0, False)
    scaled = [1000 * region.exact(b) / Fraction(coverage, 10 ** 6) for b in range(TX_END - TX_START + 1)]
    xs, ys = sref.compression(coords, scaled, .5)
    shape = [(max(region.classes(b) for b in idx), len(idx)) for _, idx in sref.bins(coords, .5)]
    return xs, ys, shape, region, coords, scaled


def check_density_axes(fig):
    dens = axes_named(fig, "density:")
    assert [ax.get_label() for ax in dens] == ["density:%d" % i for i in range(4)]
    u = Fraction(1, 2 ** 53)
    for ax, sample, coverage in zip(dens, SAMPLES, COVERAGES):
        x, y, arcs, labels = drawn(ax)
        xs, ys, shape, region, coords, scaled = expected_series(sample, coverage)
        assert [float(a) for a in x] == [float(b) for b in xs] and len(xs) > 100
        assert any(ys)
        # y against the exact value.  Roundings at unit round-off 2^-53 between the exact density and the drawn mean of a
        # bin of m bases: the density itself 2c (c distinct qlen: the bound of the device pass), the coverage / 1e6, the
        # product with 1e3 and the quotient by the coverage 3, the sum of the m values m - 1 and its division by m 1; one
        # more unit covers the products of these terms.  All values are positive, so the relative errors add.
        for got, want, (c, m) in zip(y, ys, shape):
            assert abs(Fraction(float(got)) - want) <= (2 * c + 3 + m + 1) * u * want, (sample, got, float(want))
        # three arcs: widths from the counts, the count as the label
        counts = [region.jxns[s] for s in SITES]
        assert counts == COUNTS[sample] and len(arcs) == 3
        assert sorted(w for _, w in arcs) == pytest.approx(sorted(math.log(n + 1) / math.log(10) for n in counts), rel=1e-12)
        assert sorted(labels, key=int) == sorted((str(n) for n in counts), key=int)
        for (left, right), n in zip(SITES, counts):
            ss1, ss2 = coords[left - TX_START - 1], coords[right - TX_START]
            mine = [v for v, w in arcs if v[0][0] == ss1 and v[3][0] == ss2]
            assert len(mine) == 1, (sample, left, right)
            v = mine[0]
            if (left, right) == SITES[1]:         # both isoforms have it: below the axis
                assert list(v[:, 1]) == [0, -56.25, -56.25, 0]
            else:                                 # the inclusion isoform alone: above, anchored at the densities
                ends = (float(scaled[left - TX_START - 1]), float(scaled[right - TX_START]))
                assert v[0][1] == pytest.approx(ends[0], rel=1e-12) and v[3][1] == pytest.approx(ends[1], rel=1e-12)
                assert v[1][1] == pytest.approx(ends[0] + 56.25, rel=1e-12)
        assert ax.get_ybound() == (-90.0, 150.0)
        assert [t.get_text() for t in ax.texts if not t.get_text().isdigit()] == [sample + ".sorted.bam"]
    return [drawn(ax) for ax in dens]


def test_plot_event(setup):
    index_dir, settings, d = setup
    out = d / "single"
    fig = sp.plot_event(EVENT, index_dir, settings, str(out))
    assert len(axes_named(fig, "density:")) == 4 and len(axes_named(fig, "posterior:")) == 4
    assert len(axes_named(fig, "gene_model")) == 1 and len(fig.axes) == 9
    check_density_axes(fig)
    # the posterior panels: 39 bars each, the means of the four samples
    for ax, near in zip(axes_named(fig, "posterior:"), [0.79, 0.76, 0.25, 0.25]):
        assert len([p for p in ax.patches if hasattr(p, "get_height")]) == 39
        assert ax.texts[0].get_text().startswith("$\\Psi$ = %.2f" % near)
    # the gene model: 2 + 3 exon boxes
    assert len([p for p in axes_named(fig, "gene_model")[0].patches]) == 5
    assert (out / (EVENT + ".pdf")).read_bytes().startswith(b"%PDF")
    plt.close(fig)


def test_no_posteriors_and_plot_label(setup):
    index_dir, settings, d = setup
    out = d / "labelled"
    fig = sp.plot_event(EVENT, index_dir, settings, str(out), no_posteriors=True, plot_label="x", plot_title="a title")
    assert len(axes_named(fig, "density:")) == 4 and not axes_named(fig, "posterior:") and len(fig.axes) == 5
    assert fig.get_suptitle() == "a title"
    assert os.listdir(str(out)) == ["x.pdf"] and (out / "x.pdf").read_bytes().startswith(b"%PDF")
    plt.close(fig)
    assert sp.main(["--plot-event", EVENT, index_dir, settings, "--output-dir", str(d / "cli"), "--plot-label", "y",
                    "--no-posteriors"]) == 0
    assert os.listdir(str(d / "cli")) == ["y.pdf"]


def test_plot_events(setup, capsys):
    index_dir, settings, d = setup
    single = sp.plot_event(EVENT, index_dir, settings, str(d / "one"))
    want = check_density_axes(single)
    capsys.readouterr()
    figures, unknown = sp.plot_events([EVENT, "no_such_event", EVENT], index_dir, settings, str(d / "many"),
                                      keep_figures=True)
    text = capsys.readouterr().out
    assert unknown == ["no_such_event"] and list(figures) == [EVENT]
    assert text.count("Processing BAM:") == 4                         # each BAM opened once
    got = [drawn(ax) for ax in axes_named(figures[EVENT], "density:")]
    for (x0, y0, arcs0, labels0), (x1, y1, arcs1, labels1) in zip(want, got):
        assert x0.tobytes() == x1.tobytes() and y0.tobytes() == y1.tobytes() and labels0 == labels1
        assert all((a[0] == b[0]).all() and a[1] == b[1] for a, b in zip(arcs0, arcs1)) and len(arcs0) == len(arcs1)
    assert len(figures[EVENT].axes) == 9
    plt.close(single)
    plt.close(figures[EVENT])
    # the command line: the known event's PDF is written, the unknown ID is reported, the status is non-zero
    listing = d / "events.txt"
    listing.write_text("# two lines name the same event\n%s\n\nno_such_event\n%s\n" % (EVENT, EVENT))
    out = d / "cli_many"
    assert sp.main(["--plot-events", str(listing), index_dir, settings, "--output-dir", str(out)]) == 1
    text = capsys.readouterr().out
    assert "no_such_event" in text and text.count("Processing BAM:") == 4
    assert os.listdir(str(out)) == [EVENT + ".pdf"] and (out / (EVENT + ".pdf")).read_bytes().startswith(b"%PDF")
    listing.write_text(EVENT + "\n")
    assert sp.main(["--plot-events", str(listing), index_dir, settings, "--output-dir", str(d / "cli_known")]) == 0
    assert os.listdir(str(d / "cli_known")) == [EVENT + ".pdf"]


def test_chromosome_not_in_the_file(setup, capsys, tmp_path):
    """An event whose chromosome no BAM names: the message of the reference, empty density panels, still a PDF."""
    index_dir, settings, d = setup
    gff = open(os.path.join(GOLDEN, "events.gff")).read().replace("chr17", "chrZ9")
    (tmp_path / "other.gff").write_text(gff)
    other_index = str(tmp_path / "index")
    index_gff.index_gff(str(tmp_path / "other.gff"), other_index)
    event = EVENT.replace("chr17", "chrZ9")
    fig = sp.plot_event(event, other_index, settings, str(tmp_path / "out"), no_posteriors=True)
    assert capsys.readouterr().out.count("Are you sure chrZ9 appears in your BAM file?") == 4
    for ax in axes_named(fig, "density:"):
        assert not ax.collections and not ax.patches
    assert (tmp_path / "out" / (event + ".pdf")).read_bytes().startswith(b"%PDF")
    plt.close(fig)
