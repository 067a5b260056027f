"""sashimi_plot: RNA-Seq read densities, junction reads and the MISO posterior along an event
(misopy/sashimi_plot/: sashimi_plot.py, Sashimi.py, plot_utils/plot_gene.py, plot_settings.py, plotting.py; parse_gene.py;
miso_utils.get_miso_output_files), for Python 3 and without pysam.

    python -m miso_amd.sashimi_plot --plot-event EVENT INDEX_DIR SETTINGS --output-dir D
                                    [--no-posteriors] [--plot-title T] [--plot-label L]
    python -m miso_amd.sashimi_plot --plot-events FILE INDEX_DIR SETTINGS --output-dir D
    python -m miso_amd.sashimi_plot --plot-insert-len FILE.insert_len SETTINGS --output-dir D
    python -m miso_amd.sashimi_plot --plot-bf-dist FILE.miso_bf SETTINGS --output-dir D

The reference draws one event per process and walks a Python object per read.  Here an alignment file is decoded once
into columns, so the unit of work is a LIST of events: each BAM of the settings file is opened once, the regions of all
events go to the device in one call (capi.region_densities, csrc/kernels_density.hip) and the file is closed before the
next is opened; --plot-event is the one-event case of the same code.  The drawing functions return the matplotlib Figure.

Deviations from the reference: the density is the exact sum of 1 / qlen per base rounded once per
qlen class, not a float32 running sum in file order; --plot-label L writes <output-dir>/L.pdf (the reference's save_plot
raises); chromosome names resolve through sam_utils.resolve_chrom as in the run; --plot-insert-len and --plot-bf-dist work
without --plot-event; nothing is printed per read; isoform rows come in GFF order before the stable sort by exon count.
"""
import ast
import configparser
import math
import os
import sys

import matplotlib
matplotlib.use("pdf")

import matplotlib.pyplot as plt                      # noqa: E402
import numpy as np                                   # noqa: E402
from matplotlib.patches import PathPatch             # noqa: E402
from matplotlib.path import Path                     # noqa: E402
from matplotlib.ticker import FormatStrFormatter     # noqa: E402

from . import gff_utils, miso_db                     # noqa: E402

FLOAT_PARAMS = ("intron_scale", "exon_scale", "ymax", "resolution", "fig_width", "fig_height", "font_size",
                "junction_log_base")
INT_PARAMS = ("posterior_bins", "gene_posterior_ratio", "insert_len_bins", "nyticks", "nxticks")
BOOL_PARAMS = ("logged", "show_posteriors", "number_junctions", "reverse_minus", "bar_posteriors", "show_ylabel",
               "show_xlabel", "sans_serif")
DATA_PARAMS = ("miso_files", "bam_files", "bf_thresholds", "bar_color", "sample_labels")


# ---- settings (plot_settings.py) ----
def get_default_settings():
    return {"intron_scale": 30, "exon_scale": 1, "logged": False, "ymax": None, "show_posteriors": True,
            "number_junctions": True, "posterior_bins": 40, "gene_posterior_ratio": 5, "resolution": .5,
            "fig_width": 8.5, "fig_height": 11, "bar_posteriors": False, "junction_log_base": 10.,
            "reverse_minus": False, "bf_dist_bins": 20, "font_size": 6, "insert_len_bins": 25,
            "bf_thresholds": [0, 1, 2, 5, 10, 20], "nyticks": 3, "nxticks": 4, "show_ylabel": True,
            "show_xlabel": True, "sans_serif": False, "bar_color": "k"}


def parse_plot_settings(settings_filename, event=None, chrom=None, no_posteriors=False):
    """The settings dictionary, every key typed by its kind; keys of no kind stay text.  Exit status 1 when the numbers
    of labels, BAMs, colors and coverages disagree."""
    settings = get_default_settings()
    config = configparser.ConfigParser(interpolation=None)
    print("Reading settings from: %s" % settings_filename)
    config.read(settings_filename)
    for section in config.sections():
        for option in config.options(section):
            if option in FLOAT_PARAMS:
                settings[option] = config.getfloat(section, option)
            elif option in INT_PARAMS:
                settings[option] = config.getint(section, option)
            elif option in BOOL_PARAMS:
                settings[option] = config.getboolean(section, option)
            elif option in DATA_PARAMS:
                settings[option] = ast.literal_eval(config.get(section, option))
            else:
                settings[option] = config.get(section, option)
    settings["bf_thresholds"] = [int(t) for t in settings["bf_thresholds"]]
    settings.setdefault("bam_files", [])
    if "colors" in settings:
        settings["colors"] = ast.literal_eval(settings["colors"])
    else:
        settings["colors"] = [None for _ in settings["bam_files"]]
    if "bam_prefix" in settings:
        settings["bam_files"] = [os.path.join(settings["bam_prefix"], x) for x in settings["bam_files"]]
    if "sample_labels" not in settings:
        settings["sample_labels"] = [os.path.basename(b) for b in settings["bam_files"]]
    counts = (len(settings["sample_labels"]), len(settings["bam_files"]), len(settings["colors"]))
    if not counts[0] == counts[1] == counts[2]:
        print("Error: Must provide sample label and color for each entry in bam_files!")
        print("  - Provided %d labels, %d BAMs, %d colors" % counts)
        sys.exit(1)
    if no_posteriors:
        settings["show_posteriors"] = False
    if "miso_prefix" in settings and event is not None and chrom is not None and settings["show_posteriors"]:
        settings["miso_files"] = get_miso_output_files(event, chrom, settings)
    elif "miso_files" not in settings:
        settings["miso_files"] = []
    if "coverages" in settings:
        settings["coverages"] = [float(x) / 1e6 for x in ast.literal_eval(settings["coverages"])]   # per million
    else:
        settings["coverages"] = [1 for _ in settings["bam_files"]]
    if len(settings["coverages"]) != len(settings["sample_labels"]):
        print("Error: Must provide a coverage value for each sample or leave coverages unset.")
        sys.exit(1)
    return settings


# ---- where a sample's posterior is (miso_utils.get_miso_output_files) ----
def _in_db(db_fname, event_name):
    with miso_db.MISODatabase(db_fname) as db:
        return event_name in db.get_all_event_names()


def get_miso_output_files(event_name, chrom, settings):
    """One source per entry of `miso_files`: the event's `.miso` path (the sample directory's top level first, then the
    first `<chrom>/` directory below it), `<chrom>.miso_db::<event>` for an event held in a packed chromosome, or ''
    for a sample without the event."""
    prefix = os.path.abspath(os.path.expanduser(settings["miso_prefix"])) if "miso_prefix" in settings else ""
    print("miso_prefix: %s" % prefix)
    if "miso_files" not in settings:
        print("Error: need 'miso_files' to be set in settings file in order to plot MISO estimates.")
        return []
    basename = "%s.miso" % event_name
    found = []
    for sample in settings["miso_files"]:
        sample_path = os.path.abspath(os.path.expanduser(os.path.join(prefix, sample)))
        print("Searching for MISO files in: %s" % sample_path)
        print("  - Looking for chromosome %s directories" % chrom)
        source = None
        if os.path.isfile(os.path.join(sample_path, basename)):
            source = os.path.join(sample_path, basename)
            print("Found %s MISO file in top-level directory." % event_name)
        else:
            for root, dirs, files in os.walk(sample_path):
                dirs.sort()
                if chrom in dirs and os.path.isfile(os.path.join(root, chrom, basename)):
                    source = os.path.join(root, chrom, basename)
                elif chrom + miso_db.MISO_DB_EXT in files and _in_db(os.path.join(root, chrom + miso_db.MISO_DB_EXT),
                                                                     event_name):
                    source = "%s::%s" % (os.path.join(root, chrom + miso_db.MISO_DB_EXT), event_name)
                if source:
                    print("Found %s MISO file." % event_name)
                    break
        if source is None:
            print("Error: Could not find MISO output files for sample %s (after searching in %s and its "
                  "subdirectories). Are you sure MISO output files are present in that directory?"
                  % (os.path.basename(sample_path), sample_path))
            source = ""
        else:
            print("  - Location: %s" % source)
        found.append(source)
    return found


def _source_file(source):
    """The file behind a source: the `.miso` path itself, or the database of a `<db>::<event>` source."""
    mark = miso_db.MISO_DB_EXT + "::"
    return source.split(mark, 1)[0] + miso_db.MISO_DB_EXT if mark in source else source


def load_psis(source):
    """The sampled psi of the FIRST isoform, in file order, from a `.miso` path or a `<db>::<event>` source."""
    if miso_db.MISO_DB_EXT + "::" in source:
        db_fname, event_name = source.split(miso_db.MISO_DB_EXT + "::", 1)
        with miso_db.MISODatabase(db_fname + miso_db.MISO_DB_EXT) as db:
            text = db.get_event_data_as_string(event_name)
        if text is None:
            raise KeyError(event_name)
        lines = text.splitlines()
    else:
        with open(source) as handle:
            lines = handle.read().splitlines()
    psis = []
    for line in lines:
        if line and not line.startswith("#") and not line.startswith("sampled"):
            psi, _ = line.strip().split("\t")
            psis.append(float(psi.split(",")[0]))
    return psis


# ---- the event (parse_gene.py) ----
def parse_gene(pickle_filename, event):
    """(tx_start, tx_end, exon_starts, exon_ends, gene_obj, mRNAs, strand, chrom): mRNAs one [start, end] list per
    transcript in GFF order, then stably sorted by exon count."""
    if not os.path.isfile(pickle_filename):
        raise Exception("Error: no filename %s" % pickle_filename)
    gff_genes = gff_utils.load_indexed_gff_file(pickle_filename)
    if event not in gff_genes:
        raise Exception("Event %s not found in %s" % (event, pickle_filename))
    info = gff_genes[event]
    gene_obj, tree = info["gene_object"], info["hierarchy"][event]
    tx_start, tx_end = gff_utils.get_inclusive_txn_bounds(tree)
    exon_starts, exon_ends, mRNAs, strand = [], [], [], None
    for node in tree["mRNAs"].values():
        exons = []
        for exon in node["exons"].values():
            rec = exon["record"]
            strand = rec.strand
            exon_starts.append(rec.start)
            exon_ends.append(rec.end)
            exons.append(sorted([rec.start, rec.end]))
        mRNAs.append(exons)
    mRNAs.sort(key=len)
    return tx_start, tx_end, exon_starts, exon_ends, gene_obj, mRNAs, strand, gene_obj.chrom


def find_event(event_name, index_dir):
    """The event's index file; an exception that names the event when the index does not hold it."""
    event_to_filenames = gff_utils.get_gene_ids_to_gff_index(index_dir)
    if event_name not in event_to_filenames:
        raise Exception("Event %s not found in pickled directory %s. Are you sure this is the right directory for the "
                        "event?" % (event_name, index_dir))
    return event_to_filenames[event_name]


# ---- scaling and compression (plot_gene.py getScaling, plot_density_single:76-87) ----
def get_scaling(tx_start, tx_end, strand, exon_starts, exon_ends, intron_scale, exon_scale, reverse_minus):
    """(graphcoords float32[tx_end - tx_start + 1], graphToGene): the x of every base with exons shrunk by exon_scale and
    introns by intron_scale.  The accumulator is a double; the array keeps float32 as the reference's does."""
    n = tx_end - tx_start + 1
    exoncoords = np.zeros(n)
    for s, e in zip(exon_starts, exon_ends):
        exoncoords[s - tx_start:e - tx_start] = 1
    graph_to_gene = {}
    graphcoords = np.zeros(n, dtype="f")
    x = 0
    if strand == "+" or not reverse_minus:
        for i in range(n):
            graphcoords[i] = x
            graph_to_gene[int(x)] = i + tx_start
            x += 1. / exon_scale if exoncoords[i] == 1 else 1. / intron_scale
    else:
        for i in range(n):
            graphcoords[-(i + 1)] = x
            graph_to_gene[int(x)] = tx_end - i + 1
            x += 1. / exon_scale if exoncoords[-(i + 1)] == 1 else 1. / intron_scale
    return graphcoords, graph_to_gene


def compress_density(graphcoords, wiggle, resolution):
    """The plotted series: a bin closes at the first index whose x is more than `resolution` from the bin's first x; the
    value at that index goes into the bin it closes, and the last open bin is dropped.  The test runs in float32."""
    compressed_x, compressed_wiggle = [], []
    prevx = graphcoords[0]
    values = []
    for i in range(len(graphcoords)):
        values.append(wiggle[i])
        if abs(np.float32(graphcoords[i]) - np.float32(prevx)) > resolution:
            compressed_wiggle.append(np.mean(values))
            compressed_x.append(prevx)
            prevx = graphcoords[i]
            values = []
    return compressed_x, compressed_wiggle


def cubic_bezier(pts, t):
    p0, p1, p2, p3 = (np.array(p, dtype=np.float64) for p in pts)
    return p0 * (1 - t) ** 3 + 3 * t * p1 * (1 - t) ** 2 + 3 * t ** 2 * (1 - t) * p2 + t ** 3 * p3


# ---- the panels ----
def plot_density_single(ax, density, tx_start, tx_end, gene_obj, mRNAs, strand, graphcoords, graph_to_gene,
                        color="r", ymax=None, logged=False, coverage=1, number_junctions=True, resolution=.5,
                        show_x_axis=True, nxticks=4, font_size=6, junction_log_base=10):
    """One sample's density and junction arcs.  density: (wiggle float64[tx_end - tx_start + 1], [(leftss, rightss,
    count)]) from capi.region_densities, or None (the chromosome is not in the file): the panel stays empty."""
    if density is None:
        return ax
    wiggle, jxns = density
    wiggle = 1e3 * np.asarray(wiggle, dtype=np.float64) / coverage
    if logged:
        wiggle = np.log10(wiggle + 1)
    if ymax is None:
        ymax = 1.1 * max(wiggle)
    ymin = -.5 * ymax
    compressed_x, compressed_wiggle = compress_density(graphcoords, wiggle, resolution)
    ax.fill_between(compressed_x, compressed_wiggle, y2=0, color=color, lw=0)
    sslists = [[c for exon in mRNA for c in exon] for mRNA in mRNAs]
    for leftss, rightss, count in jxns:
        ss1, ss2 = graphcoords[leftss - tx_start - 1], graphcoords[rightss - tx_start]
        h = -3 * ymin / 4
        numisoforms = sum(1 for ss in sslists if leftss in ss and rightss in ss)
        if numisoforms == 0:
            continue
        if numisoforms % 2 == 0:                      # below the axis
            pts = [(ss1, 0), (ss1, -h), (ss2, -h), (ss2, 0)]
        else:                                         # above, anchored at the densities
            leftdens, rightdens = wiggle[leftss - tx_start - 1], wiggle[rightss - tx_start]
            pts = [(ss1, leftdens), (ss1, leftdens + h), (ss2, rightdens + h), (ss2, rightdens)]
        midpt = cubic_bezier(pts, .5)
        if number_junctions:
            ax.text(midpt[0], midpt[1], "%s" % count, fontsize=6, ha="center", va="center", backgroundcolor="w")
        arc = Path(pts, [Path.MOVETO, Path.CURVE4, Path.CURVE4, Path.CURVE4])
        ax.add_patch(PathPatch(arc, ec=color, lw=math.log(count + 1) / math.log(junction_log_base), fc="none"))
    ax.spines["right"].set_color("none")
    ax.spines["top"].set_color("none")
    if show_x_axis:
        ax.xaxis.set_ticks_position("bottom")
        ax.set_xlabel('Genomic coordinate (%s), "%s" strand' % (gene_obj.chrom, strand), fontsize=font_size)
        max_graphcoords = max(graphcoords) - 1
        ticks = np.linspace(0, max_graphcoords, nxticks)
        ax.set_xticks(ticks)
        ax.set_xticklabels([graph_to_gene[int(x)] for x in ticks], fontsize=font_size - (font_size * 0.2))
    else:
        ax.spines["bottom"].set_color("none")
        ax.set_xticks([])
    ax.set_xlim(0, max(graphcoords))
    return ax


def py2_round(x):
    """round() of Python 2: halves away from zero."""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def posterior_summary(psis, ci=.95):
    """(mean, lower, upper): the bounds are the sorted samples at round(alpha / 2 * n) - 1 and round((1 - alpha / 2) * n)
    - 1, rounded as Python 2 rounds."""
    alpha = 1 - ci
    ordered = sorted(psis)
    lidx = int(py2_round((alpha / 2) * len(ordered)) - 1)
    hidx = int(py2_round((1 - alpha / 2) * len(ordered)) - 1)
    return np.mean(psis), ordered[lidx], ordered[hidx]


def plot_posterior_single(source, ax, posterior_bins, show_x_axis=True, show_y_axis=True, show_ylabel=True,
                          font_size=6, bar_posterior=False):
    """The posterior of the first isoform's psi: histogram, mean and 95 % interval, or the bar form."""
    psis = load_psis(source)
    mean, clow, chigh = posterior_summary(psis)
    label = "$\\Psi$ = %.2f\n[%.2f, %.2f]" % (mean, clow, chigh)
    if not bar_posterior:
        y, _, _ = ax.hist(psis, np.linspace(0, 1, int(posterior_bins)), density=True, facecolor="k", edgecolor="w",
                          lw=.2)
        ax.axvline(clow, ymin=.33, linestyle="--", dashes=(1, 1), color="#CCCCCC", lw=.5)
        ax.axvline(chigh, ymin=.33, linestyle="--", dashes=(1, 1), color="#CCCCCC", lw=.5)
        ax.axvline(mean, ymin=.33, color="r")
        ymax = max(y) * 1.5
        ymin = -.5 * ymax
        ax.text(1, ymax, label, fontsize=font_size, va="top", ha="left")
        ax.set_ylim(ymin, ymax)
        ax.spines["left"].set_bounds(0, ymax)
        ax.spines["right"].set_color("none")
        ax.spines["top"].set_color("none")
        ax.spines["bottom"].set_position(("data", 0))
        ax.xaxis.set_ticks_position("bottom")
        ax.yaxis.set_ticks_position("left")
        if show_y_axis:
            ticks = np.linspace(0, ymax, 4)
            ax.set_yticks(ticks)
            ax.set_yticklabels(["%d" % t for t in ticks], fontsize=font_size)
        else:
            ax.set_yticks([])
        if show_ylabel:
            ax.set_ylabel("Frequency", fontsize=font_size, ha="right", va="center")
    else:
        ax.errorbar([mean], [1], xerr=[[mean - clow], [chigh - mean]], fmt="o", ms=4, ecolor="k",
                    markerfacecolor="#ffffff", markeredgecolor="k")
        ax.text(1, 1, label, fontsize=font_size, va="top", ha="left")
        ax.set_yticks([])
    ax.set_xlim([0, 1])
    ax.set_xticks([0, .2, .4, .6, .8, 1])
    ax.tick_params(axis="x", labelsize=font_size - (font_size * 0.3))
    shown = ["bottom", "left"] if (not bar_posterior) and show_y_axis else ["bottom"]
    for name in shown:
        ax.spines[name].set_linewidth(0.2)
        ax.xaxis.set_tick_params(size=1.2, color="k")
    if show_x_axis:
        ax.xaxis.set_major_formatter(FormatStrFormatter("%g"))
        for tick_label in ax.get_xticklabels():
            tick_label.set_visible(True)
        ax.set_xlabel("MISO $\\Psi$", fontsize=font_size)
    _show_spines(ax, shown)
    if not show_x_axis:
        for tick_label in ax.get_xticklabels():
            tick_label.set_visible(False)
    return mean, clow, chigh


def _show_spines(ax, spines):
    for loc, spine in ax.spines.items():
        if loc not in spines:
            spine.set_color("none")
    if "left" in spines:
        ax.yaxis.set_ticks_position("left")
    else:
        ax.yaxis.set_ticks([])
    if "bottom" in spines:
        ax.xaxis.set_ticks_position("bottom")
    else:
        ax.xaxis.set_ticks([])


def plot_mRNAs(ax, tx_start, mRNAs, strand, graphcoords, reverse_minus):
    """The gene model: one row per isoform, exons as boxes, the intron line with its direction arrows."""
    exonwidth, narrows = .3, 50
    top = max(graphcoords)
    for yloc, mRNA in enumerate(mRNAs):
        for s, e in mRNA:
            s, e = s - tx_start, e - tx_start
            ax.fill([graphcoords[s], graphcoords[e], graphcoords[e], graphcoords[s]],
                    [yloc - exonwidth / 2, yloc - exonwidth / 2, yloc + exonwidth / 2, yloc + exonwidth / 2],
                    "k", lw=.5, zorder=20)
        ax.axhline(yloc, color="k", lw=.5)
        spread = .2 * top / narrows
        for i in range(narrows):
            loc = float(i) * top / narrows
            if strand == "+" or reverse_minus:
                x = [loc - spread, loc, loc - spread]
            else:
                x = [loc + spread, loc, loc + spread]
            ax.plot(x, [yloc - exonwidth / 5, yloc, yloc + exonwidth / 5], lw=.5, color="k")
    ax.set_xlim(0, top)
    ax.set_ylim(-.5, len(mRNAs) + .5)
    ax.set_frame_on(False)
    ax.set_xticks([])
    ax.set_yticks([])


def plot_density(fig, settings, gene, densities, event, plot_title=None):
    """plot_gene.py plot_density on `fig`: per sample a density panel (label "density:<i>") and, with show_posteriors, a
    posterior panel ("posterior:<i>"), then the gene model ("gene_model").  gene: parse_gene's tuple; densities: one
    entry per sample as plot_density_single takes it."""
    tx_start, tx_end, exon_starts, exon_ends, gene_obj, mRNAs, strand, chrom = gene
    ratio, nyticks, font_size = settings["gene_posterior_ratio"], settings["nyticks"], settings["font_size"]
    colors, ymax, logged = settings["colors"], settings["ymax"], settings["logged"]
    print("Using intron scale ", settings["intron_scale"])
    print("Using exon scale ", settings["exon_scale"])
    graphcoords, graph_to_gene = get_scaling(tx_start, tx_end, strand, exon_starts, exon_ends, settings["intron_scale"],
                                             settings["exon_scale"], settings["reverse_minus"])
    nfiles = len(settings["bam_files"])
    fig.suptitle(plot_title if plot_title is not None else event, fontsize=10)
    plotted_axes = []
    for i in range(nfiles):
        show_x_axis = i == nfiles - 1
        ax1 = plt.subplot2grid((nfiles + 3, ratio), (i, 0), colspan=ratio - 1, fig=fig)
        ax1.set_label("density:%d" % i)
        print("Reading sample label: %s" % settings["sample_labels"][i])
        plot_density_single(ax1, densities[i], tx_start, tx_end, gene_obj, mRNAs, strand, graphcoords, graph_to_gene,
                            color=colors[i], ymax=ymax, logged=logged, coverage=settings["coverages"][i],
                            number_junctions=settings["number_junctions"], resolution=settings["resolution"],
                            show_x_axis=show_x_axis, nxticks=settings["nxticks"], font_size=font_size,
                            junction_log_base=settings["junction_log_base"])
        plotted_axes.append(ax1)
        if settings["show_posteriors"]:
            ax2 = plt.subplot2grid((nfiles + 3, ratio), (i, ratio - 1), fig=fig)
            ax2.set_label("posterior:%d" % i)
            source = os.path.expanduser(settings["miso_files"][i]) if i < len(settings["miso_files"]) else ""
            try:
                if not os.path.isfile(_source_file(source)):
                    print("Warning: MISO file %s not found" % source)
                print("Loading MISO file: %s" % source)
                plot_posterior_single(source, ax2, settings["posterior_bins"], show_x_axis=show_x_axis,
                                      show_ylabel=False, font_size=font_size, bar_posterior=settings["bar_posteriors"])
            except Exception:
                ax2.clear()
                ax2.set_label("posterior:%d" % i)
                ax2.set_frame_on(False)
                ax2.set_xticks([])
                ax2.set_yticks([])
                print("Posterior plot failed.")
    # one y axis for all samples
    if ymax is not None:
        max_used_yval = ymax
    else:
        max_used_yval = math.ceil(max(ax.get_ylim()[1] for ax in plotted_axes))
    fake_ymin = -0.6 * max_used_yval                   # room for the arcs below the axis
    universal_yticks = np.linspace(0, max_used_yval, nyticks + 1)
    for sample_num, ax in enumerate(plotted_axes):
        ax.set_ybound(lower=fake_ymin, upper=max_used_yval)
        labels = ["" if t <= 0 else "%.1f" % t if t % 1 != 0 else "%d" % t for t in universal_yticks]
        ax.spines["left"].set_bounds(0, max_used_yval)
        ax.set_yticks(universal_yticks)
        ax.set_yticklabels(labels, fontsize=font_size)
        ax.yaxis.set_ticks_position("left")
        ax.spines["right"].set_color("none")
        if settings["show_ylabel"]:
            if logged:
                ax.set_ylabel("RPKM $(\\mathregular{\\log}_{\\mathregular{10}})$", fontsize=font_size, ha="left")
            else:
                ax.set_ylabel("RPKM", fontsize=font_size, va="bottom", ha="left")
        if len(universal_yticks) >= 2:
            label_ypos = universal_yticks[-2] + (universal_yticks[-1] - universal_yticks[-2]) / 2.
        else:
            label_ypos = universal_yticks[-1]
        ax.text(max(graphcoords), label_ypos, settings["sample_labels"][sample_num], fontsize=font_size, va="bottom",
                ha="right", color=colors[sample_num])
    ax = plt.subplot2grid((nfiles + 3, ratio), (nfiles + 1, 0), colspan=ratio - 1, rowspan=2, fig=fig)
    ax.set_label("gene_model")
    plot_mRNAs(ax, tx_start, mRNAs, strand, graphcoords, settings["reverse_minus"])
    fig.subplots_adjust(hspace=.10, wspace=.7)
    return fig


# ---- figures (Sashimi.py) ----
def setup_figure(settings):
    if settings["sans_serif"]:
        print("Using sans serif fonts.")
        plt.rcParams["pdf.fonttype"] = 42
        plt.rcParams["font.family"] = "sans-serif"
        plt.rcParams["font.size"] = settings["font_size"]
    print("Setting up plot using dimensions: ", [settings["fig_width"], settings["fig_height"]])
    return plt.figure(figsize=[settings["fig_width"], settings["fig_height"]])


def save_plot(fig, output_dir, label):
    output_filename = os.path.join(os.path.abspath(os.path.expanduser(output_dir)), "%s.pdf" % label)
    print("Saving plot to: %s" % output_filename)
    fig.savefig(output_filename)
    return output_filename


# ---- events ----
def densities_of_bam(bam_file, genes, device=0):
    """The density of every event of `genes` (parse_gene tuples) in one alignment file: opened once, one device call,
    closed.  One entry per event, None where the file has no reference for the event's chromosome."""
    from . import capi, sam_utils
    print("Processing BAM: %s" % bam_file)
    bamfile = sam_utils.Samfile(os.path.expanduser(bam_file))
    try:
        names = [sam_utils.resolve_chrom(bamfile, g[7]) for g in genes]
        have = [k for k, name in enumerate(names) if name in bamfile.references]
        for k, name in enumerate(names):
            if k not in have:
                print("Error retrieving files from %s: no such reference" % genes[k][7])
                print("Are you sure %s appears in your BAM file?" % genes[k][7])
                print("Aborting plot...")
        out = [None] * len(genes)
        if have:
            _, wiggle, jxns, stats = capi.region_densities(bamfile, [names[k] for k in have],
                                                           [genes[k][0] for k in have], [genes[k][1] for k in have],
                                                           device=device)
            for at, k in enumerate(have):
                out[k] = (wiggle[at], jxns[at])
            print("  - %d records fetched, %d with more than one junction skipped, %d without CIGAR skipped"
                  % (stats["fetched"], stats["skipped_multi_n"], stats["skipped_no_cigar"]))
    finally:
        bamfile.close()
    return out


def plot_events(event_names, index_dir, settings_filename, output_dir, no_posteriors=False, plot_title=None,
                plot_label=None, device=0, keep_figures=False):
    """One PDF per event of the list.  Returns (figures by event when keep_figures, else output files by event; the event
    names the index does not hold)."""
    if not os.path.isfile(settings_filename):
        print("Error: settings filename %s not found." % settings_filename)
        sys.exit(1)
    if not os.path.isdir(index_dir):
        print("Error: event pickle directory %s not found." % index_dir)
        sys.exit(1)
    event_to_filenames = gff_utils.get_gene_ids_to_gff_index(index_dir)
    known, unknown = [], []
    for name in dict.fromkeys(event_names):
        (known if name in event_to_filenames else unknown).append(name)
    for name in unknown:
        print("Error: Event %s not found in pickled directory %s." % (name, index_dir))
    if no_posteriors:
        print("Asked to not plot MISO posteriors.")
    genes = [parse_gene(event_to_filenames[name], name) for name in known]
    base = parse_plot_settings(settings_filename, no_posteriors=no_posteriors)
    # every BAM once: all events' regions in one device call
    per_bam = [densities_of_bam(b, genes, device=device) for b in base["bam_files"]] if genes else []
    os.makedirs(output_dir, exist_ok=True)
    results = {}
    for k, name in enumerate(known):
        print("Plotting read densities and MISO estimates along event...")
        print("  - Event: %s" % name)
        settings = parse_plot_settings(settings_filename, event=name, chrom=genes[k][7], no_posteriors=no_posteriors)
        fig = setup_figure(settings)
        plot_density(fig, settings, genes[k], [d[k] for d in per_bam], name, plot_title=plot_title)
        out = save_plot(fig, output_dir, plot_label if plot_label is not None else name)
        if keep_figures:
            results[name] = fig
        else:
            results[name] = out
            plt.close(fig)
    return results, unknown


def plot_event(event_name, index_dir, settings_filename, output_dir, no_posteriors=False, plot_title=None,
               plot_label=None, device=0):
    """Read densities, junctions and posteriors of one event; returns the Figure.  An event the index does not hold is
    an exception that names it."""
    if os.path.isfile(settings_filename) and os.path.isdir(index_dir):
        find_event(event_name, index_dir)
    figures, _ = plot_events([event_name], index_dir, settings_filename, output_dir, no_posteriors=no_posteriors,
                             plot_title=plot_title, plot_label=plot_label, device=device, keep_figures=True)
    return figures[event_name]


def read_event_list(filename):
    """One event ID per line; blank lines and lines starting with # are ignored."""
    with open(filename) as handle:
        return [line.strip() for line in handle if line.strip() and not line.lstrip().startswith("#")]


# ---- the two host-only plots (sashimi_plot.py plot_insert_len, plot_bf_dist) ----
def plot_insert_len(insert_len_filename, settings_filename, output_dir):
    from . import pe_utils
    if not os.path.isfile(settings_filename):
        print("Error: settings filename %s not found." % settings_filename)
        sys.exit(1)
    plot_name = os.path.basename(insert_len_filename)
    settings = parse_plot_settings(settings_filename)
    fig = setup_figure(settings)
    ax = fig.add_subplot(1, 1, 1)
    print("Plotting insert length distribution...")
    print("  - Distribution file: %s" % insert_len_filename)
    insert_dist, _ = pe_utils.load_insert_len(insert_len_filename)
    mean, sdev, dispersion, num_pairs = pe_utils.compute_insert_len_stats(insert_dist)
    print("min insert: %.1f" % min(insert_dist))
    print("max insert: %.1f" % max(insert_dist))
    ax.set_title("%s (%d read-pairs)" % (plot_name, num_pairs), fontsize=10)
    ax.hist(insert_dist, bins=settings["insert_len_bins"], color="k", edgecolor="#ffffff", align="mid")
    ax.set_aspect(1 / ax.get_data_ratio())
    ax.text(0.05, 0.95, "$\\mu$: %.1f\n$\\sigma$: %.1f\n$d$: %.1f" % (round(mean, 2), round(sdev, 2),
                                                                  round(dispersion, 2)),
            horizontalalignment="left", verticalalignment="top",
            bbox=dict(edgecolor="k", facecolor="#ffffff", alpha=0.5), fontsize=10, transform=ax.transAxes)
    ax.set_xlabel("Insert length (nt)")
    ax.set_ylabel("No. read pairs")
    os.makedirs(output_dir, exist_ok=True)
    save_plot(fig, output_dir, plot_name)
    return fig


def plot_bf_dist(bf_filename, settings_filename, output_dir, max_bf=1e12):
    """The number of events at or above each Bayes factor threshold, from a `.miso_bf` table; rows whose Bayes factor is
    a list (more than two isoforms) are skipped."""
    if not bf_filename.endswith(".miso_bf"):
        print("WARNING: %s does not end in .miso_bf, are you sure it is the output of a MISO samples comparison?"
              % bf_filename)
    if not os.path.isfile(settings_filename):
        print("Error: settings filename %s not found." % settings_filename)
        sys.exit(1)
    with open(bf_filename) as handle:
        header = handle.readline().rstrip("\n").split("\t")
        rows = [dict(zip(header, line.rstrip("\n").split("\t"))) for line in handle if line.strip()]
    plot_name = os.path.basename(bf_filename)
    settings = parse_plot_settings(settings_filename)
    fig = setup_figure(settings)
    ax = fig.add_subplot(1, 1, 1)
    bfs = []
    for row in rows:
        if "," in row["bayes_factor"]:
            print("WARNING: %s is a multi-isoform event, skipping..." % row.get("event_name", row))
            continue
        bfs.append(min(max_bf, float(row["bayes_factor"])))
    bfs = np.array(bfs, dtype=np.float64)
    num_events = len(bfs)
    print("Loaded %d event comparisons." % num_events)
    print("Plotting Bayes factors distribution")
    bf_thresholds, bar_color = settings["bf_thresholds"], settings["bar_color"]
    num_events_used = int(np.sum(bfs >= min(bf_thresholds)))
    print("Using BF thresholds: ")
    print(bf_thresholds)
    print("Using bar color: %s" % bar_color)
    ax.set_yscale("log")
    ax.bar(bf_thresholds, [float(np.sum(bfs >= t)) for t in bf_thresholds], align="center", color=str(bar_color),
           edgecolor="#ffffff")
    ax.set_xticks(bf_thresholds)
    ax.set_xlim([bf_thresholds[0] - 1, bf_thresholds[-1] + 1])
    ax.set_title("Bayes factor distributions\n(using %d/%d events)" % (num_events_used, num_events))
    ax.set_xlabel("Bayes factor thresh.")
    ax.set_ylabel("No. events")
    os.makedirs(output_dir, exist_ok=True)
    save_plot(fig, output_dir, plot_name)
    return fig


def greeting():
    print("Sashimi plot: Visualize spliced RNA-Seq reads along gene models. Part of the MISO (Mixture of Isoforms "
          "model) framework.")
    print("See --help for usage.\n")


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Read densities, junction reads and MISO posteriors along events.")
    ap.add_argument("--plot-insert-len", nargs=2, metavar=("INSERT_LEN", "SETTINGS"),
                    help="Plot the insert length distribution of a *.insert_len file.")
    ap.add_argument("--plot-bf-dist", nargs=2, metavar=("MISO_BF", "SETTINGS"),
                    help="Plot the Bayes factor distribution of a *.miso_bf file.")
    ap.add_argument("--plot-event", nargs=3, metavar=("EVENT", "INDEX_DIR", "SETTINGS"),
                    help="Plot read densities and MISO inferences for one event of an indexed GFF.")
    ap.add_argument("--plot-events", nargs=3, metavar=("FILE", "INDEX_DIR", "SETTINGS"),
                    help="The same for every event ID of FILE (one per line; blank lines and # lines ignored): one PDF "
                         "per event, every BAM read once.")
    ap.add_argument("--no-posteriors", action="store_true", help="Do not plot MISO posterior estimates.")
    ap.add_argument("--plot-title", default=None, help="Title at the top of the plot (--plot-event).")
    ap.add_argument("--plot-label", default=None,
                    help="Save the plot in the output directory as <plot_label>.pdf (--plot-event).")
    ap.add_argument("--output-dir", default=None, help="Output directory.")
    ap.add_argument("--device", type=int, default=0, help="HIP device of the density pass.")
    a = ap.parse_args(argv)
    if not (a.plot_event or a.plot_events or a.plot_insert_len or a.plot_bf_dist):
        greeting()
        return 1
    if a.output_dir is None:
        print("Error: need --output-dir")
        return 1
    if a.plot_events and (a.plot_label is not None or a.plot_title is not None):
        print("Error: --plot-label and --plot-title name one plot: use them with --plot-event")
        return 1
    output_dir = os.path.abspath(os.path.expanduser(a.output_dir))
    os.makedirs(output_dir, exist_ok=True)
    full = lambda p: os.path.abspath(os.path.expanduser(p))      # noqa: E731
    status = 0
    if a.plot_insert_len:
        plt.close(plot_insert_len(full(a.plot_insert_len[0]), full(a.plot_insert_len[1]), output_dir))
    if a.plot_bf_dist:
        plt.close(plot_bf_dist(full(a.plot_bf_dist[0]), full(a.plot_bf_dist[1]), output_dir))
    if a.plot_event:
        plt.close(plot_event(a.plot_event[0], full(a.plot_event[1]), full(a.plot_event[2]), output_dir,
                             no_posteriors=a.no_posteriors, plot_title=a.plot_title, plot_label=a.plot_label,
                             device=a.device))
    if a.plot_events:
        _, unknown = plot_events(read_event_list(full(a.plot_events[0])), full(a.plot_events[1]),
                                 full(a.plot_events[2]), output_dir, no_posteriors=a.no_posteriors, device=a.device)
        if unknown:
            print("Error: %d event(s) not in the index: %s" % (len(unknown), ", ".join(unknown)))
            status = 1
    return status


if __name__ == "__main__":
    sys.exit(main())
