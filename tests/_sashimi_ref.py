"""Test checker: literal restatements of sashimi_plot's x scaling (plot_gene.py getScaling) and of the loop that thins
the density before it is drawn (plot_density_single:76-87), sharing no code with the package."""
import numpy as np


def scaling(tx_start, tx_end, strand, exon_starts, exon_ends, intron_scale, exon_scale, reverse_minus):
    """(float32 x of every base, {int(x): coordinate}): exon bases advance x by 1 / exon_scale, the others by
    1 / intron_scale, from the left end, or from the right end for "-" with reverse_minus.  x is a double; the array keeps
    float32."""
    n = tx_end - tx_start + 1
    is_exon = [0] * n
    for s, e in zip(exon_starts, exon_ends):
        for k in range(s - tx_start, e - tx_start):
            is_exon[k] = 1
    coords = np.zeros(n, dtype=np.float32)
    back = {}
    x = 0
    forward = strand == "+" or not reverse_minus
    for i in range(n):
        k = i if forward else n - 1 - i
        coords[k] = x
        back[int(x)] = i + tx_start if forward else tx_end - i + 1
        x += 1. / exon_scale if is_exon[k] else 1. / intron_scale
    return coords, back


def bins(coords, resolution):
    """[(x of the bin, [indices in it])]: a bin closes at the first index whose float32 x is more than `resolution` from
    the bin's first x, and that index belongs to the bin it closes; what is still open at the end is dropped."""
    out, first, held = [], coords[0], []
    for i in range(len(coords)):
        held.append(i)
        if abs(np.float32(coords[i]) - np.float32(first)) > resolution:
            out.append((first, held))
            first, held = coords[i], []
    return out


def compression(coords, wiggle, resolution):
    """(x, mean of the bin) per bin; the mean in the arithmetic of the values given (float or Fraction)."""
    made = bins(coords, resolution)
    return [x for x, _ in made], [sum(wiggle[i] for i in idx) / len(idx) for _, idx in made]
