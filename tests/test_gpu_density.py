"""GPU: the density pass of sashimi_plot (csrc/kernels_density.hip, capi.region_densities) against the restatement in
tests/_density_ref.py: a seeded random file as SAM, BAM and shuffled SAM at several chunk sizes and accumulator budgets,
the corner cases of the rules, and the four real files of tests/golden/sashimi."""
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import _density_ref as ref
from _bam import sam_to_bam
from miso_amd import capi, sam_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sashimi")
EVENT_REGION = ("chr17", 45814875, 45816265)
# the junction counts of the four real files as the issue of this feature lists them: records, then the counts of
# 45814965:45815912, 45814965:45816186, 45815950:45816186
REAL = {"heartWT1": (81, 8, 1, 13), "heartWT2": (167, 31, 7, 25), "heartKOa": (61, 4, 11, 1), "heartKOb": (52, 5, 12, 3)}
SITES = [(45814965, 45815912), (45814965, 45816186), (45815950, 45816186)]


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible")


# the corner region: nothing random lands near it
S, E = 2600000, 2601000


def corner_records():
    """(name suffix, pos0, cigar) on chr3 around the corner region [S, E]."""
    return [
        ("left", S - 20, "50M"),                 # straddles tx_start
        ("right", E - 20, "50M"),                # straddles tx_end
        ("last", E - 1, "50M"),                  # pos == tx_end - 1: fetched, covers tx_end - 1 and tx_end
        ("out", E, "50M"),                       # pos == tx_end: not fetched (rule 1), though rule 4 would take tx_end
        ("ls_at_start", S - 10, "10M100N30M"),   # leftss == tx_start: x = tx_start - 1 is outside, no junction
        ("ls_after_start", S - 9, "10M100N30M"),  # leftss == tx_start + 1: counts
        ("rs_before_end", E - 2 - 120, "20M100N30M"),   # rightss == tx_end - 1: counts
        ("rs_at_end", E - 1 - 120, "20M100N30M"),       # rightss == tx_end: no junction
        ("ls_before_end", E - 2 - 19, "20M100N30M"),    # leftss == tx_end - 1, rightss beyond: no junction
        ("rs_after_start", S - 120, "20M100N30M"),      # rightss == tx_start + 1 but leftss before tx_start: none
        ("d_gap", S + 300, "30M5D20M"),          # a junction from a D
        ("d_and_n", S + 400, "20M3D10M200N20M"),  # two from one record
        ("only_clip", S + 500, "50S"),           # fetched, no aligned position: adds nothing
        ("ins", S + 600, "25M2I23M"),
    ]


def build_case(seed):
    """~10^5 records on three references and ~300 regions: nested, overlapping, duplicate, one on an absent reference,
    one with start > end, one of at least 300 kb, and the corner region.  Returns (regions, sam text, shuffled sam text)."""
    rng = random.Random(seed)
    refs = ["chr1", "2", "chr3"]
    regions = [("chr1", 100000, 420000)]                        # at least 300 kb
    for g in range(296):
        r = rng.random()
        if r < 0.1:                                             # nested in an earlier region
            seqid, s, e = regions[rng.randrange(len(regions))]
            start = rng.randint(s, e)
            end = rng.randint(start, min(e, start + 20000))
        elif r < 0.15:                                          # a duplicate
            seqid, start, end = regions[rng.randrange(len(regions))]
        elif r < 0.25:                                          # overlapping an earlier one
            seqid, s, e = regions[rng.randrange(len(regions))]
            start = rng.randint(max(1, s - 500), e)
            end = start + rng.randint(300, 5000)
        else:
            seqid = rng.choice(refs)
            start = rng.randint(1, 2000000)
            end = start + rng.randint(300, 20000)
        regions.append((seqid, start, end))
    regions.append(("chr9", 1, 3000000))                        # a reference the file lacks
    regions.append(("chr1", 5000, 4000))                        # start > end
    regions.append(("chr3", S, E))
    recs = []

    def cigar():
        u = rng.random()
        if u < 0.40: return "50M"
        if u < 0.48: return "36M"
        if u < 0.53: return "76M"
        if u < 0.68: return "20M%dN30M" % rng.randint(10, 3000)
        if u < 0.74: return "15M%dN10M%dN25M" % (rng.randint(10, 900), rng.randint(10, 900))    # two N: skipped
        if u < 0.79: return "30M5D20M"
        if u < 0.83: return "20M%dD10M%dN20M" % (rng.randint(1, 9), rng.randint(10, 2000))
        if u < 0.87: return "25M2I23M"
        if u < 0.91: return "10S40M"
        if u < 0.94: return "40M10S"
        if u < 0.97: return "20=5X25M"
        return "*"
    for i in range(100000):
        if rng.random() < 0.6:                                  # near a region
            seqid, s, e = regions[rng.randrange(297)]
            pos0 = max(0, rng.randint(s - 200, min(e, s + 30000) + 50) - 1)
        else:
            seqid, pos0 = rng.choice(refs), rng.randint(0, 2400000)
        flag = rng.choice([0, 0, 0, 16, 256, 1024, 512, 4, 99, 147])       # no flag filters anything
        recs.append("q%d\t%d\t%s\t%d\t50\t%s\t*\t0\t0\t*\t*" % (i, flag, seqid, pos0 + 1, cigar()))
    for name, pos0, cg in corner_records():
        recs.insert(rng.randrange(len(recs)), "%s\t0\tchr3\t%d\t50\t%s\t*\t0\t0\t*\t*" % (name, pos0 + 1, cg))
    head = "".join("@SQ\tSN:%s\tLN:3000000\n" % r for r in refs)
    shuffled = list(recs)
    rng.shuffle(shuffled)
    return regions, head + "\n".join(recs) + "\n", head + "\n".join(shuffled) + "\n"


SEED = 11


@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("density")
    regions, sam, shuffled = build_case(SEED)
    paths = {"sam": str(d / "reads.sam"), "bam": str(d / "reads.bam"), "shuffled": str(d / "shuffled.sam")}
    open(paths["sam"], "w").write(sam)
    open(paths["shuffled"], "w").write(shuffled)
    sam_to_bam(sam, paths["bam"], block=60000)
    want = {"sam": ref.regions(sam, regions), "shuffled": ref.regions(shuffled, regions)}
    want["bam"] = want["sam"]                                    # the same records in the same order
    return regions, paths, want


def test_the_case_is_not_vacuous(random_case):
    """On the checker's output alone."""
    regions, _, want = random_case
    got, stats = want["sam"]
    assert sum(1 for r in got if r.depth.any()) >= 100
    assert sum(1 for r in got if r.jxns) >= 50
    assert sum(r.d_junctions for r in got) >= 1
    assert stats["skipped_multi_n"] > 1000
    assert stats["qlen_classes"] >= 4
    assert any(Fraction(float(r.float32[w])) != r.exact(w) for r in got for w in list(r.by_qlen)[:1])
    assert max(b - a + 1 for _, a, b in regions) >= 300000
    # the corner region: rule 1 against rule 4, rule 5's strict bounds
    corner = got[-1]
    assert regions[-1] == ("chr3", S, E) and len(corner.depth) == E - S + 1
    assert corner.depth[E - S] >= 2 and corner.depth[0] >= 1       # "right" and "last" reach tx_end; "out" is not fetched
    lefts, rights = {l for l, _ in corner.jxns}, {r for _, r in corner.jxns}
    assert S + 1 in lefts and S not in lefts and E - 1 not in lefts
    assert E - 1 in rights and E not in rights and S + 1 not in rights
    assert (S + 330, S + 336) in corner.jxns and (S + 420, S + 424) in corner.jxns and (S + 433, S + 634) in corner.jxns
    # the shuffled file: the same integers, another float32 sum somewhere
    other, _ = want["shuffled"]
    assert all((a.depth == b.depth).all() and a.jxns == b.jxns for a, b in zip(got, other))
    assert any((a.float32 != b.float32).any() for a, b in zip(got, other))


_EXACT = {}


def _exact(region, w):
    key = tuple(sorted(region.by_qlen[w].items()))
    if key not in _EXACT:
        _EXACT[key] = region.exact(w)
    return _EXACT[key]


def check_against(got, want, regions, label):
    depth, wiggle, jxns, _ = got
    u53, u23 = Fraction(1, 2 ** 53), 2.0 ** -23
    for i, w in enumerate(want):
        assert depth[i].dtype == np.int32 and wiggle[i].dtype == np.float64
        assert len(depth[i]) == len(w.depth) == max(0, regions[i][2] - regions[i][1] + 1)
        assert (depth[i] == w.depth).all(), (label, i)
        assert jxns[i] == sorted((l, r, n) for (l, r), n in w.jxns.items()), (label, i)
        assert not wiggle[i][w.depth == 0].any()
        # within 2c * 2^-53 * wiggle of the exact rational value, c = distinct qlen at the base (c quotients and c - 1
        # additions of positive terms, each rounded once at unit round-off 2^-53): compared in rational arithmetic
        for b in w.by_qlen:
            x = Fraction(float(wiggle[i][b]))
            assert abs(x - _exact(w, b)) <= 2 * w.classes(b) * u53 * x, (label, i, b)
        # within (n + 1) * 2^-23 * wiggle of the reference's float32 running sum in file order, n = records at the base
        # (the comparison itself is made in double: its own rounding, 2^-53 relative, is far below the bound's 2^-23)
        f32 = w.float32.astype(np.float64)
        assert (np.abs(wiggle[i] - f32) <= (w.depth + 1) * u23 * wiggle[i]).all(), (label, i)


def test_densities_equal_the_checker(random_case):
    regions, paths, want = random_case
    names, starts, ends = [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions]
    first = None
    for budget in (0, 4 << 20):
        for which in ("sam", "bam", "shuffled"):
            f = sam_utils.Samfile(paths[which])
            for chunk in (1000, 4096, 0):
                got = capi.region_densities(f, names, starts, ends, chunk_records=chunk, accum_bytes=budget)
                label = (which, chunk, budget)
                st = got[3]
                assert st["chunks"] >= (len(f) + (chunk or 1 << 22) - 1) // (chunk or 1 << 22), label
                for key, value in want[which][1].items():
                    assert st[key] == value, (label, key)
                if budget:
                    assert st["groups"] >= 3, label
                else:
                    assert st["groups"] == 1, label
                if first is None or which == "shuffled" and chunk == 1000:
                    check_against(got, want[which][0], regions, label)   # every bound, once per record order and budget
                if first is None:
                    first = got
                    continue
                for i in range(len(regions)):                            # bit-identical to the first run
                    assert (got[0][i] == first[0][i]).all(), (label, i)
                    assert got[1][i].tobytes() == first[1][i].tobytes(), (label, i)
                    assert got[2][i] == first[2][i], (label, i)
            f.close()


def test_raw_names_and_empty(random_case):
    regions, paths, _ = random_case
    f = sam_utils.Samfile(paths["sam"])
    depth, wiggle, jxns, st = capi.region_densities(f, [], [], [])
    assert depth == [] and wiggle == [] and jxns == [] and st["fetched"] == 0 and st["groups"] == 0
    # the C ABI matches names exactly: "chr2" is not the file's "2"
    depth, wiggle, jxns, _ = capi.region_densities(f, ["chr2", "2"], [1, 1], [300000, 300000])
    assert len(depth[0]) == len(depth[1]) == 300000
    assert not depth[0].any() and not wiggle[0].any() and jxns[0] == []
    assert depth[1].any() and wiggle[1].any()


@pytest.mark.parametrize("sample", sorted(REAL))
def test_real_files(sample):
    path = os.path.join(GOLDEN, "bam-data", sample + ".sorted.bam")
    sam = ref.bam_to_sam(path)
    (want,), stats = ref.regions(sam, [EVENT_REGION])
    records, *counts = REAL[sample]
    # the checker against the table of the issue
    assert stats["fetched"] == want.fetched == records == len(sam.splitlines()) - sam.count("@SQ")
    assert stats["skipped_multi_n"] == stats["skipped_no_cigar"] == 0 and want.qlen_seen == {48}
    assert [want.jxns[s] for s in SITES] == counts and len(want.jxns) == 3
    f = sam_utils.Samfile(path)
    got = capi.region_densities(f, [EVENT_REGION[0]], [EVENT_REGION[1]], [EVENT_REGION[2]])
    check_against(got, [want], [EVENT_REGION], sample)
    assert got[3]["fetched"] == records == len(f) and got[3]["qlen_classes"] == 1
    assert got[3]["skipped_multi_n"] == got[3]["skipped_no_cigar"] == 0
    assert got[2][0] == [(l, r, n) for (l, r), n in zip(SITES, counts)]
