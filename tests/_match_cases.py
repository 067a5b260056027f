"""Seeded reads and genes that no simulator makes, for read x isoform matching (solve.c:8-108, 141-218;
gff.c:1041-1084): the inputs of tests/golden/match/adversarial.npz, tests/test_match_cases.py and
tests/test_gpu_match_adversarial.py.  Pure Python and numpy; coordinates are 1-based and inclusive.

The gene "tangled" has an alternative 5' site, an alternative 3' site, a one-base exon, a retained intron, a double
skip and two abutting exons, so its exons overlap, nest and touch.  Around it: the same gene far down a chromosome
("shifted") and wide genes of 33, 64, 65 and 256 isoforms that carry the tangled isoforms on both sides of every
32-bit word boundary of the device's masks.

`model_match` / `model_match_paired` restate the rule in plain Python.  The generator uses them to plant reads (a
planted pair must fit its isoform before its fragment length means anything); the expected values the tests compare
with come from the real reference, through the golden file.
"""
import hashlib
import math
import random

import numpy as np

READ_LEN = 36                      # the length every CIGAR below is written for; read length 30 truncates them
OVERHANGS = (1, 4, 8)
READ_LENS = (36, 30)
MEAN_VARS = ((250.0, 900.0), (120.0, 400.0), (60.0, 100.0))
NUM_DEVS = 4.0
N_RANDOM = 8000
SEED = 20240229
SHIFT = 240000000                  # chromosome-sized, still int32

TANGLED_EXONS = [(101, 200), (101, 230), (301, 400), (281, 400), (501, 501), (601, 700), (201, 300), (101, 400)]
TANGLED_ISOFORMS = [[0, 2, 5], [1, 2, 5], [0, 3, 5], [0, 2, 4, 5], [7, 5], [0, 5], [0, 6, 2, 5]]
WIDE_K = (33, 64, 65, 256)
WIDE_K_PAIRED = (33, 64)           # above 64 isoforms only single-end REASSIGN events are packed

# the wide genes' filler: 24 exons right of 700, one filler isoform per pair of them (276 pairs, 249 needed)
N_EXTRA = 24
EXTRA_EXONS = [(1001 + 150 * j, 1100 + 150 * j) for j in range(N_EXTRA)]
EXTRA_PAIRS = [(a, b) for a in range(N_EXTRA) for b in range(a + 1, N_EXTRA)]
PLANTED_WHOLE = (0, 5, 23)         # extra exons that get a `36M` read: every filler isoform holding one is matched


def tangled():
    return list(TANGLED_EXONS), [list(i) for i in TANGLED_ISOFORMS]


def shifted():
    return [(s + SHIFT, e + SHIFT) for s, e in TANGLED_EXONS], [list(i) for i in TANGLED_ISOFORMS]


def tangled_slots(K):
    """Where the seven tangled isoforms sit in the wide gene of K isoforms: 0, 31, 32, 63, 64, K - 2, K - 1 (those
    below K, once each, in that order); what is left of the seven where these are fewer goes to 1, 2, ..."""
    slots = []
    for s in (0, 31, 32, 63, 64, K - 2, K - 1):
        if s < K and s not in slots:
            slots.append(s)
    nxt = 1
    while len(slots) < len(TANGLED_ISOFORMS):
        if nxt not in slots:
            slots.append(nxt)
        nxt += 1
    return slots[:len(TANGLED_ISOFORMS)]


def wide(K):
    """(exons, isoforms): the tangled isoforms at tangled_slots(K), distinct filler isoforms of two extra exons each
    everywhere else (the first K - 7 of EXTRA_PAIRS, in order)."""
    exons = list(TANGLED_EXONS) + list(EXTRA_EXONS)
    slots = tangled_slots(K)
    isoforms, f = [], 0
    for k in range(K):
        if k in slots:
            isoforms.append(list(TANGLED_ISOFORMS[slots.index(k)]))
        else:
            a, b = EXTRA_PAIRS[f]
            isoforms.append([len(TANGLED_EXONS) + a, len(TANGLED_EXONS) + b])
            f += 1
    return exons, isoforms


def gene(name):
    if name == "tangled":
        return tangled()
    if name == "shifted":
        return shifted()
    assert name.startswith("wide")
    return wide(int(name[4:]))


def gene_names(paired):
    return ["tangled", "shifted"] + ["wide%d" % K for K in (WIDE_K_PAIRED if paired else WIDE_K)]


# ---- the rule, in plain Python ----
def parse_cigar(cigar, read_len):
    """(blocks, covered): M = X S H D blocks positive, N blocks negative, I dropped; a block that would pass read_len
    (> 0) is cut to what is left, down to zero (solve.c:220-306)."""
    s = cigar.decode() if isinstance(cigar, bytes) else cigar
    blocks, covered, num = [], 0, ""
    for ch in s:
        if ch.isdigit():
            num += ch
            continue
        l, num = int(num), ""
        if ch in "M=XSHD":
            if read_len > 0 and covered + l > read_len:
                l = read_len - covered
            covered += l
            blocks.append(l)
        elif ch == "N":
            blocks.append(-l)
        else:
            assert ch == "I", "unsupported CIGAR " + s
    return blocks, covered


def iso_exons(exons, isoform):
    return [exons[e] for e in isoform]


def fits(ex, pos, blocks):
    """solve.c:65-94 for one isoform (its exons in order) and one usable read"""
    i = 0
    while i < len(ex) and (pos < ex[i][0] or ex[i][1] < pos):
        i += 1
    if i >= len(ex):
        return False
    p = pos
    for o in blocks:
        if o > 0:
            if p + o - 1 > ex[i][1]:
                return False
            p += o
        else:
            if p != ex[i][1] + 1:
                return False
            p -= o
            i += 1
            if i >= len(ex) or p != ex[i][0]:
                return False
    return True


def usable(blocks, covered, read_len, overhang):
    return covered >= read_len and len(blocks) > 0 and blocks[0] >= overhang and blocks[-1] >= overhang


def model_match(exons, isoforms, pos, cigars, read_len, overhang):
    out = np.zeros((len(pos), len(isoforms)), np.uint8)
    tabs = [iso_exons(exons, i) for i in isoforms]
    for r, (p, c) in enumerate(zip(pos, cigars)):
        blocks, covered = parse_cigar(c, read_len)
        if usable(blocks, covered, read_len, overhang):
            for k, ex in enumerate(tabs):
                out[r, k] = fits(ex, int(p), blocks)
    return out


def genomic_to_iso(ex, p):
    """gff.c:1041-1084: 1-based place of genomic p in the isoform, -1 outside its exons"""
    before = 0
    for s, e in ex:
        if e < p:
            before += e - s + 1
            continue
        return before + p - s + 1 if s <= p else -1
    return -1


def iso_to_genomic(ex, q):
    for s, e in ex:
        if q <= e - s + 1:
            return s + q - 1
        q -= e - s + 1
    raise ValueError("past the isoform's end")


def cigar_for(ex, start, length):
    """the CIGAR of `length` bases read along the isoform from genomic `start`"""
    i = 0
    while ex[i][1] < start:
        i += 1
    out, left, p = "", length, start
    while ex[i][1] < p + left - 1:
        m = ex[i][1] - p + 1
        out += "%dM%dN" % (m, ex[i + 1][0] - ex[i][1] - 1)
        left -= m
        p = ex[i + 1][0]
        i += 1
    return out + "%dM" % left


def normal_fragment(mean, var, read_len, num_devs=NUM_DEVS):
    """(start, il) of the fragment-length window (simulator.c:198-219): lengths start .. start + il - 1"""
    sd = math.sqrt(var)
    start, end = int(mean - sd * num_devs), int(mean + sd * num_devs)
    start = max(start, read_len)
    end = max(end, start)
    return start, end - start + 1


def model_match_paired(exons, isoforms, pos, cigars, read_len, overhang, mean, var):
    """fragment lengths [pairs, K], -1 = none (solve.c:187-205)"""
    m = model_match(exons, isoforms, pos, cigars, read_len, overhang)
    start, il = normal_fragment(mean, var, read_len)
    tabs = [iso_exons(exons, i) for i in isoforms]
    fl = np.full((len(pos) // 2, len(isoforms)), -1, np.int32)
    for r in range(len(pos) // 2):
        for k, ex in enumerate(tabs):
            if m[2 * r, k] and m[2 * r + 1, k]:
                frag = genomic_to_iso(ex, int(pos[2 * r + 1])) - genomic_to_iso(ex, int(pos[2 * r])) + read_len
                if start <= frag < start + il:
                    fl[r, k] = frag
    return fl


# ---- named corner reads ----
def corner_reads():
    """(name, pos, cigar, row at read length 36, row at read length 30): the compatibility with the seven tangled
    isoforms at overhang 1, as the rule named in the comment gives it.  At overhang 4 and 8 the row stays where the
    first and the last block (after the cut to the read length) are that long, and is all zero otherwise."""
    return [
        ("first_base", 101, "36M", "1111111", "1111111"),            # starts on the first base of exons 0, 1 and 7
        ("last_exon_first_base", 601, "36M", "1111111", "1111111"),  # ... of the last exon of every isoform
        ("starts_on_last_base", 200, "1M100N35M", "1001000", "1001000"),   # exend < pos is false on an exon's last base
        ("one_base_exon_start", 501, "1M99N35M", "0001000", "0001000"),    # start == end == pos
        ("before_first_exon", 100, "36M", "0000000", "0000000"),     # pos < exstart of every exon: no start exon
        ("ends_on_last_base", 165, "36M", "1111111", "1111111"),     # p + o - 1 == exend is inside
        ("overruns_by_one", 166, "36M", "0100100", "1111111"),       # p + o - 1 == exend + 1: only exons (101,230), (101,400) hold it; not 0 + 6, a read never walks into an abutting exon without an N; cut to 30 it ends on 195
        ("ends_on_gene_end", 665, "36M", "1111111", "1111111"),
        ("overruns_gene_end", 666, "36M", "0000000", "1111111"),     # 701 is in no exon; cut to 30 it ends on 695
        ("junction_exact", 181, "20M100N16M", "1001000", "1001000"),       # 200 -> 301: isoforms with exon 0 then exon 2
        ("junction_plus_one", 181, "20M101N16M", "0000000", "0000000"),    # lands on 302: p != exstart
        ("junction_minus_one", 181, "20M99N16M", "0000000", "0000000"),    # lands on 300
        ("alt3_exact", 181, "20M80N16M", "0010000", "0010000"),      # 200 -> 281, the alternative 3' site
        ("alt3_plus_one", 181, "20M81N16M", "0000000", "0000000"),
        ("alt3_minus_one", 181, "20M79N16M", "0000000", "0000000"),
        ("alt5_exact", 211, "20M70N16M", "0100000", "0100000"),      # 230 -> 301, the alternative 5' site; the retained intron's exon ends at 400
        ("alt5_plus_one", 212, "20M69N16M", "0000000", "0000000"),   # leaves from 231: overruns exon (101,230) by one
        ("leaves_one_early", 180, "20M101N16M", "0000000", "0000000"),     # lands on 301 but leaves from 199: p != exend + 1
        ("double_skip", 181, "20M400N16M", "0000010", "0000010"),    # 200 -> 601 over exons 2 and 4: only the isoform whose next exon is 5
        ("skip_one_base_exon", 381, "20M200N16M", "1110101", "1110101"),   # 400 -> 601: every isoform with an exon ending at 400 but the one with the one-base exon between
        ("through_one_base_exon", 381, "20M100N1M99N15M", "0001000", "0001000"),   # 400 -> 501 -> 601
        ("two_in_one_base_exon", 381, "20M100N2M98N14M", "0000000", "0000000"),    # 502 > exend 501
        ("abutting_zero_intron", 195, "6M0N30M", "0000001", "0000001"),    # 200 -> 201 with 0N: exons 0 and 6 abut
        ("abutting_plain", 195, "36M", "0100100", "0100100"),        # the same bases without the N: exons (101,230) and (101,400) only; cut to 30 it ends on 224
        ("retained_intron", 240, "36M", "0000101", "0000101"),       # 240..275: the retained intron and exon 6
        ("retained_intron_to_exon", 270, "36M", "0000100", "0000101"),     # 270..305 leaves exon 6 (ends 300); cut to 30 it ends on 299, still inside
        ("alt3_region", 285, "36M", "0010100", "0010100"),           # 285..320: exon 3 and the retained intron; exon 6 holds 285 but ends at 300
        ("ends_in_N", 165, "36M100N", "0000000", "0000000"),         # last block negative: below any overhang
        ("starts_in_N", 65, "100N36M", "0000000", "0000000"),        # first block negative
        ("too_short", 120, "30M", "0000000", "1111111"),             # covered 30 < 36; exactly the read length at 30
        ("too_long_cut", 162, "40M", "1111111", "1111111"),          # cut to 36: ends on 197, uncut it would overrun 200
        ("soft_clip_front", 170, "5S31M", "0100100", "1111111"),     # a clip counts as bases: 170..205 overruns 200
        ("soft_clip_back", 170, "31M5S", "0100100", "0000000"),      # cut to 30 the clip is a zero-length last block: below overhang 1
        ("insertion", 165, "20M5I16M", "1111111", "1111111"),        # I takes no genome: 165..200
        ("deletion", 165, "20M3D13M", "1111111", "1111111"),         # D counts as bases: 165..200
        ("split_match", 165, "3M33M", "1111111", "1111111"),         # two blocks, first of 3: gone at overhang 4
        ("eq_and_x", 165, "20=5X11M", "1111111", "1111111"),
        ("zero_last_block", 195, "6M100N30M10S", "0000000", "0000000"),    # the clip is cut to zero length: last block 0 < overhang
        ("cut_last_block", 195, "6M100N40M", "1001000", "1001000"),  # 40M cut to 30 (24): no zero block, 200 -> 301
        ("empty", 120, "", "0000000", "0000000"),                    # covers nothing: shorter than any positive read length
        ("pos_zero", 0, "36M", "0000000", "0000000"),
        ("pos_negative", -5, "36M", "0000000", "0000000"),
    ]


def corner_expected(row36, row30, cigar, read_len, overhang):
    blocks, _ = parse_cigar(cigar, read_len)
    row = row36 if read_len == 36 else row30
    if not blocks or blocks[0] < overhang or blocks[-1] < overhang:
        row = "0000000"
    return np.array([int(c) for c in row], np.uint8)


def filler_reads():
    """Reads on the wide genes' extra exons (they match nothing in "tangled"): a junction read for every third filler
    pair -- it fits the one isoform made of exactly that pair -- and a `36M` read on the exons of PLANTED_WHOLE, which
    fits every filler isoform holding that exon.  The other filler isoforms are matched by nothing."""
    out = []
    for f, (a, b) in enumerate(EXTRA_PAIRS):
        if f % 3 == 0:
            out.append((EXTRA_EXONS[a][1] - 19, "20M%dN16M" % (EXTRA_EXONS[b][0] - EXTRA_EXONS[a][1] - 1)))
    for a in PLANTED_WHOLE:
        out.append((EXTRA_EXONS[a][0] + 7, "36M"))
    return out


ODD_CIGARS = ["30M", "40M", "5S31M", "31M5S", "20M5I16M", "20M3D13M", "3M33M", "20=5X11M", "36M100N", "100N36M",
              "6M100N30M10S", "6M100N40M", "6M0N30M", "20M100N1M99N15M"]


def random_reads(n=N_RANDOM, seed=SEED):
    """About 70 % within [-40, +5] of a random exon boundary, the rest anywhere in [90, 700]; `36M`, a junction from
    the read's position to the end of some exon and on to a later exon's start (one time in three one base off), or
    one of the odd shapes."""
    rng = random.Random(seed)
    bounds = sorted({c for e in TANGLED_EXONS for c in e})
    out = []
    for _ in range(n):
        pos = rng.choice(bounds) + rng.randint(-40, 5) if rng.random() < 0.7 else rng.randint(90, 700)
        u = rng.random()
        cigar = "36M"
        if u < 0.5:
            ends = sorted({e for _, e in TANGLED_EXONS if pos <= e < pos + READ_LEN - 1})
            if ends:
                end = rng.choice(ends)
                starts = sorted({s for s, _ in TANGLED_EXONS if s > end})
                if starts:
                    land = rng.choice(starts) + rng.choice((0, 0, 0, 0, 1, -1))
                    a = end - pos + 1
                    if land - end - 1 >= 0:
                        cigar = "%dM%dN%dM" % (a, land - end - 1, READ_LEN - a)
        elif u < 0.65:
            cigar = rng.choice(ODD_CIGARS)
        out.append((pos, cigar))
    return out


def single_reads(n_random=N_RANDOM):
    """(pos int32[], cigars [bytes], {corner name: index}): corners, filler reads, random reads; an even number"""
    reads, where = [], {}
    for name, pos, cigar, _, _ in corner_reads():
        where[name] = len(reads)
        reads.append((pos, cigar))
    reads += filler_reads()
    reads += random_reads(n_random)
    if len(reads) % 2:
        reads.append((150, "36M"))
    return (np.array([p for p, _ in reads], np.int32), [c.encode() for _, c in reads], where)


def window_isoform():
    """the tangled isoform the window pairs are planted on: the longest (first of them)"""
    lens = [sum(e - s + 1 for s, e in iso_exons(TANGLED_EXONS, i)) for i in TANGLED_ISOFORMS]
    return int(np.argmax(lens))


def paired_corners(mean, var, read_len):
    """[(name, (pos1, cigar1), (pos2, cigar2))] for one fragment window.  window_*: mate 1 at place 10 of
    window_isoform(), mate 2 where the fragment on that isoform is start - 1, start, start + il - 1, start + il;
    both mates fit that isoform at every overhang of the grid (asserted here with the model)."""
    start, il = normal_fragment(mean, var, read_len)
    k = window_isoform()
    ex = iso_exons(TANGLED_EXONS, TANGLED_ISOFORMS[k])
    q1 = 10
    m1 = (iso_to_genomic(ex, q1), cigar_for(ex, iso_to_genomic(ex, q1), read_len))
    out = []
    for name, frag in (("window_below", start - 1), ("window_first", start), ("window_last", start + il - 1),
                       ("window_above", start + il)):
        g2 = iso_to_genomic(ex, q1 + frag - read_len)
        m2 = (g2, cigar_for(ex, g2, read_len))
        for pos, cigar in (m1, m2):
            blocks, covered = parse_cigar(cigar, read_len)
            assert usable(blocks, covered, read_len, max(OVERHANGS)) and fits(ex, pos, blocks), (name, pos, cigar)
        out.append((name, m1, m2))
    far = iso_to_genomic(ex, q1 + start + il // 2 - read_len)
    rl = "%dM" % read_len
    out += [
        ("swapped", (far, cigar_for(ex, far, read_len)), m1),        # mate 2 left of mate 1: a negative span, no fragment
        ("same_place", m1, m1),                                      # fragment == read length: inside only where start was clamped to it
        ("one_unusable", m1, (m1[0] + 40, "%dM" % (read_len - 1))),  # mate 2 shorter than the read length
        ("disjoint_sets", (181, "20M100N%dM" % (read_len - 20)), (211, "20M70N%dM" % (read_len - 20))),   # {0, 3} and {1}
        ("split_lengths", (160, rl), (301, rl)),                     # at 36: 77 on exons 0 + 2, 97 by the alternative 3' site, 107 by the 5' one, 177 through the retained intron
    ]
    return out


def paired_reads(mean, var, read_len, n_random=N_RANDOM):
    """(pos, cigars, {corner name: pair index}): the planted pairs, then single_reads() two by two"""
    reads, where = [], {}
    for name, a, b in paired_corners(mean, var, read_len):
        where[name] = len(reads) // 2
        reads += [a, b]
    pos, cig, _ = single_reads(n_random)
    return (np.concatenate([np.array([p for p, _ in reads], np.int32), pos]), [c.encode() for _, c in reads] + cig,
            where)


def se_key(name, overhang, read_len):
    return "se_%s_ov%d_rl%d" % (name, overhang, read_len)


def pe_key(name, overhang, read_len, mean, var):
    return "pe_%s_ov%d_rl%d_m%d_v%d" % (name, overhang, read_len, int(mean), int(var))


def inputs_digest():
    """SHA-256 over every generated input: genes, single-end reads, paired reads of every window"""
    h = hashlib.sha256()
    for name in gene_names(False):
        ex, iso = gene(name)
        h.update(repr((name, ex, iso)).encode())
    pos, cig, where = single_reads()
    h.update(pos.tobytes() + b"\0".join(cig) + repr(sorted(where.items())).encode())
    for mean, var in MEAN_VARS:
        for rl in READ_LENS:
            pos, cig, where = paired_reads(mean, var, rl)
            h.update(pos.tobytes() + b"\0".join(cig) + repr(sorted(where.items())).encode())
    return h.hexdigest()


class Golden:
    """tests/golden/match/adversarial.npz (tests/golden/make_golden.py match_adversarial): what the real reference
    returned for the cases above.  "shifted" is "tangled"; a wide gene is "tangled" in its tangled_slots() plus the
    stored filler entries -- both equalities were asserted on the reference's output when the file was made, and
    tests/test_match_cases.py asserts them again wherever the reference library is built."""

    def __init__(self, path):
        z = np.load(path, allow_pickle=False)
        self.z = {k: z[k] for k in z.files}
        self.digest = str(self.z["digest"])
        self.seven = len(TANGLED_ISOFORMS)

    def _widen(self, name, key, base, fill_len=False):
        if name in ("tangled", "shifted"):
            return base
        K = int(name[4:])
        out = np.full((base.shape[0], K), -1 if fill_len else 0, base.dtype)
        out[:, tangled_slots(K)] = base
        idx = self.z[key + "_filler"]
        out[idx[:, 0], idx[:, 1]] = self.z[key + "_filler_len"] if fill_len else 1
        return out

    def se(self, name, overhang, read_len):
        """match uint8 [N, K]"""
        base = np.unpackbits(self.z[se_key("tangled", overhang, read_len)], axis=1)[:, :self.seven]
        return self._widen(name, se_key(name, overhang, read_len), base)

    def pe(self, name, overhang, read_len, mean, var):
        """(match uint8 [pairs, K], fragment lengths int32 [pairs, K], -1 = none)"""
        t = pe_key("tangled", overhang, read_len, mean, var)
        m = np.unpackbits(self.z[t + "_match"], axis=1)[:, :self.seven]
        fl = self.z[t + "_fraglen"].astype(np.int32)
        key = pe_key(name, overhang, read_len, mean, var)
        return self._widen(name, key, m), self._widen(name, key, fl, fill_len=True)
