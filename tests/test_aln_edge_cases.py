"""The case builders of tests/_aln_edge_cases.py run through the checkers alone (tests/_density_ref.py,
tests/_insert_len_ref.py): every case reaches what it is built for.  tests/test_gpu_aln_edges.py feeds the same cases to
the device passes; a case that drifts away from its branch fails here, without a GPU."""
import _aln_edge_cases as cases
import _density_ref as dref
import _insert_len_ref as iref


def test_overrun_case_overruns_both_lists():
    sam, regions = cases.overrun_case()
    assert len(regions) == 64 and len({r[1] for r in regions}) == 64
    seqid, s, e = regions[0]
    refs, recs = dref.parse_sam(sam)
    assert len(recs) == 9000
    for r in recs:                                   # both junctions of every record strictly inside region 0
        aligned = r.positions()
        sites = [(x + 1, y + 1) for x, y in zip(aligned, aligned[1:]) if y > x + 1]
        assert len(sites) == 2 and all(s < site < e for pair in sites for site in pair)
        assert s <= aligned[0] and aligned[-1] <= e
    want = dref.region(refs, recs, seqid, s, e)
    entries, distinct = sum(want.jxns.values()), len(want.jxns)
    print("junction entries %d, distinct pairs %d" % (entries, distinct))
    assert entries == 2 * len(recs) and want.d_junctions == len(recs)
    assert 64 * entries > cases.FIRST_JXN_CAP, "grow the case: the junction list of one group no longer overruns"
    assert 64 * distinct > cases.WRAPPER_JXN_CAP, "grow the case: the wrapper's first arrays hold every junction"
    # two groups of 32 stay below the first capacity, and the budget that cuts them exists
    assert 32 * entries <= cases.FIRST_JXN_CAP
    assert want.qlen_seen == {50}
    budget = cases.group_bytes(regions[32:], 1)
    assert cases.group_bytes(regions[:32], 1) <= budget < cases.group_bytes(regions[:33], 1)


def test_words_case_ends_chunks_on_words():
    sam, (region,) = cases.words_case()
    cigars = cases.cigars_of(sam)
    ops = [cases.n_ops(c) for c in cigars]
    assert 2900 <= len(cigars) <= 3100
    assert sum(ops) / len(ops) > 4 and max(ops) >= 9
    plain = [c for c in cigars if c == "50M"]
    assert 5 <= len(plain) <= 30 and all(6 <= n <= 9 for n, c in zip(ops, cigars) if c != "50M")
    assert all(c.count("N") <= 1 for c in cigars)
    # the word bound max(4 C, longest) is met before C records at every chunk size of the GPU test but 1
    for chunk in (2, 7, 64, 1000):
        bound = max(cases.WORDS_PER_RECORD * chunk, max(ops))
        assert any(sum(ops[i:i + chunk]) > bound for i in range(0, len(ops), chunk)), chunk
    assert max(ops) > cases.WORDS_PER_RECORD * 1               # chunk size 1: W = the longest CIGAR
    (want,), stats = dref.regions(sam, [region])
    assert region[2] - region[1] == 20000
    assert stats["fetched"] > 2500 and stats["with_indel"] > 2500 and stats["skipped_multi_n"] == 0
    assert len(want.jxns) > 1000 and want.depth[0] > 0 and want.depth[-1] > 0
    assert stats["qlen_classes"] >= 5


def test_shapes_case_is_accepted_by_the_checker():
    sam, regions = cases.shapes_case()
    refs, recs = dref.parse_sam(sam)
    assert [("".join("%d%s" % (n, op) for op, n in r.cigar)) for r in recs[:-1]] == cases.SHAPES
    want, stats = dref.regions(sam, regions)
    whole = want[0]
    assert stats["fetched"] == len(cases.SHAPES) + 1 == whole.fetched
    at = lambda shape: cases.SHAPES_AT + 100 * cases.SHAPES.index(shape) - regions[0][1]
    for shape in ("0M50M", "50M0M", "10M5P40M", "10M0N40M", "50M5D"):       # 50 bases from pos, no junction
        assert whole.depth[at(shape):at(shape) + 50].all() and not whole.depth[at(shape) + 50]
    assert whole.depth[at("5H45M") + 44] and not whole.depth[at("5H45M") + 45]
    for shape in ("5D50M", "5N50M"):                                          # a leading gap shifts the bases
        assert not whole.depth[at(shape):at(shape) + 5].any() and whole.depth[at(shape) + 5:at(shape) + 55].all()
    for shape in ("3I", "10S"):                                               # fetched, no aligned position
        assert not whole.depth[at(shape) - 5:at(shape) + 15].any()
    p = cases.SHAPES_AT + 100 * cases.SHAPES.index("20M5D0M5D30M")
    assert whole.jxns[(p + 20, p + 31)] == 1                                   # one gap of ten, not two of five
    p = cases.SHAPES_AT + 100 * cases.SHAPES.index("1M1D1M1D1M1D1M")
    assert [whole.jxns[(p + 1 + 2 * k, p + 3 + 2 * k)] for k in range(3)] == [1, 1, 1]
    assert len(whole.jxns) == 4                                                # 0N, leading and trailing gaps: none
    assert whole.depth[at("25M2I23M") + 47] and not whole.depth[at("25M2I23M") + 48]
    assert whole.depth[cases.SHAPES_AT + 100 * len(cases.SHAPES) - regions[0][1] + 49] == 1   # the record flagged 4
    assert recs[-1].end == recs[-1].pos + 1
    assert whole.qlen_seen == {50, 45, 4}
    # the region that begins inside the gap loses the junction (leftss < tx_start) and keeps the bases after it
    assert (cases.SHAPES_AT + 1020, cases.SHAPES_AT + 1031) not in want[1].jxns and want[1].depth[8]
    assert not want[1].depth[:8].any()
    # the region that ends inside the steps keeps the junctions strictly inside it
    q = cases.SHAPES_AT + 100 * cases.SHAPES.index("20M5D0M5D30M")
    assert sorted(want[2].jxns) == [(q + 20, q + 31), (p + 1, p + 3)]          # rightss p + 5 == tx_end: not counted
    assert want[2].depth[-1] == 0 and want[2].depth[-2] == 1 and regions[2][2] == p + 5


def test_qlen_case_meets_the_bitmap_top():
    for extra in (None, "outside"):
        (want,), stats = dref.regions(*cases.qlen_case(extra))
        assert want.qlen_seen == {50, 65535} and stats["qlen_classes"] == 2 and stats["fetched"] == 3
        assert len(want.depth) == 70000 and want.depth.max() == 2 and 65535 >> 5 == 2047 and 65535 & 31 == 31
    (want,), stats = dref.regions(*cases.qlen_case("inside"))
    assert want.qlen_seen == {50, 65535, 65536} and stats["fetched"] == 4


def test_coords_case_meets_the_int32_end():
    sam, regions = cases.coords_case()
    refs, recs = dref.parse_sam(sam)
    assert max(r.end for r in recs) == cases.BIG == 2 ** 31 - 1 and min(r.pos for r in recs) == 0
    want, stats = dref.regions(sam, regions)
    assert stats["fetched"] == 4
    assert [len(w.depth) for w in want] == [151, 2 ** 31 + 1000 - (cases.BIG - 100) + 1, 1, 1, 251]
    for w in want[:2]:
        assert w.jxns == {(cases.BIG - 35, cases.BIG - 24): 1} and w.fetched == 2
        assert w.depth[99] == 1 and w.depth[100] == 0          # the last base of the reference, the first beyond it
    assert all(site >= 2 ** 31 - 64 for site in list(want[0].jxns)[0])
    assert not want[2].depth.any() and not want[3].depth.any() and want[2].fetched == want[3].fetched == 0
    assert want[4].jxns == {(30, 41): 1} and want[4].depth[50] == 1 and not want[4].depth[:50].any()


def test_tagging_case_has_every_kind():
    ivs, sam = cases.tagging_case()
    intervals = [iref.Interval(s, a, b, ".") for s, a, b in ivs]
    recs = iref.parse_sam(sam)
    assert 240 <= len(ivs) <= 270 and len(recs) >= 8000
    tags = [iref.tags(r, intervals) for r in recs]
    kinds = {"none": sum(1 for t in tags if not t), "single": sum(1 for t in tags if len(t) == 1),
             "multi": sum(1 for t in tags if len(t) > 1)}
    print(kinds)
    assert min(kinds.values()) >= 100, kinds
    codes = iref.record_codes(recs, intervals)
    assert sum(1 for c in codes if c & iref.TAG_NONE == iref.TAG_MULTI) == kinds["multi"]
    # the kinds the search has to get right
    giant = ivs.index(("chrA", 1, cases.REF_LEN))
    assert sum(1 for t in tags if t == [giant]) >= 100                              # held only by the giant interval
    assert any(len(t) == 2 and ivs[t[0]][:2] == ivs[t[1]][:2] and ivs[t[0]][2] != ivs[t[1]][2] for t in tags)
    assert any(len(t) == 2 and ivs[t[0]] == ivs[t[1]] for t in tags)                # exactly two, exact duplicates
    assert any(len(t) >= 3 for t in tags)
    # the interval list: duplicates, start > end, start == end, a reference the file lacks, same-start groups whose
    # longest member is not the first listed
    assert len(set(ivs)) < len(ivs) and any(a > b for _, a, b in ivs) and sum(1 for _, a, b in ivs if a == b) >= 2
    assert ("chrQ", 1, cases.REF_LEN) in ivs and "chrQ" not in sam
    groups = {}
    for s, a, b in ivs:
        if s == "chrC" and a >= 50000 and a < 90000:
            groups.setdefault(a, []).append(b)
    assert len(groups) == 12 and all(3 <= len(g) <= 5 and g[0] != max(g) for g in groups.values())
    assert not any(s == "chrB" and b - a > 200 for s, a, b in ivs)                  # chrB: short intervals only
    held_one = [t[0] for t in tags if len(t) == 1]
    assert any(ivs[k][1] == ivs[k][2] for k in held_one)                            # a one-base interval holds a record
    assert not any(ivs[k][1] > ivs[k][2] or ivs[k][0] == "chrQ" for t in tags for k in t)
    # near an edge: most records begin or end within 60 bases of an interval's first or last base
    by_ref = {}
    for s, a, b in ivs:
        by_ref.setdefault(s, set()).update((a - 1, b))
    near = sum(1 for r in recs if any(abs(r.pos - x) <= 60 or abs(r.end - x) <= 60 for x in by_ref.get(r.rname, ())))
    assert near >= 0.6 * len(recs)
    flags = {r.flag for r in recs}
    assert flags == set(cases.TAG_FLAGS)
    assert sum(1 for r in recs if len(r.cigar) == 3) >= 500 and min(r.end - r.pos for r in recs) == 1


def test_pairs_case_fills_wavefronts_with_different_intervals():
    ivs, sam = cases.pairs_case()
    intervals = iref.gff_intervals(cases.gff_text(ivs))
    recs = iref.parse_sam(sam)
    assert len(ivs) == 128 and all(a[2] < b[1] for a, b in zip(ivs, ivs[1:]))
    left = [iref.tags(r, intervals) for r in recs[0::2]]
    cycle = cases.PAIR_INTERVALS * cases.PAIRS_EACH
    assert all(len(t) == 1 for t in left[:cycle])
    order = [t[0] for t in left[:cycle]]
    assert all(len(set(order[i:i + 64])) == 64 for i in range(cycle - 63))
    assert {t[0] for t in left[cycle:cycle + cases.ONE_INTERVAL_PAIRS]} == {5}
    by_interval, counts = iref.insert_len(recs, intervals)
    n = cases.REFUSALS_EACH
    assert counts == {"kept": cycle + cases.ONE_INTERVAL_PAIRS, "skipped": 2 * n, "unpaired": 0, "same_strand": n,
                      "nonpositive": n, "tagged": len(recs)}
    assert sorted(by_interval) == list(range(128))
    assert len(by_interval[5]) == cases.PAIRS_EACH + cases.ONE_INTERVAL_PAIRS
    pairs = len(recs) // 2
    assert pairs % 100 % 64 and pairs % 64 and pairs % 1000 % 64                  # part-filled last wavefronts
