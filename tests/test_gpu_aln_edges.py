"""GPU: the density pass (csrc/kernels_density.hip) and the insert-length passes (csrc/kernels_insert.hip) on the cases
of tests/_aln_edge_cases.py, against tests/_density_ref.py and tests/_insert_len_ref.py: the junction list that overruns
and the group that runs twice, chunks that end on the CIGAR-word bound, the CIGAR shapes the rules mention in passing,
the top of the qlen bitmap, the int32 end and regions beyond it, the three refusals; the record search against brute
force, and the pair pass on wavefronts of 64 different intervals.  tests/test_aln_edge_cases.py shows, without a GPU,
that each case reaches its branch.  Every comparison is for equality but the two wiggle bounds of
test_gpu_density.check_against.  A refusal arrives as capi.InternalError, the exception capi.check raises for
MISO_EINVAL; where "nothing written" is part of it, the C entry point is called on arrays filled with a sentinel."""
import ctypes as C

import numpy as np
import pytest

import _aln_edge_cases as cases
import _density_ref as dref
import _insert_len_ref as iref
from _bam import sam_to_bam
from miso_amd import capi, sam_utils
from test_gpu_density import check_against
from test_gpu_insert_len import _check_end_to_end

pytestmark = pytest.mark.gpu

STAT_KEYS = ("fetched", "skipped_multi_n", "skipped_no_cigar", "with_indel", "qlen_classes")


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible")


def _open(directory, name, sam, as_bam=False):
    path = str(directory / (name + (".bam" if as_bam else ".sam")))
    if as_bam:
        sam_to_bam(sam, path, block=60000)
    else:
        with open(path, "w") as out:
            out.write(sam)
    return sam_utils.Samfile(path)


def _densities(f, regions, **kw):
    return capi.region_densities(f, [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], **kw)


def _same(got, first, label):
    """Bit-identical depth, wiggle and junctions, and the same counts."""
    assert len(got[0]) == len(first[0])
    for i in range(len(first[0])):
        assert got[0][i].tobytes() == first[0][i].tobytes(), (label, i)
        assert got[1][i].tobytes() == first[1][i].tobytes(), (label, i)
        assert got[2][i] == first[2][i], (label, i)
    assert {k: got[3][k] for k in STAT_KEYS} == {k: first[3][k] for k in STAT_KEYS}, label


def _raw_densities(f, regions, out_cap, jxn_cap=16):
    """miso_region_densities itself, every output array filled with a sentinel first: (return code, arrays, n_jxn)."""
    n, names, st, en = capi._intervals([r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions])
    depth, wiggle = np.full(max(out_cap, 1), -7, np.int32), np.full(max(out_cap, 1), -7.0, np.float64)
    jr, jl = np.full(jxn_cap, -7, np.int32), np.full(jxn_cap, -7, np.int64)
    jrt, jc = np.full(jxn_cap, -7, np.int64), np.full(jxn_cap, -7, np.int64)
    found, stats = C.c_int64(-7), capi.DensityStats()
    L = capi.lib()
    L.miso_region_densities.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
                                        + [C.c_int64, C.POINTER(C.c_int64), C.POINTER(capi.DensityStats)])
    p = capi._p
    rc = L.miso_region_densities(f._h, 0, n, names, p(st), p(en), 0, 0, p(depth), p(wiggle), out_cap, p(jr), p(jl),
                                 p(jrt), p(jc), jxn_cap, C.byref(found), C.byref(stats))
    return rc, (depth, wiggle, jr, jl, jrt, jc), found.value


def _untouched(arrays, found):
    return found == -7 and all((a == -7).all() for a in arrays)


# ---- 1. the junction list overruns; the wrapper calls twice ----
@pytest.fixture(scope="module")
def overrun(tmp_path_factory):
    sam, regions = cases.overrun_case()
    f = _open(tmp_path_factory.mktemp("overrun"), "overrun", sam)
    refs, recs = dref.parse_sam(sam)
    want0 = dref.region(refs, recs, *regions[0])                  # region k: the same junctions, depth behind k zeros
    first = _densities(f, regions)                                # the default budget: one group
    yield f, regions, want0, first
    f.close()


def test_junction_list_overruns_and_the_group_runs_again(overrun):
    f, regions, want0, got = overrun
    depth, wiggle, jxns, st = got
    print("overrun, default budget: groups %d, junction_retries %d, chunks %d"
          % (st["groups"], st["junction_retries"], st["chunks"]))
    assert st["groups"] == 1
    assert st["junction_retries"] >= 1, "grow the case: the junction list of one group no longer overruns"
    assert sum(len(j) for j in jxns) > cases.WRAPPER_JXN_CAP, "grow the case: the wrapper's first arrays held it all"
    assert st["fetched"] == 9000 and st["with_indel"] == 9000 and st["qlen_classes"] == 1
    check_against(([depth[0]], [wiggle[0]], [jxns[0]], st), [want0], regions[:1], "overrun")
    want_jxns = sorted((l, r, n) for (l, r), n in want0.jxns.items())
    for k in range(len(regions)):
        # region k is region 0 behind k zeros: the same integers, and the same doubles, as wiggle is a function of the
        # per-class depths alone; so the two wiggle bounds checked on region 0 hold on every region
        assert len(depth[k]) == len(depth[0]) + 2 * k
        assert not depth[k][:k].any() and not depth[k][len(depth[k]) - k:].any(), k
        assert not wiggle[k][:k].any() and not wiggle[k][len(wiggle[k]) - k:].any(), k
        assert depth[k][k:k + len(depth[0])].tobytes() == depth[0].tobytes(), k     # a second pass that did not zero
        assert wiggle[k][k:k + len(depth[0])].tobytes() == wiggle[0].tobytes(), k   # the rows would double these
        assert jxns[k] == want_jxns, k                                               # the keys under their own region


@pytest.mark.parametrize("two_groups, chunk", [(False, 1000), (True, 0), (True, 1000)])
def test_junction_list_overrun_by_group_and_chunk(overrun, two_groups, chunk):
    f, regions, want0, first = overrun
    budget = cases.group_bytes(regions[32:], 1) if two_groups else 0
    got = _densities(f, regions, chunk_records=chunk, accum_bytes=budget)
    st = got[3]
    print("overrun, budget %d, chunk %d: groups %d, junction_retries %d, chunks %d"
          % (budget, chunk, st["groups"], st["junction_retries"], st["chunks"]))
    if two_groups:
        assert st["groups"] == 2 and st["junction_retries"] == 0
    else:
        assert st["groups"] == 1 and st["junction_retries"] >= 1, "grow the case"
    _same(got, first, (two_groups, chunk))


# ---- 2. chunks that end on CIGAR words ----
@pytest.fixture(scope="module")
def words(tmp_path_factory):
    sam, regions = cases.words_case()
    f = _open(tmp_path_factory.mktemp("words"), "words", sam)
    want, stats = dref.regions(sam, regions)
    first = _densities(f, regions, chunk_records=1)               # W = the longest CIGAR > 4 slot_n
    yield f, regions, want, stats, first
    f.close()


@pytest.mark.parametrize("chunk", [1, 2, 7, 64, 1000, 0])
def test_chunks_end_on_cigar_words(words, chunk):
    f, regions, want, stats, first = words
    got = first if chunk == 1 else _densities(f, regions, chunk_records=chunk)
    st = got[3]
    print("words, chunk %d: chunks %d of %d records" % (chunk, st["chunks"], len(f)))
    assert {k: st[k] for k in STAT_KEYS} == stats
    assert (got[0][0] == want[0].depth).all()
    assert got[2][0] == sorted((l, r, n) for (l, r), n in want[0].jxns.items())
    if chunk == 1:
        check_against(got, want, regions, "words")
        assert st["chunks"] == len(f)
    else:
        _same(got, first, chunk)
    if chunk in (2, 7, 64, 1000):
        assert st["chunks"] > -(-len(f) // chunk), "no chunk ended on the word bound"


# ---- 3. CIGAR shapes ----
@pytest.mark.parametrize("as_bam", [False, True])
def test_cigar_shapes(tmp_path, as_bam):
    sam, regions = cases.shapes_case()
    want, stats = dref.regions(sam, regions)
    f = _open(tmp_path, "shapes", sam, as_bam)                    # the reader accepts every shape, as SAM and as BAM
    assert len(f) == len(cases.SHAPES) + 1
    got = _densities(f, regions)
    check_against(got, want, regions, ("shapes", as_bam))
    assert {k: got[3][k] for k in STAT_KEYS} == stats
    _same(_densities(f, regions, chunk_records=1), got, ("shapes, chunk 1", as_bam))
    f.close()


# ---- 4. qlen limits ----
def test_qlen_limits(tmp_path):
    sam, regions = cases.qlen_case()
    want, stats = dref.regions(sam, regions)
    f = _open(tmp_path, "top", sam)
    first = _densities(f, regions)
    assert first[3]["qlen_classes"] == 2 and {k: first[3][k] for k in STAT_KEYS} == stats
    check_against(first, want, regions, "qlen 65535")
    f.close()
    # qlen 65536 in a fetched record: refused, and named
    f = _open(tmp_path, "inside", cases.qlen_case("inside")[0])
    with pytest.raises(capi.InternalError) as err:
        _densities(f, regions)
    assert "65536" in str(err.value) and "65535" in str(err.value)
    f.close()
    # the same record where no region fetches it: as if it were not there
    f = _open(tmp_path, "outside", cases.qlen_case("outside")[0])
    _same(_densities(f, regions), first, "qlen 65536 outside")
    f.close()


# ---- 5. coordinates ----
def test_int32_end_and_regions_beyond(tmp_path):
    sam, regions = cases.coords_case()
    want, stats = dref.regions(sam, regions)
    f = _open(tmp_path, "coords", sam)
    got = _densities(f, regions)
    check_against(got, want, regions, "coords")
    assert {k: got[3][k] for k in STAT_KEYS} == stats
    assert got[2][0] == got[2][1] == [(cases.BIG - 35, cases.BIG - 24, 1)] and got[2][4] == [(30, 41, 1)]
    _same(_densities(f, regions, chunk_records=1, accum_bytes=1), got, "coords, one region per group")
    f.close()


@pytest.mark.parametrize("region", [("chrBig", cases.COORD_LIMIT + 1, cases.COORD_LIMIT + 1),
                                    ("chrBig", -cases.COORD_LIMIT - 1, -cases.COORD_LIMIT - 1),
                                    ("chrBig", -cases.COORD_LIMIT, -cases.COORD_LIMIT - 1)])
def test_coordinates_beyond_the_limit_are_refused(tmp_path, region):
    """start = 2^40 + 1; start and end = -2^40 - 1; end = -2^40 - 1 alone (an empty region otherwise)."""
    sam, regions = cases.coords_case()
    f = _open(tmp_path, "coords", sam)
    regions = [regions[4], region]
    with pytest.raises(capi.InternalError, match="region 1: coordinate out of range"):
        _densities(f, regions)
    rc, arrays, found = _raw_densities(f, regions, out_cap=1000)
    assert rc == capi.MISO_EINVAL and _untouched(arrays, found)   # nothing written
    f.close()


def test_small_output_arrays_are_refused(tmp_path):
    sam, regions = cases.coords_case()
    f = _open(tmp_path, "coords", sam)
    regions = [regions[4], regions[0]]                            # 251 + 151 entries
    rc, arrays, found = _raw_densities(f, regions, out_cap=401)
    assert rc == capi.MISO_EINVAL and _untouched(arrays, found)
    message = capi.lib().miso_last_error().decode()
    assert "401" in message and "402" in message
    rc, arrays, found = _raw_densities(f, regions, out_cap=402)   # exactly enough
    assert rc == 0 and found == 2
    want, _ = dref.regions(sam, regions)
    assert (arrays[0][:251] == want[0].depth).all() and (arrays[0][251:402] == want[1].depth).all()
    assert list(zip(arrays[2][:2], arrays[3][:2], arrays[4][:2], arrays[5][:2])) == \
        [(0, 30, 41, 1), (1, cases.BIG - 35, cases.BIG - 24, 1)]
    f.close()


# ---- 6. the record search against brute force ----
@pytest.fixture(scope="module")
def tagging():
    ivs, sam = cases.tagging_case()
    recs = iref.parse_sam(sam)
    intervals = [iref.Interval(s, a, b, ".") for s, a, b in ivs]
    want = {flt: iref.record_codes(recs, intervals, filter_reads=flt) for flt in (True, False)}
    return ivs, sam, want


@pytest.mark.parametrize("as_bam", [False, True])
def test_record_search_equals_brute_force(tagging, tmp_path, as_bam):
    ivs, sam, want = tagging
    f = _open(tmp_path, "tags", sam, as_bam)
    assert len(f) == len(want[True])
    seqids, starts, ends = [v[0] for v in ivs], [v[1] for v in ivs], [v[2] for v in ivs]
    for flt in (True, False):
        expect = np.array(want[flt], dtype=np.int64)
        for chunk in (0, 100, 777):
            got = capi.insert_tag_records(f, seqids, starts, ends, filter_reads=flt, chunk_records=chunk)
            wrong = np.flatnonzero(got.astype(np.int64) != expect)
            assert not len(wrong), (flt, chunk, len(wrong), int(wrong[0]), int(got[wrong[0]]), int(expect[wrong[0]]))
    f.close()


# ---- 7. the pair pass, interval patterns ----
def test_pair_pass_on_64_different_intervals(tmp_path):
    ivs, sam = cases.pairs_case()
    gff = str(tmp_path / "pairs.gff")
    with open(gff, "w") as out:
        out.write(cases.gff_text(ivs))
    path = str(tmp_path / "pairs.sam")
    with open(path, "w") as out:
        out.write(sam)
    texts = set()
    for chunk in (0, 64, 100, 1000):
        counts, text = _check_end_to_end(path, sam, gff, chunk_records=chunk, tmp_path=tmp_path)
        assert counts["kept"] == cases.PAIR_INTERVALS * cases.PAIRS_EACH + cases.ONE_INTERVAL_PAIRS
        assert counts["same_strand"] == counts["nonpositive"] == cases.REFUSALS_EACH
        assert counts["skipped"] == 2 * cases.REFUSALS_EACH
        texts.add(text)
    assert len(texts) == 1
