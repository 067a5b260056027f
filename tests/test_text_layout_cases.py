"""CPU: the planted sample text of tests/_text_layout_cases.py is what it claims to be (each byte where the case says,
by the layout of tests/_text_layout_ref.py), the reference agrees with Python's float() and with itself, and the host
parser (samples_utils._parse_rows, parse_miso_file) follows the same contract as the device decoder: empty lines are
ignored, the last LF may be missing."""
import numpy as np
import pytest

import _text_layout_cases as cases
import _text_layout_ref as ref
from miso_amd import samples_utils

FAMILIES = cases.families()
NAMES = sorted(FAMILIES)


def where(fam, chunk_bytes=0):
    return ref.layout(cases.offsets_of(fam), chunk_bytes)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_module_is_under_three_megabytes_and_every_family_has_one_sample_count():
    total = sum(len(f.prefix) + sum(len(b) for b in f.bodies) for f in FAMILIES.values())
    assert total < 3_000_000
    for f in FAMILIES.values():
        assert len(f.bodies) == len(f.K) and all(1 <= k <= 256 for k in f.K)
        assert max(len(b) for b in f.bodies) <= 2_000_000


@pytest.mark.parametrize("name", ["phases", "prefix"])
def test_phases_put_a_line_start_on_every_span_byte_for_every_begin_phase(name):
    fam = FAMILIES[name]
    lay = where(fam)
    assert len(fam.bodies) == 256 and all(w.chunk == 0 and w.tiles == 1 for w in lay)
    pairs, minus, lf_in_previous_thread = set(), set(), 0
    for body, w in zip(fam.bodies, lay):
        starts = ref.line_starts(body)
        assert len(starts) == 3 and starts[0] == 0
        assert w.at(0)[2] == w.begin % ref.SPAN
        pairs.add((w.begin % ref.SPAN, w.at(starts[1])[2]))
        for s in starts[1:]:
            tile, thread, byte, _ = w.at(s)
            if byte == 0:
                assert w.at(s - 1)[:3] == (tile, thread - 1, 15) and body[s - 1:s] == b"\n"
                lf_in_previous_thread += 1
        at = body.find(b"-inf")
        while at >= 0:
            minus.add(w.at(at)[3])
            at = body.find(b"-inf", at + 1)
    assert pairs == {(p, j) for p in range(16) for j in range(16)}
    assert lf_in_previous_thread >= 16
    assert minus == set(range(8))                        # (byte 7: the look-ahead behind `-` loads the next word)


def test_prefix_is_two_lines_that_belong_to_no_event_and_leaves_the_layout_of_phases():
    fam = FAMILIES["prefix"]
    assert len(fam.prefix) == 37 and fam.prefix.count(b"\n") == 2 and fam.prefix.endswith(b"\n")
    assert cases.offsets_of(fam)[0] == 37
    assert fam.bodies == FAMILIES["phases"].bodies and where(fam) == where(FAMILIES["phases"])
    assert ref.decode(fam.prefix, 2, 2)[0] == 0          # (taken for rows, the two lines would decode)


def test_tile_edges_have_their_byte_where_they_say():
    fam = FAMILIES["tile_edges"]
    lay = where(fam)
    assert [w.tiles for w in lay] == [4] * 6
    names = [m[0] for m in fam.marks["bytes"]]
    assert sorted(set(names)) == ["lf_last_start_first", "minus_inf_1_3", "minus_inf_2_2", "minus_inf_3_1", "start_last",
                                  "tab_last"]
    for name, e, i, byte, coords in fam.marks["bytes"]:
        body, w = fam.bodies[e], lay[e]
        assert body[i:i + 1] == byte and w.at(i)[:3] == coords, (name, w.at(i), coords)
    by = {}
    for name, e, i, byte, coords in fam.marks["bytes"]:
        by.setdefault(name, []).append((e, i, coords))
    (e, lf, c_lf), (_, start, c_start) = by["lf_last_start_first"]
    assert c_lf[1:] == (255, 15) and c_start == (c_lf[0] + 1, 0, 0) and start in ref.line_starts(fam.bodies[e])
    (e, lf, c_lf), (_, start, c_start) = by["start_last"]
    assert c_start[1:] == (255, 15) and c_lf[1:] == (255, 14) and start in ref.line_starts(fam.bodies[e])
    (e, i, c), = by["tab_last"]
    assert c[1:] == (255, 15)
    for name, last_byte in (("minus_inf_1_3", 15), ("minus_inf_2_2", 14), ("minus_inf_3_1", 13)):
        (e, i, c), = by[name]
        assert fam.bodies[e][i - 1:i + 5] == b"\t-inf\n" and c[1:] == (255, last_byte)
        assert lay[e].at(i + 3)[0] == c[0] + 1           # the `f` is the next tile's


def test_long_rows_have_a_tile_and_a_last_tile_without_a_line_start():
    fam = FAMILIES["long_rows"]
    lay = where(fam)
    assert fam.K == [2, 256, 256, 256]
    for e in (1, 3):
        body, w = fam.bodies[e], lay[e]
        assert all(len(ln) > ref.TILE for ln in ref.lines_of(body))
        assert all(len(f) == 24 for ln in ref.lines_of(body) for f in ln.split(b"\t")[0].split(b","))
        with_start = {w.at(s)[0] for s in ref.line_starts(body)}
        assert w.tiles - 1 not in with_start and any(t not in with_start for t in range(w.tiles - 1))
    assert lay[1].begin % ref.SPAN != 0
    assert all(len(f) == 1 for ln in ref.lines_of(fam.bodies[2]) for f in ln.split(b"\t")[0].split(b","))


def test_tile_counts_are_exactly_63_64_65_128_and_129():
    fam = FAMILIES["tile_counts"]
    lay = where(fam)
    assert [w.tiles for w in lay] == [63, 64, 65, 128, 129]
    in_last = [(w.begin - w.aligned + w.length) - ref.TILE * (w.tiles - 1) for w in lay]
    assert in_last[1] == ref.TILE and in_last[2] == 1
    w = lay[2]
    assert w.at(ref.line_starts(fam.bodies[2])[-1])[0] == w.tiles - 2        # the last tile holds the final LF alone
    for body in fam.bodies:
        rows = ref.lines_of(body)
        assert len(rows) == fam.S and len({r.split(b"\t")[0] for r in rows}) == fam.S


def test_tiny_has_several_events_in_one_span_and_empty_events_between_neighbours():
    fam = FAMILIES["tiny"]
    lay = where(fam)
    assert len(fam.bodies) == 200 and fam.S == 1
    assert all(3 <= len(b) <= 15 for i, b in enumerate(fam.bodies) if i not in fam.marks["empty"])
    assert {bytes(fam.bodies[i]) for i in fam.marks["empty"]} == {b"", b"\n", b"\n\n", b"\n" * 17}
    whole = {}
    for i, w in enumerate(lay):
        if w.length and w.begin // ref.SPAN == (w.begin + w.length - 1) // ref.SPAN:
            whole.setdefault(w.begin // ref.SPAN, []).append(i)
    assert max(len(v) for v in whole.values()) >= 3
    for i in fam.marks["no_lf"]:
        assert not fam.bodies[i].endswith(b"\n") and fam.bodies[i + 1][:1].isdigit()
    for (st, _), body, i in zip(cases.reference(fam), fam.bodies, range(200)):
        assert st == (ref.ECOUNT if i in fam.marks["empty"] else 0), i
        assert ref.shape(body) == ((0, 0) if i in fam.marks["empty"] else (1, 1))
    # single empty events and a run of three stand between valid neighbours; the text ends in an empty event
    empty = fam.marks["empty"]
    assert {28, 29, 30} <= set(empty) and 27 not in empty and 31 not in empty and 199 in empty and 198 not in empty
    assert sum(1 for i in empty if i - 1 not in empty and i + 1 not in empty and i < 199) >= 5


@pytest.mark.parametrize("name", ["ends"] + ["ends_last_%d" % i for i in range(7)])
def test_ends_are_cut_where_they_say_and_the_next_event_begins_with_the_byte_named(name):
    fam = FAMILIES[name]
    lay = where(fam)
    got = cases.reference(fam)
    cut_events = set()
    for e, first, status in fam.marks["pairs"]:
        cut_events.add(e)
        assert got[e][0] == status and ref.shape(fam.bodies[e]) == (2, 3)
        assert not fam.bodies[e].endswith(b"\n")
        if first is None:
            assert e == len(fam.bodies) - 1
        else:
            assert fam.bodies[e + 1].startswith(first)
    for e in range(len(fam.bodies)):
        if e not in cut_events:
            assert got[e][0] == 0 and ref.shape(fam.bodies[e]) == (fam.K[e], 3)
    if name == "ends":
        assert len(fam.marks["pairs"]) == 8 * len(cases.ENDS)
        for n in range(len(cases.ENDS)):
            ends_at = {(lay[e].begin + lay[e].length) % ref.WORD for e, _, _ in fam.marks["pairs"][n::len(cases.ENDS)]}
            assert ends_at == set(range(8)), n


def test_blank_lines_change_nothing_and_their_runs_cross_a_span_and_a_tile_boundary():
    fam = FAMILIES["blank_lines"]
    lay = where(fam)
    got = cases.reference(fam)
    none = bits(got[0][1]).tobytes()
    for e, body in enumerate(fam.bodies):
        st, s = ref.decode(cases.strip_blank(body), fam.K[e], fam.S)
        assert st == 0 and got[e][0] == 0 and bits(s).tobytes() == bits(got[e][1]).tobytes()
        assert ref.shape(body) == (20, 12)
        if e < 7:
            assert bits(got[e][1]).tobytes() == none
    assert fam.bodies[0].count(b"\n") == 12 and all(b.count(b"\n") > 12 for b in fam.bodies[1:6])
    assert fam.bodies[5].count(b"\n\n") == 12 and fam.bodies[1].startswith(b"\n") and fam.bodies[4].endswith(b"\n\n\n")
    assert fam.bodies[6].startswith(b"\n") and not fam.bodies[6].endswith(b"\n") and fam.bodies[6].count(b"\n\n") == 11
    runs = {name: (e, i, n) for name, e, i, n in fam.marks["runs"]}
    e, i, n = runs["span_run"]
    assert fam.bodies[e][i - 1:i + n] == b"\n" * (n + 1) and b"\n" not in (fam.bodies[e][i - 2:i - 1], fam.bodies[e][i + n:i + n + 1])
    assert lay[e].at(i)[2] == 14 and lay[e].at(i + n)[1:3] == (lay[e].at(i)[1] + 2, 2)
    e, i, n = runs["tile_run"]
    assert fam.bodies[e][i - 1:i + n] == b"\n" * (n + 1) and fam.bodies[e][i + n:i + n + 1] != b"\n"
    assert lay[e].at(i)[:3] == (0, 255, 6) and lay[e].at(i + n)[:3] == (1, 0, 10)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_agrees_with_float_and_with_what_the_cases_claim(name):
    fam = FAMILIES[name]
    got = cases.reference(fam)
    for e, (body, K) in enumerate(zip(fam.bodies, fam.K)):
        k, rows = ref.shape(body)
        assert k in (0, K)
        for ln in ref.lines_of(body):
            for f in ln.split(b"\t")[0].split(b","):
                v = ref.psi_value(f)
                if v is not None:
                    assert bits(v) == bits(float(f)), f
        st, s = got[e]
        assert (s is None) == (st != 0)
        if st == 0:
            assert s.shape == (fam.S, K) and rows == fam.S
    if not name.startswith(("tiny", "ends")):
        assert [st for st, _ in got] == [0] * len(fam.bodies)


def test_the_reference_status_bits_as_tabulated():
    assert ref.decode(b"0.5,0.5\t-1\n0.5,0.\n", 2, 2)[0] == ref.EPSI
    assert ref.decode(b"0.5,0.5\t-1\n0.5,0", 2, 2)[0] == ref.EROW
    assert ref.decode(b"0.5,0.5\t-1\n0.5\t1\n", 2, 2)[0] == ref.EROW
    assert ref.decode(b"0.5,0.5\t-1\n0.5,0.5\t-in", 2, 2)[0] == ref.ESCORE
    assert ref.decode(b"0.5,0.5\tNaN\n0.5,0.5\t1\r\n", 2, 2)[0] == ref.ESCORE
    assert ref.decode(b"0.5,0.5\t-1\n", 2, 2)[0] == ref.ECOUNT
    assert ref.decode(b"0.5,0.5\t-1\n1e-3,0.5\t-1\n0.5,0.5\t\n", 2, 2)[0] == ref.EPSI + ref.ECOUNT     # rows < S only
    assert ref.decode(b"0.1234567890123456\t1\n", 1, 1)[0] == ref.EPSI                  # 16 significant digits
    assert ref.decode(b"0." + b"0" * 22 + b"1\t1\n", 1, 1)[0] == ref.EPSI                 # 23 decimals
    st, s = ref.decode(b"\n\n-0.0000,00012.5\tinf\n\n0.0000000999999999999999,7\t-inf", 2, 2)
    assert st == 0 and bits(s).tolist() == bits([[-0.0, 12.5], [0.0000000999999999999999, 7.0]]).tolist()
    assert ref.shape(b"") == (0, 0) and ref.shape(b"\n\n") == (0, 0) and ref.shape(b"\n1,2,3\t0\n\n1\t0") == (3, 2)
    lay, chunks = ref.layout([37, 47, 47, 5047, 5050], 0)
    assert chunks == 1 and [tuple(w) for w in lay] == [(0, 0, 0, 1, 10), (0, 10, 0, 1, 0), (0, 10, 0, 2, 5000),
                                                       (0, 5010, 5008, 1, 3)]
    assert lay[2].at(4085) == (0, 255, 15, 7) and lay[2].at(4086) == (1, 0, 0, 0)
    lay, chunks = ref.layout([37, 47, 47, 5047, 5050], 10)
    assert chunks == 3 and [w.chunk for w in lay] == [0, 0, 1, 2] and [w.begin for w in lay] == [0, 10, 0, 0]


# ---- the host parser: the same contract ----
@pytest.mark.parametrize("name", NAMES)
def test_host_parser_gives_the_reference_bits_for_every_decodable_body(name):
    fam = FAMILIES[name]
    n = 0
    for body, (st, want) in zip(fam.bodies, cases.reference(fam)):
        if st == 0:
            have = samples_utils._parse_rows(body.decode())
            assert have.shape == want.shape and have.dtype == np.float64
            assert bits(have).tobytes() == bits(want).tobytes()
            n += 1
    assert n >= 1


def test_host_parser_ignores_empty_lines_and_takes_k_from_the_first_row():
    want = bits([[0.5, 0.5], [0.25, 0.75]]).tolist()
    for text in ("0.5,0.5\t-1.0\n\n0.25,0.75\t-2.0\n", "\n0.5,0.5\t-1.0\n0.25,0.75\t-2.0", "\n\n0.5,0.5\t-1.0\n\n\n0.25,0.75\tnan\n\n",
                 "0.5,0.5\t-1.0\n0.25,0.75\t-inf"):
        have = samples_utils._parse_rows(text)
        assert have.shape == (2, 2) and bits(have).tolist() == want, text
    for text in ("", "\n", "\n\n\n"):
        with pytest.raises(ValueError):
            samples_utils._parse_rows(text)


def test_parse_miso_file_reads_through_the_same_parser(tmp_path):
    fam = FAMILIES["blank_lines"]
    header = "#isoforms=['a','b']\tcounts=(0,1):5\nsampled_psi\tlog_score\n"
    for e in (0, 1, 3, 5, 6):
        path = tmp_path / ("ev%d.miso" % e)
        path.write_bytes(header.encode() + fam.bodies[e])
        name, samples, fields = samples_utils.parse_miso_file(str(path))
        assert name == "ev%d" % e and fields == {"isoforms": "['a','b']", "counts": "(0,1):5"}
        assert bits(samples).tobytes() == bits(cases.reference(fam)[e][1]).tobytes()
        assert bits(samples_utils.parse_miso_text(name, header, fam.bodies[e].decode())[1]).tobytes() == bits(samples).tobytes()
    empty = tmp_path / "none.miso"
    empty.write_text(header + "\n\n")
    with pytest.raises(ValueError):
        samples_utils.parse_miso_file(str(empty))
