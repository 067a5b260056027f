"""GPU: the device decoder of `.miso` sample text (kernels_text.hip through capi.text_shape and
capi.SamplesBatch.from_text) on text planted where its bytes lie, not what its values are: the families of
tests/_text_layout_cases.py (every begin phase and span byte, tile edges, rows longer than a tile, 63 - 129 tiles, events
shorter than a span, rows cut off at an event's end, empty lines, text before the first event) against the plain-Python
reference tests/_text_layout_ref.py.  Every comparison is for equality: statuses, and the pool bit for bit."""
import os

import numpy as np
import pytest

import _text_layout_cases as cases
import _text_layout_ref as ref
from miso_amd import capi, miso_db, miso_pack, samples_utils
from test_gpu_miso_text import summarize, write_two_sample_trees

pytestmark = pytest.mark.gpu

FAMILIES = cases.families()
NAMES = sorted(FAMILIES)
_RUNS = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def text_of(fam):
    return fam.prefix + b"".join(fam.bodies), np.asarray(cases.offsets_of(fam), dtype=np.int64)


def run(fam, chunk_bytes=0):
    """(statuses, pool bits per event, text_stats) of the family as one batch, decoded once per chunk size."""
    key = (fam.name, chunk_bytes)
    if key not in _RUNS:
        text, offs = text_of(fam)
        b = capi.SamplesBatch.from_text(text, offs, fam.K, fam.S, chunk_bytes=chunk_bytes)
        _RUNS[key] = ([int(s) for s in b.status], [bits(b.samples(i)).tobytes() for i in range(len(fam.bodies))],
                      b.text_stats)
    return _RUNS[key]


def chunk_sizes(fam):
    return [0, 1, ref.TILE, len(fam.bodies[0])]


@pytest.mark.parametrize("name", NAMES)
def test_shape_status_and_pool_bits_are_the_reference_s(name):
    fam = FAMILIES[name]
    text, offs = text_of(fam)
    K, rows = capi.text_shape(text, offs)
    want_shape = [ref.shape(b) for b in fam.bodies]
    assert list(zip(K.tolist(), rows.tolist())) == want_shape
    status, pool, stats = run(fam)
    want = cases.reference(fam)
    for e, (st, samples) in enumerate(want):
        if st == 0 or st & (st - 1) == 0:
            assert status[e] == st, (e, status[e], st, fam.bodies[e][-40:])
        else:
            assert status[e] & st == st, (e, status[e], st)
        if st == 0:
            assert pool[e] == bits(samples).tobytes(), (e, np.nonzero(np.frombuffer(pool[e], np.uint64)
                                                                      != bits(samples).ravel())[0][:5])
    assert stats["decoded"] == sum(1 for st, _ in want if st == 0)
    assert stats["decoded"] + stats["not_decoded"] == len(fam.bodies)
    assert stats["text_bytes"] == len(text) - len(fam.prefix) and stats["chunks"] == 1


@pytest.mark.parametrize("name", NAMES)
def test_the_chunk_size_changes_neither_a_status_nor_a_bit_of_the_pool(name):
    fam = FAMILIES[name]
    offs = cases.offsets_of(fam)
    status0, pool0, _ = run(fam)
    sizes = chunk_sizes(fam)
    if min(len(b) for b in fam.bodies) > 1:                               # every event a chunk of its own, at phase 0
        assert ref.layout(offs, 1)[1] == len(fam.bodies)
    else:                                                                 # (an empty event takes the next empty one along)
        assert ref.layout(offs, 1)[1] == len(fam.bodies) - 1
    if name == "ends":
        lay = ref.layout(offs, sizes[3])[0]
        assert lay[0].chunk != lay[1].chunk                               # the first pair: cut by a chunk boundary
    for c in sizes[1:]:
        status, pool, stats = run(fam, c)
        assert stats["chunks"] == ref.layout(offs, c)[1], c
        assert stats["decoded"] + stats["not_decoded"] == len(fam.bodies)
        assert status == status0, (c, [e for e in range(len(status)) if status[e] != status0[e]][:5])
        differ = [e for e in range(len(status)) if status0[e] == 0 and pool[e] != pool0[e]]
        assert differ == [], (c, differ[:5])


@pytest.mark.parametrize("name", ["tiny", "ends"])
def test_a_rejected_or_empty_event_costs_its_neighbours_nothing(name):
    fam = FAMILIES[name]
    want = cases.reference(fam)
    checked = 0
    for c in chunk_sizes(fam):
        status, pool, _ = run(fam, c)
        for e, (st, _) in enumerate(want):
            if st == 0:
                continue
            assert status[e] != 0, (c, e)
            for nb in (e - 1, e + 1):
                if 0 <= nb < len(want) and want[nb][0] == 0:
                    assert status[nb] == 0 and pool[nb] == bits(want[nb][1]).tobytes(), (c, e, nb)
                    checked += 1
    assert checked >= 4 * sum(1 for st, _ in want if st)      # (as many valid neighbours as rejected events, at least)


# ---- a tree: the same values with empty lines and without the last LF, through summarize with either decoder ----
def respace(rows, how):
    """The body of the rows `rows` (each without its LF) laid out anew; the values stay."""
    if how == "leading":
        return "\n" + "".join(r + "\n" for r in rows)
    if how == "interior":
        return "".join(r + ("\n\n" if i in (0, 7, 8) else "\n\n\n" if i == len(rows) // 2 else "\n") for i, r in enumerate(rows))
    if how == "trailing":
        return "".join(r + "\n" for r in rows) + "\n\n\n"
    if how == "no_final_lf":
        return "\n".join(rows)
    if how == "blank_and_no_final_lf":
        return "\n\n" + "\n".join(r + ("\n" if i % 5 == 0 else "") for i, r in enumerate(rows[:-1])) + "\n\n" + rows[-1]
    assert how == "every_row"
    return "".join(r + "\n\n" for r in rows)


REWRITTEN = {"ev003": "leading", "ev010": "interior", "ev025": "trailing", "ev040": "no_final_lf",
             "ev055": "blank_and_no_final_lf", "ev070": "every_row"}


def test_a_tree_with_empty_lines_gives_the_table_of_the_untouched_tree_with_either_decoder(tmp_path, monkeypatch):
    ctl = write_two_sample_trees(tmp_path)[0]
    untouched = {}
    for decoder in ("host", "device"):
        untouched[decoder], st = summarize(ctl, str(tmp_path / "sum0" / decoder), decoder, monkeypatch)
    assert untouched["host"] == untouched["device"] and len(untouched["host"].splitlines()) == 73
    bodies = {}
    for name, how in REWRITTEN.items():
        path = os.path.join(ctl, "chr%d" % (int(name[2:]) % 3), name + ".miso")
        lines = open(path).read().splitlines()
        header, rows = lines[:2], lines[2:]
        assert len(rows) > 20 and all(rows)
        body = respace(rows, how)
        assert [ln for ln in body.split("\n") if ln] == rows and body != "".join(r + "\n" for r in rows)
        with open(path, "w", newline="") as f:
            f.write("".join(h + "\n" for h in header) + body)
        bodies[name] = body.encode()
    for form in ("unpacked", "packed"):
        if form == "packed":
            assert miso_pack.main(["--pack", ctl]) == 0
            assert sorted(os.listdir(ctl)) == ["chr0.miso_db", "chr1.miso_db", "chr2.miso_db"]
            # a `.miso_db` row keeps the body's bytes as the file had them: the same text reaches the decoders
            for name in REWRITTEN:
                with miso_db.MISODatabase(os.path.join(ctl, "chr%d.miso_db" % (int(name[2:]) % 3)), text_factory=bytes) as db:
                    stored = [rows for ev, rows, _ in db if ev.decode() == name]
                assert stored == [bodies[name]], name
        for decoder in ("host", "device"):
            table, st = summarize(ctl, str(tmp_path / "sum" / form / decoder), decoder, monkeypatch)
            assert st["decoder"] == decoder
            if decoder == "device":               # it cannot pass by leaving the events to the host parser
                assert st["fallback_events"] == [] and st["device_events"] == 72
            assert table == untouched[decoder], (form, decoder)
