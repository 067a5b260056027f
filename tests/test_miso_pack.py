"""CPU: miso_pack / miso_db (the packed `.miso_db` form of a MISO output tree, as misopy/miso_db.py and
misopy/miso_pack.py define it), how summarize / compare list packed, unpacked and mixed directories, and the host-only
shape call of the text decoder.  The databases are made here, by the packer or with plain sqlite3 calls."""
import ctypes
import os
import sqlite3
import stat

import numpy as np
import pytest

from miso_amd import capi, miso_db, miso_pack, samples_utils

HEADER2 = "sampled_psi\tlog_score\n"


def miso_text(name, K=2, rows=5, seed=0):
    rng = np.random.default_rng(seed)
    out = ["#isoforms=%s\texon_lens=('a',100),('b',50)\titers=100\tburn_in=10\tlag=2\tpercent_accept=90.00\tproposal_type=drift\t"
           "counts=(0,1):3,(1,1):9\tassigned_counts=0:5,1:7\tchrom=chr1\tstrand=+\tmRNA_starts=1,1\tmRNA_ends=9,9\n"
           % ",".join("'%s.%d'" % (name, k) for k in range(K)), HEADER2]
    for _ in range(rows):
        psi = rng.dirichlet(np.ones(K))
        out.append("%s\t%.2f\n" % (",".join("%.4f" % v for v in psi), -rng.random() * 100))
    return "".join(out)


def make_tree(root):
    """out/{chr1,10,X}/*.miso plus a non-MISO sub-directory; returns {chrom: {event: text}}."""
    tree = {}
    for ci, chrom in enumerate(("chr1", "10", "X")):
        d = root / chrom
        d.mkdir(parents=True)
        tree[chrom] = {}
        for e in range(3 + ci):
            name = "ev_%s_%d" % (chrom, e)
            text = miso_text(name, K=2 + e % 2, rows=4 + e, seed=10 * ci + e)
            (d / (name + ".miso")).write_text(text)
            tree[chrom][name] = text
    other = root / "logs"
    other.mkdir()
    (other / "run.log").write_text("not MISO output\n")
    (other / "notes.txt").write_text("x\n")
    return tree


def snapshot(root):
    out = {}
    for base, dirs, files in os.walk(str(root)):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, str(root))] = open(p, "rb").read()
        for d in dirs:
            out[os.path.relpath(os.path.join(base, d), str(root)) + "/"] = None
    return out


def test_pack_writes_one_database_per_chromosome_directory(tmp_path):
    root = tmp_path / "out"
    tree = make_tree(root)
    assert miso_pack.main(["--pack", str(root)]) == 0
    for chrom, events in tree.items():
        dbf = root / (chrom + ".miso_db")
        assert dbf.is_file() and not (root / chrom).exists()
        conn = sqlite3.connect(str(dbf))
        assert [r[0] for r in conn.execute("SELECT name FROM sqlite_master WHERE type='table'")] == ["table_" + chrom]
        cols = [(r[1], r[2].lower()) for r in conn.execute("PRAGMA table_info('table_%s')" % chrom)]
        assert cols == [("event_name", "text"), ("psi_vals_and_scores", "text"), ("header", "text")]
        got = {n: (h, r) for n, r, h in conn.execute("SELECT * FROM 'table_%s'" % chrom)}
        conn.close()
        assert sorted(got) == sorted(events)
        for name, text in events.items():
            header, rows = got[name]
            assert header + rows == text
            assert header == "".join(text.splitlines(keepends=True)[:2]) and header.endswith(HEADER2)
    assert sorted(os.listdir(str(root / "logs"))) == ["notes.txt", "run.log"]
    assert sorted(os.listdir(str(root))) == ["10.miso_db", "X.miso_db", "chr1.miso_db", "logs"]   # no temporary left


def test_pack_again_changes_nothing_and_an_existing_database_keeps_its_directory(tmp_path):
    root = tmp_path / "out"
    make_tree(root)
    assert miso_pack.main(["--pack", str(root)]) == 0
    # a directory whose .miso_db already exists: both stay as they are
    again = root / "chr1"
    again.mkdir()
    (again / "late.miso").write_text(miso_text("late"))
    before = snapshot(root)
    assert miso_pack.main(["--pack", str(root)]) == 0
    assert snapshot(root) == before
    assert (again / "late.miso").is_file()


def test_pack_of_several_directories_and_a_missing_one(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    make_tree(a); make_tree(b)
    assert miso_pack.main(["--pack", "%s,%s" % (a, b)]) == 0
    assert (a / "chr1.miso_db").is_file() and (b / "X.miso_db").is_file()
    with pytest.raises(SystemExit) as ex:
        miso_pack.main(["--pack", str(tmp_path / "nowhere")])
    assert ex.value.code == 1


def test_failed_pack_keeps_the_directory_and_leaves_no_database(tmp_path, monkeypatch):
    root = tmp_path / "out"
    tree = make_tree(root)
    victim = "ev_10_1"
    real = miso_db.load_miso_file_as_str

    def vanishing(path):                       # a file that disappears between listing and reading
        if os.path.basename(path) == victim + ".miso":
            raise FileNotFoundError(path)
        return real(path)

    monkeypatch.setattr(miso_db, "load_miso_file_as_str", vanishing)
    assert miso_pack.main(["--pack", str(root)]) != 0
    assert sorted(os.listdir(str(root / "10"))) == sorted(n + ".miso" for n in tree["10"])
    assert not [f for f in os.listdir(str(root)) if f.startswith("10.")]          # no database, no temporary
    # the other directories were still tried, and packed
    assert (root / "chr1.miso_db").is_file() and (root / "X.miso_db").is_file() and not (root / "chr1").exists()
    monkeypatch.undo()
    assert miso_pack.main(["--pack", str(root)]) == 0 and (root / "10.miso_db").is_file() and not (root / "10").exists()


def test_truncated_row_fails_the_check_against_the_directory(tmp_path, monkeypatch):
    """What the reference would lose: the conversion `succeeds` with short text, the directory goes."""
    root = tmp_path / "out"
    tree = make_tree(root)
    real = miso_db.load_miso_file_as_str

    def short(path):
        header, rows = real(path)
        return (header, rows[:-7]) if os.path.basename(path) == "ev_X_0.miso" else (header, rows)

    monkeypatch.setattr(miso_db, "load_miso_file_as_str", short)
    assert miso_pack.main(["--pack", str(root)]) == 1
    assert sorted(os.listdir(str(root / "X"))) == sorted(n + ".miso" for n in tree["X"])
    assert not (root / "X.miso_db").exists()


@pytest.mark.skipif(os.geteuid() == 0, reason="root writes into read-only directories")
def test_unwritable_target_keeps_the_directory(tmp_path):
    root = tmp_path / "out"
    tree = make_tree(root)
    os.chmod(str(root), stat.S_IRUSR | stat.S_IXUSR)
    try:
        assert miso_pack.main(["--pack", str(root)]) != 0
    finally:
        os.chmod(str(root), stat.S_IRWXU)
    for chrom, events in tree.items():
        assert sorted(os.listdir(str(root / chrom))) == sorted(n + ".miso" for n in events)
        assert not (root / (chrom + ".miso_db")).exists()


def write_foreign_db(path, table, rows):
    conn = sqlite3.connect(str(path))
    conn.execute("CREATE TABLE %s (event_name text, psi_vals_and_scores text, header text)" % table)
    for name, text in rows:
        header = "".join(text.splitlines(keepends=True)[:2])
        conn.execute("INSERT INTO %s VALUES (?, ?, ?)" % table, (name, text[len(header):], header))
    conn.commit()
    conn.close()


def test_database_written_elsewhere_is_read_back(tmp_path, capsys):
    texts = {n: miso_text(n, K=2 + i, rows=3 + i, seed=i) for i, n in enumerate(("zeta", "alpha", "mid@x:1-2"))}
    dbf = tmp_path / "17.miso_db"                      # a numeric (Ensembl) chromosome, rows in arbitrary order
    write_foreign_db(dbf, "table_17", list(texts.items()))
    db = miso_db.MISODatabase(str(dbf))
    assert db.table_name == "table_17"
    assert db.get_all_event_names() == list(texts)
    for name, text in texts.items():
        header = "".join(text.splitlines(keepends=True)[:2])
        assert db.get_event_data_as_string(name) == header + "\n" + text[len(header):] + "\n"
    assert db.get_event_data_as_string("nobody") is None
    assert [(n, h + r) for n, r, h in db] == list(texts.items())
    db.close()
    capsys.readouterr()
    assert miso_pack.main(["--view", str(dbf)]) == 0
    assert capsys.readouterr().out.splitlines() == ["Database contains 3 events"] + list(texts)
    # the same name twice: an error, not a silent pick
    dup = tmp_path / "chrD.miso_db"
    write_foreign_db(dup, "table_chrD", [("twin", texts["zeta"]), ("twin", texts["alpha"]), ("single", texts["alpha"])])
    db = miso_db.MISODatabase(str(dup))
    with pytest.raises(ValueError, match="More than one entry"):
        db.get_event_data_as_string("twin")
    assert db.get_event_data_as_string("single") is not None
    db.close()
    with pytest.raises(FileNotFoundError):
        miso_db.MISODatabase(str(tmp_path / "none.miso_db"))


def test_small_helpers(tmp_path):
    assert miso_db.is_miso_db_fname("a/chrX.miso_db") and not miso_db.is_miso_db_fname("a/chrX.miso")
    assert miso_db.strip_miso_ext("ev.miso") == "ev" and miso_db.strip_miso_ext("ev.txt") == "ev.txt"
    (tmp_path / "outer" / "inner").mkdir(parents=True)
    (tmp_path / "outer" / "inner" / "e.miso").write_text(miso_text("e"))
    assert miso_db.is_miso_unpacked_dir(str(tmp_path / "outer" / "inner"))
    assert not miso_db.is_miso_unpacked_dir(str(tmp_path / "outer"))            # files directly inside only
    assert not miso_db.is_miso_unpacked_dir(str(tmp_path / "outer" / "inner" / "e.miso"))


def listed(samples_dir):
    files, rows = samples_utils.list_events(str(samples_dir))
    return sorted([os.path.basename(f)[:-len(".miso")] for f in files] + [n for names in rows.values() for n in names])


def test_listing_gives_each_event_once(tmp_path, capsys):
    unpacked, packed, mixed = tmp_path / "u", tmp_path / "p", tmp_path / "m"
    tree = make_tree(unpacked); make_tree(packed); make_tree(mixed)
    every = sorted(n for events in tree.values() for n in events)
    assert miso_pack.main(["--pack", str(packed)]) == 0
    # mixed: one chromosome packed, and one of its events ALSO left as a file with other content
    assert miso_pack.pack_dir(str(mixed / "X")) is True
    (mixed / "X").mkdir()
    (mixed / "X" / "ev_X_1.miso").write_text(miso_text("ev_X_1", K=4, rows=6, seed=99))
    capsys.readouterr()
    assert listed(unpacked) == every
    assert "WARNING" not in capsys.readouterr().out
    assert listed(packed) == every
    assert "WARNING" not in capsys.readouterr().out
    names = samples_utils.get_samples_dir_filenames(str(packed))
    assert sorted(os.path.basename(n) for n in names) == ["10.miso_db", "X.miso_db", "chr1.miso_db"]
    assert listed(mixed) == every
    assert "WARNING: Directory %s has both *.miso and *.miso_db files" % mixed in capsys.readouterr().out
    files, rows = samples_utils.list_events(str(mixed))
    assert str(mixed / "X" / "ev_X_1.miso") in files                               # the file beats the row
    assert "ev_X_1" not in rows[str(mixed / "X.miso_db")] and "ev_X_0" in rows[str(mixed / "X.miso_db")]
    # a database one level down is found too (the reference lists both places)
    (tmp_path / "deep" / "sub").mkdir(parents=True)
    os.rename(str(packed / "10.miso_db"), str(tmp_path / "deep" / "sub" / "10.miso_db"))
    assert listed(tmp_path / "deep") == sorted(tree["10"])


def test_packed_event_parses_like_its_file(tmp_path):
    root = tmp_path / "out"
    tree = make_tree(root)
    want = {n: samples_utils.parse_miso_file(str(root / c / (n + ".miso"))) for c, ev in tree.items() for n in ev}
    assert miso_pack.main(["--pack", str(root)]) == 0
    seen = 0
    for chrom in tree:
        with miso_db.MISODatabase(str(root / (chrom + ".miso_db"))) as db:
            for name, rows, header in db:
                got = samples_utils.parse_miso_text(name, header, rows)
                assert got[0] == want[name][0] and got[2] == want[name][2]
                assert got[1].tobytes() == want[name][1].tobytes() and got[1].shape == want[name][1].shape
                seen += 1
    assert seen == len(want)


def test_text_shape():
    bodies = [b"0.1000,0.9000\t-1.50\n0.2000,0.8000\t-2.50\n",          # plain
              b"\n0.1,0.2,0.7\t-1\n\n\n0.3,0.3,0.4\t-2\n\n",              # blank lines (get_event_data_as_stream adds some)
              b"0.5000\t-3.00\n0.2500\t-4.00",                             # no final LF, one isoform
              b"0.1,0.2,0.3,0.4,0.0\tnan\n",                               # one row
              b"",                                                         # empty
              b"\n\n",                                                     # only blank lines
              b"0.1,0.9 no tab here\n0.1,0.9\t-1\n"]                       # commas of the whole first line
    text = b"".join(bodies)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bodies])])
    K, rows = capi.text_shape(text, offs)
    assert K.tolist() == [2, 3, 1, 5, 0, 0, 2]
    assert rows.tolist() == [2, 2, 2, 1, 0, 0, 2]
    K0, rows0 = capi.text_shape(b"", [0])
    assert len(K0) == 0 and len(rows0) == 0
    with pytest.raises(ValueError):
        capi.text_shape(text, [0, len(text) + 1])
    # many events: the threaded path gives what the single events give
    many = bodies * 300
    offs = np.concatenate([[0], np.cumsum([len(b) for b in many])])
    K, rows = capi.text_shape(b"".join(many), offs)
    assert K.tolist() == [2, 3, 1, 5, 0, 0, 2] * 300 and rows.tolist() == [2, 2, 2, 1, 0, 0, 2] * 300


def test_decoder_switch_is_checked(monkeypatch):
    monkeypatch.setenv("MISO_TEXT_DECODE", "gpu")
    with pytest.raises(ValueError, match="host.*device"):
        samples_utils._decoder(None)
    assert samples_utils._decoder("device") == "device"
    monkeypatch.setenv("MISO_TEXT_DECODE", "device")
    assert samples_utils._decoder(None) == "device"
    monkeypatch.delenv("MISO_TEXT_DECODE")
    assert samples_utils._decoder(None) == samples_utils.DEFAULT_DECODER


def test_no_cpu_fallback_without_device():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    body = b"0.1000,0.9000\t-1.50\n0.2000,0.8000\t-2.50\n"
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.SamplesBatch.from_text(body, [0, len(body)], [2], 2)
    text = np.frombuffer(body, np.uint8)
    offs, K, status = np.array([0, len(body)], np.int64), np.array([2], np.int32), np.zeros(1, np.int32)
    h = ctypes.c_void_p()
    L = capi.lib()
    L.miso_batch_from_miso_text.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rc = L.miso_batch_from_miso_text(1, capi._p(text), capi._p(offs), capi._p(K), 2, 0, 0, ctypes.byref(h),
                                     capi._p(status), None)
    assert rc == capi.MISO_ENODEVICE and not h.value
    assert b"no HIP device" in L.miso_last_error()
