"""misopy/miso_db.py for Python 3: the packed form of a directory of `.miso` files, one SQLite file per chromosome
directory.

    <parent>/<dirname>.miso_db, one table `table_<dirname>` (the prefix because Ensembl chromosome names are numeric)
    with the columns (event_name text, psi_vals_and_scores text, header text); one row per `<event>.miso` file directly
    in the directory: event_name = the file name without `.miso`, header = the file's first two lines (newlines
    included), psi_vals_and_scores = everything after them, unchanged.

The format is the interface: what this module writes the reference reads, and the other way round.  Deviations, all on
the writing side: rows are inserted in sorted file-name order (the reference's order is the file system's), and the
database is written under a temporary name beside its target and renamed when complete, so an interrupted pack never
leaves a `.miso_db` that the packer's "exists, move on" rule would trust.  Compressed event IDs (`--use-compressed`,
`.shelve` maps) are out of scope: names are stored and returned as the files have them.
"""
import os
import sqlite3

MISO_DB_EXT = ".miso_db"
MISO_EXT = ".miso"


def is_miso_db_fname(fname):
    return fname.endswith(MISO_DB_EXT)


def is_miso_unpacked_dir(dirname):
    """A directory with `.miso` files DIRECTLY inside it (those of a sub-directory do not count)."""
    return os.path.isdir(dirname) and any(f.endswith(MISO_EXT) for f in os.listdir(dirname))


def strip_miso_ext(filename):
    return filename[:-len(MISO_EXT)] if filename.endswith(MISO_EXT) else filename


def get_table_name_from_file(db_fname):
    base = os.path.basename(db_fname)
    return base[:-len(MISO_DB_EXT)] if base.endswith(MISO_DB_EXT) else None


def miso_filenames(dirname):
    """The `.miso` files directly in dirname, sorted by name."""
    return sorted(os.path.join(dirname, f) for f in os.listdir(dirname)
                  if f.endswith(MISO_EXT) and os.path.isfile(os.path.join(dirname, f)))


def split_miso_text(text):
    """(header, psi_vals_and_scores) of a `.miso` file's text: its first two lines, and the rest."""
    cut = text.find("\n")
    cut = text.find("\n", cut + 1) if cut >= 0 else -1
    return (text, "") if cut < 0 else (text[:cut + 1], text[cut + 1:])


def load_miso_file_as_str(miso_filename):
    """newline="": the text as the file has it (no newline translation), so that header + rows IS the file."""
    with open(miso_filename, newline="") as f:
        return split_miso_text(f.read())


class MISODatabase:
    """One `.miso_db` file, read-only; the table name comes from the file name.  text_factory=bytes hands the text
    columns over undecoded (the bulk reader of miso_amd/samples_utils.py)."""

    def __init__(self, db_fname, text_factory=str):
        if not os.path.isfile(db_fname):
            raise FileNotFoundError("%s does not exist." % db_fname)
        name = get_table_name_from_file(db_fname)
        if name is None:
            raise ValueError("Cannot retrieve name of MISO db file %s" % db_fname)
        self.db_fname = db_fname
        self.table_name = "table_%s" % name
        self.conn = sqlite3.connect("file:%s?mode=ro" % _uri_path(db_fname), uri=True)
        self.conn.text_factory = text_factory

    def close(self):
        self.conn.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _table(self):
        return '"%s"' % self.table_name.replace('"', '""')

    def get_all_events(self):
        """Iterator over (event_name, psi_vals_and_scores, header): one SELECT for the whole table."""
        return self.conn.execute("SELECT event_name, psi_vals_and_scores, header FROM %s" % self._table())

    def __iter__(self):
        return iter(self.get_all_events())

    def get_all_event_names(self):
        return [r[0] for r in self.conn.execute("SELECT event_name FROM %s" % self._table())]

    def get_event_data_as_string(self, event_name):
        """`header + "\\n" + rows + "\\n"` as the reference builds it; None for an unknown name."""
        rows = self.conn.execute("SELECT event_name, psi_vals_and_scores, header FROM %s WHERE event_name=?"
                                 % self._table(), (event_name,)).fetchall()
        if not rows:
            return None
        if len(rows) > 1:
            raise ValueError("More than one entry for event %s" % event_name)
        _, psi_vals_and_scores, header = rows[0]
        return "%s\n%s\n" % (header, psi_vals_and_scores)


def _uri_path(path):
    from urllib.parse import quote
    return quote(os.path.abspath(path))


def miso_dir_to_db(dir_to_compress, output_filename, verbose=True):
    """The `.miso` files directly in dir_to_compress as the database output_filename.  Returns output_filename, or
    None when it already exists.  The database appears under its name only once it is complete."""
    if verbose:
        print("Converting MISO directory into database")
        print("  - MISO dir: %s" % dir_to_compress)
        print("  - Output file: %s" % output_filename)
    if not os.path.isdir(dir_to_compress):
        raise NotADirectoryError("%s not a directory" % dir_to_compress)
    if os.path.exists(output_filename):
        print("Error: Database %s already exists, aborting." % output_filename)
        return None
    fnames = miso_filenames(dir_to_compress)
    if verbose:
        print("  - %d files to compress" % len(fnames))
    table = '"table_%s"' % os.path.basename(os.path.normpath(dir_to_compress)).replace('"', '""')
    tmp = "%s.tmp%d" % (output_filename, os.getpid())
    if os.path.exists(tmp):
        os.remove(tmp)
    try:
        conn = sqlite3.connect(tmp)
        try:
            conn.execute("CREATE TABLE %s (event_name text, psi_vals_and_scores text, header text)" % table)
            conn.executemany("INSERT INTO %s VALUES (?, ?, ?)" % table, (_row_of(f) for f in fnames))
            conn.commit()
        finally:
            conn.close()
        os.rename(tmp, output_filename)
    except BaseException:
        for leftover in (tmp, tmp + "-journal"):
            if os.path.exists(leftover):
                os.remove(leftover)
        raise
    return output_filename


def _row_of(miso_fname):
    header, rows = load_miso_file_as_str(miso_fname)
    return strip_miso_ext(os.path.basename(miso_fname)), rows, header
