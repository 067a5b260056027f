"""misopy/miso_pack.py for Python 3: pack the `.miso` files of a MISO output tree into one SQLite database per
chromosome directory (miso_amd/miso_db.py), or list a database.

    python -m miso_amd.miso_pack --pack DIR[,DIR...]
    python -m miso_amd.miso_pack --view DB

`--pack` walks each directory given; every directory below it that holds `*.miso` files directly becomes its sibling
`<dirname>.miso_db` and is then removed.  Where the `.miso_db` already exists the directory is left alone ("move on").
summarize / compare (miso_amd/samples_utils.py) read packed, unpacked and mixed trees alike.

One deviation from the reference, which removes the directory whatever the conversion returned (miso_pack.py:73-76)
and so loses the data of a failed pack: here the directory is removed only after the finished database has been
reopened and checked against it -- as many rows as `*.miso` files, and for every row header + rows as long as the file.
On any failure the directory stays, the partial database goes, the failure is reported and the run ends non-zero after
the remaining directories have been tried.
"""
import os
import shutil
import sqlite3
import sys
import time

from . import miso_db


def _pathify(p):
    return os.path.abspath(os.path.expanduser(p))


def verify_packed(dirname, db_fname):
    """Raises ValueError unless db_fname holds exactly dirname's `.miso` files, each with its full length."""
    sizes = {miso_db.strip_miso_ext(os.path.basename(f)): os.path.getsize(f) for f in miso_db.miso_filenames(dirname)}
    db = miso_db.MISODatabase(db_fname)
    try:
        got = db.conn.execute("SELECT event_name, length(CAST(header AS BLOB)) + length(CAST(psi_vals_and_scores AS BLOB)) "
                              "FROM %s" % db._table()).fetchall()
    finally:
        db.close()
    if len(got) != len(sizes):
        raise ValueError("%d rows for %d .miso files" % (len(got), len(sizes)))
    for name, n in got:
        if sizes.get(name) != n:
            raise ValueError("event %s: %s bytes packed, %s in the file" % (name, n, sizes.get(name)))


def pack_dir(dir_to_compress):
    """One `*.miso`-holding directory -> its sibling database.  True: packed and removed; None: the database was
    already there, nothing touched.  Raises on failure, with the directory intact and no database left."""
    base = os.path.basename(os.path.normpath(dir_to_compress))
    if not base:
        raise ValueError("Basename for %s is empty!" % dir_to_compress)
    db_fname = os.path.join(os.path.dirname(os.path.normpath(dir_to_compress)), base + miso_db.MISO_DB_EXT)
    if os.path.exists(db_fname):                         # if the packed file exists, move on
        return None
    if miso_db.miso_dir_to_db(dir_to_compress, db_fname) is None:     # (a failed conversion leaves no database)
        raise ValueError("%s appeared while packing" % db_fname)
    try:
        verify_packed(dir_to_compress, db_fname)
    except BaseException:
        if os.path.exists(db_fname):
            os.remove(db_fname)
        raise
    shutil.rmtree(dir_to_compress)
    return True


def pack_dirs(miso_dirnames):
    """Every `*.miso`-holding directory at or below the given ones.  Returns the number of directories that failed."""
    t1 = time.time()
    failed = 0
    for miso_dirname in miso_dirnames:
        print("Processing: %s" % miso_dirname)
        if not os.path.isdir(miso_dirname):
            print("Error: %s not a directory." % miso_dirname)
            sys.exit(1)
        # (listed before anything is removed: the walk never steps into a directory that is going away)
        todo = [d for d, _, _ in os.walk(miso_dirname) if miso_db.is_miso_unpacked_dir(d)]
        for d in sorted(todo):
            try:
                pack_dir(d)
            except (OSError, ValueError, sqlite3.Error) as err:
                failed += 1
                print("Error: Failed to pack MISO directory %s: %s (directory kept)" % (d, err))
    print("Packing took %.2f minutes" % ((time.time() - t1) / 60.))
    return failed


def pack_miso_output(dirs_to_pack_as_str):
    return pack_dirs([_pathify(d) for d in dirs_to_pack_as_str.split(",") if d])


def view_miso_db(db_fname):
    db_fname = _pathify(db_fname)
    if not os.path.isfile(db_fname):
        print("Error: %s does not exist." % db_fname)
        sys.exit(1)
    db = miso_db.MISODatabase(db_fname)
    try:
        names = db.get_all_event_names()
    finally:
        db.close()
    print("Database contains %d events" % len(names))
    for name in names:
        print(name)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Pack the MISO output into SQLite databases (.miso_db), or view one")
    ap.add_argument("--pack", default=None, metavar="DIR[,DIR...]",
                    help="a directory, or a comma-separated set of directories, that contain MISO output")
    ap.add_argument("--view", default=None, metavar="DB", help="list a MISO database (.miso_db file)")
    a = ap.parse_args(argv)
    if a.pack is None and a.view is None:
        ap.print_help()
        return 1
    status = 0
    if a.pack is not None:
        if pack_miso_output(a.pack):
            status = 1
    if a.view is not None:
        view_miso_db(a.view)
    return status


if __name__ == "__main__":
    sys.exit(main())
