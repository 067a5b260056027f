"""GPU: the `.miso` sample text decoded on the device (kernels_text.hip text_decode_kernel through
capi.SamplesBatch.from_text) against Python's float(), bit for bit, and summarize / compare over packed, unpacked and
damaged trees with the `device` and the `host` decoder: byte-identical tables."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from miso_amd import capi, miso_pack, samples_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))
DATA = os.path.join(ROOT, "tests", "golden", "data")

pytestmark = pytest.mark.gpu

SCORES = ["-1.50", "-123456.78", "nan", "-0.00", "inf", "-inf", "-17.25", "0.00", "-99999999999999999999.99"]


def body_of(rows, score0=0):
    """rows: lists of field strings -> the event's text, log scores cycling through SCORES."""
    return "".join("%s\t%s\n" % (",".join(r), SCORES[(score0 + i) % len(SCORES)]) for i, r in enumerate(rows)).encode()


def expected(rows):
    return np.array([[float(f) for f in r] for r in rows], dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def random_decimal(rng):
    """1 - 15 significant digits, 0 - 22 decimals, a sign now and then; sometimes all zeros ("-0.0000")."""
    d, f = int(rng.integers(1, 16)), int(rng.integers(0, 23))
    m = 0 if rng.random() < 0.02 else int(rng.integers(10 ** (d - 1), 10 ** d))
    s = str(m)
    if f:
        s = s.rjust(f + 1, "0")
        s = s[:-f] + "." + s[-f:]
    if rng.random() < 0.1:
        s = "00" + s                                # leading zeros are not significant
    return ("-" if rng.random() < 0.3 else "") + s


def decode(bodies, want_K, want_S, chunk_bytes=0):
    """Every body through text_shape and from_text (one batch per sample count): ([samples], [status], [stats])."""
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    text = b"".join(bodies)
    K, S = capi.text_shape(text, offs)
    assert K.tolist() == list(want_K) and S.tolist() == list(want_S)
    samples, status, stats = [None] * len(bodies), [None] * len(bodies), []
    for s in sorted(set(S.tolist())):
        idx = [i for i in range(len(bodies)) if S[i] == s]
        sub = [bodies[i] for i in idx]
        o = np.concatenate([[0], np.cumsum([len(b) for b in sub])]).astype(np.int64)
        b = capi.SamplesBatch.from_text(b"".join(sub), o, [K[i] for i in idx], s, chunk_bytes=chunk_bytes)
        stats.append(b.text_stats)
        for j, i in enumerate(idx):
            samples[i], status[i] = b.samples(j), int(b.status[j])
    return samples, status, stats


def check_exact(all_rows, chunk_bytes=0):
    bodies = [body_of(r, score0=i) for i, r in enumerate(all_rows)]
    samples, status, stats = decode(bodies, [len(r[0]) for r in all_rows], [len(r) for r in all_rows], chunk_bytes)
    assert status == [0] * len(bodies)
    for i, r in enumerate(all_rows):
        want = expected(r)
        assert samples[i].shape == want.shape
        diff = np.nonzero(bits(samples[i]) != bits(want))
        assert diff[0].size == 0, (i, [(r[a][b], samples[i][a, b]) for a, b in zip(*diff)][:5])
    return stats


def test_fixed_four_decimals_of_random_psi():
    rng = np.random.default_rng(11)
    all_rows = []
    for K in (1, 2, 5, 20):
        for S in (1, 2, 7, 64, 513, 2700, 5000):
            psi = rng.dirichlet(np.ones(K), size=S) if K > 1 else rng.random((S, 1))
            all_rows.append([["%.4f" % v for v in row] for row in psi])
    stats = check_exact(all_rows)
    assert all(s["not_decoded"] == 0 and s["kernel_ms"] > 0 for s in stats)


def test_every_four_decimal_value_of_the_unit_interval():
    vals = ["%.4f" % (i / 10000.0) for i in range(10001)]
    assert vals[0] == "0.0000" and vals[-1] == "1.0000" and len(set(vals)) == 10001
    padded = vals + ["0.0000"] * 4
    check_exact([[[v] for v in vals],                                         # K = 1, 10 001 rows
                 [padded[i:i + 5] for i in range(0, len(padded), 5)],          # K = 5
                 [[v, vals[10000 - i]] for i, v in enumerate(vals)][:5000],    # K = 2
                 [["-0.0000", "0.0000", "-0.5000"]]])                           # the sign is applied last: -0.0


def test_random_decimals_up_to_15_digits_and_22_decimals():
    rng = np.random.default_rng(12)
    all_rows = [[[random_decimal(rng) for _ in range(K)] for _ in range(S)]
                for K, S in ((1, 5000), (2, 2700), (5, 2700), (20, 1000), (3, 1), (7, 33))]
    # the corners of the grammar by hand
    all_rows.append([["999999999999999", "0.0000000000000000000001", "-123456789.012345", "1", "0",
                      "0.999999999999999", "9007199254.74099", "0.0000000999999999999999"]])
    check_exact(all_rows)


def test_chunked_stream_gives_the_same_pool():
    """Dozens of chunks, and one event larger than a chunk: the pool does not depend on the chunk size."""
    rng = np.random.default_rng(13)
    S = 513
    all_rows = [[["%.4f" % v for v in row] for row in rng.dirichlet(np.ones(2), size=S)] for _ in range(60)]
    all_rows.insert(17, [[random_decimal(rng) for _ in range(20)] for _ in range(S)])     # ~ 100 KB of text
    bodies = [body_of(r, score0=i) for i, r in enumerate(all_rows)]
    assert max(len(b) for b in bodies) > 3 * 32768 > 32768 > min(len(b) for b in bodies)
    whole = check_exact(all_rows)
    small = check_exact(all_rows, chunk_bytes=32768)
    assert whole[0]["chunks"] == 1 and small[0]["chunks"] >= 24
    one, _, _ = decode(bodies, [len(r[0]) for r in all_rows], [S] * len(bodies))
    many, _, _ = decode(bodies, [len(r[0]) for r in all_rows], [S] * len(bodies), chunk_bytes=32768)
    assert all(bits(a).tobytes() == bits(b).tobytes() for a, b in zip(one, many))


def test_events_outside_the_grammar_get_a_status_and_cost_nobody_else():
    rng = np.random.default_rng(14)
    K, S = 3, 6

    def good():
        return [["%.4f" % v for v in row] for row in rng.dirichlet(np.ones(K), size=S)]

    def text(rows, **kw):
        return body_of(rows, **kw)

    g = [good() for _ in range(12)]
    bad = {}
    r = good(); r[2][1] = "0.1234567890123456"; bad[1] = (text(r), capi.MISO_TEXT_EPSI)             # 16 digits
    r = good(); r[0][0] = "1.2340e-01"; bad[3] = (text(r), capi.MISO_TEXT_EPSI)                     # an exponent
    r = good(); r[5][2] = "nan"; bad[5] = (text(r), capi.MISO_TEXT_EPSI)                            # nan as psi
    r = good(); r[3] = r[3][:2]; bad[7] = (text(r), capi.MISO_TEXT_EROW)                            # a short row
    bad[9] = (text(good()).replace(b"\t", b" ", 1), None)                                            # a row without TAB
    bad[10] = (text(good()).replace(b"\n", b"\r\n"), None)                                           # CRLF line ends
    r = good(); r[1][0] = "0." + "0" * 22 + "1"; bad[11] = (text(r), capi.MISO_TEXT_EPSI)           # 23 decimals
    bad[12] = (text(good()).replace(b"\tnan\n", b"\tNaN\n"), capi.MISO_TEXT_ESCORE)                  # another spelling
    assert b"NaN" in bad[12][0]
    bodies, rows_of, flags = [], [], []
    gi = iter(g)
    for i in range(20):
        if i in bad:
            bodies.append(bad[i][0]); rows_of.append(None); flags.append(bad[i][1])
        else:
            rows = next(gi, None) or good()
            bodies.append(text(rows, score0=i)); rows_of.append(rows); flags.append(0)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    for chunk in (0, 256):
        b = capi.SamplesBatch.from_text(b"".join(bodies), offs, [K] * len(bodies), S, chunk_bytes=chunk)
        for i, (rows, flag) in enumerate(zip(rows_of, flags)):
            if rows is None:
                assert b.status[i] != 0, i
                if flag:
                    assert b.status[i] & flag, (i, b.status[i])
            else:
                assert b.status[i] == 0, (i, b.status[i])
                assert bits(b.samples(i)).tobytes() == bits(expected(rows)).tobytes(), i
        assert b.text_stats["not_decoded"] == len(bad) and b.text_stats["decoded"] == len(bodies) - len(bad)


def test_row_count_other_than_the_batch_s_is_a_status_and_stays_inside_its_region():
    rng = np.random.default_rng(15)
    K, S = 2, 60
    rows = [[["%.4f" % v for v in row] for row in rng.dirichlet(np.ones(K), size=n)] for n in (S, S - 1, S, S + 40, S, 0, S)]
    bodies = [body_of(r, score0=i) for i, r in enumerate(rows)]
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    b = capi.SamplesBatch.from_text(b"".join(bodies), offs, [K] * len(bodies), S)
    assert [int(s) for s in b.status] == [0, capi.MISO_TEXT_ECOUNT, 0, capi.MISO_TEXT_ECOUNT, 0, capi.MISO_TEXT_ECOUNT, 0]
    for i in (0, 2, 4, 6):
        assert bits(b.samples(i)).tobytes() == bits(expected(rows[i])).tobytes(), i
    b.summarize(0.95)                                   # the batch is a samples batch like any other
    m, lo, hi = b.summary(0)
    want = expected(rows[0])
    assert abs(m[0] - want[:, 0].mean()) < 1e-12 and lo[0] <= m[0] <= hi[0]


def write_two_sample_trees(tmp_path):
    """Two sample trees written by run_sampler_batch (as tests/test_gpu_frontend.py
    test_summarize_and_compare_existing_miso_directories makes them): 72 events of 2 - 4 isoforms on three chromosomes."""
    import miso_sampler
    from miso_sampler import SimpleGene
    rng = np.random.default_rng(5)
    dirs = []
    for label, shift in (("ctl", 0.0), ("kd", 0.25)):
        out = tmp_path / "unpacked" / label
        params = miso_sampler.get_single_end_sampler_params(2, 36, 1)
        sampler = miso_sampler.MISOSampler(params, paired_end=False)
        events = []
        for e in range(72):
            K = 2 + (e % 3)
            exons = [(1 + 200 * i, 100 + 200 * i) for i in range(K + 1)]
            isoforms = [list(range(K + 1))] + [[x for x in range(K + 1) if x != k] for k in range(1, K)]
            gene = SimpleGene(exons, isoforms, label="ev%03d" % e, chrom="chr%d" % (e % 3))
            n = 60 + 7 * e
            pos = rng.integers(1, 200 * K + 60, size=n)
            if shift:
                pos = np.where(rng.random(n) < shift, rng.integers(1, 60, size=n), pos)
            events.append(((list(int(x) for x in pos), ["36M"] * n), gene, str(out / gene.chrom / gene.label)))
        sampler.run_sampler_batch(600, events, num_chains=2, burn_in=100, lag=2, seed=9, first_event_id=0,
                                  summary_file=str(tmp_path / (label + ".live_summary")))
        dirs.append(str(out))
    return dirs


def summarize(samples_dir, out_dir, decoder, monkeypatch):
    monkeypatch.setenv("MISO_TEXT_DECODE", decoder)
    assert samples_utils.main(["--summarize-samples", samples_dir, out_dir]) == 0
    label = os.path.basename(samples_dir)
    return open(os.path.join(out_dir, "summary", label + ".miso_summary"), "rb").read(), dict(samples_utils.last_decode_stats)


def compare(d1, d2, out_dir, decoder, monkeypatch):
    monkeypatch.setenv("MISO_TEXT_DECODE", decoder)
    assert samples_utils.main(["--compare-samples", d1, d2, out_dir]) == 0
    name = "%s_vs_%s" % (os.path.basename(d1), os.path.basename(d2))
    return (open(os.path.join(out_dir, name, "bayes-factors", name + ".miso_bf"), "rb").read(),
            dict(samples_utils.last_decode_stats))


def test_packed_and_unpacked_trees_give_the_same_tables_with_either_decoder(tmp_path, monkeypatch):
    dirs = write_two_sample_trees(tmp_path)
    packed = []
    for d in dirs:
        p = str(tmp_path / "packed" / os.path.basename(d))
        shutil.copytree(d, p)
        assert miso_pack.main(["--pack", p]) == 0
        assert sorted(os.listdir(p)) == ["chr0.miso_db", "chr1.miso_db", "chr2.miso_db"]
        packed.append(p)
    for which, (u, p) in enumerate(zip(dirs, packed)):
        tables = {}
        for form, d in (("unpacked", u), ("packed", p)):
            for decoder in ("host", "device"):
                tables[form, decoder], st = summarize(d, str(tmp_path / "sum" / form / decoder), decoder, monkeypatch)
                assert st["decoder"] == decoder
                if decoder == "device":
                    # every event took the device path: a test that passes because everything fell back shows nothing
                    assert st["fallback_events"] == [] and st["fallback_share"] == 0 and st["device_events"] == 72
                    assert st["kernel_ms"] > 0 and st["text_bytes"] > 72 * 500 * 10
        assert len(set(tables.values())) == 1, [k for k in tables if tables[k] != tables["unpacked", "host"]]
        assert len(tables["unpacked", "host"].splitlines()) == 73
        live = sorted(open(str(tmp_path / (("ctl", "kd")[which] + ".live_summary"))).read().splitlines()[1:])
        assert sorted(tables["packed", "device"].decode().splitlines()[1:]) == live
    tables = {}
    for form, (d1, d2) in (("unpacked", dirs), ("packed", packed)):
        for decoder in ("host", "device"):
            tables[form, decoder], st = compare(d1, d2, str(tmp_path / "cmp" / form / decoder), decoder, monkeypatch)
            if decoder == "device":
                assert st["fallback_events"] == [] and st["fallback_share"] == 0 and st["device_events"] == 144
    assert len(set(tables.values())) == 1, [k for k in tables if tables[k] != tables["unpacked", "host"]]
    assert len(tables["unpacked", "host"].splitlines()) == 73


def test_events_the_device_decoder_leaves_fall_back_to_the_host_parser(tmp_path, monkeypatch):
    dirs = write_two_sample_trees(tmp_path)
    ctl = dirs[0]

    def rewrite(name, field):
        path = os.path.join(ctl, "chr%d" % (int(name[2:]) % 3), name + ".miso")
        lines = open(path).read().splitlines(keepends=True)
        out = lines[:2]
        for ln in lines[2:]:
            psi, score = ln.rstrip("\n").split("\t")
            out.append("%s\t%s\n" % (",".join(field(v) for v in psi.split(",")), score))
        open(path, "w").write("".join(out))

    rewrite("ev007", lambda v: "%.4e" % float(v))          # the same values in exponent notation
    rewrite("ev041", lambda v: "nan")                      # rows of nan
    for form in ("unpacked", "packed"):
        if form == "packed":
            for d in dirs:
                assert miso_pack.main(["--pack", d]) == 0
        host, _ = summarize(ctl, str(tmp_path / "sum" / form / "host"), "host", monkeypatch)
        dev, st = summarize(ctl, str(tmp_path / "sum" / form / "device"), "device", monkeypatch)
        assert dev == host and len(host.splitlines()) == 73
        assert sorted(st["fallback_events"]) == ["ev007", "ev041"] and st["device_events"] == 70
        hostc, _ = compare(ctl, dirs[1], str(tmp_path / "cmp" / form / "host"), "host", monkeypatch)
        devc, st = compare(ctl, dirs[1], str(tmp_path / "cmp" / form / "device"), "device", monkeypatch)
        assert devc == hostc and len(hostc.splitlines()) == 73
        assert sorted(st["fallback_events"]) == ["ev007", "ev041"]
    # the exponent notation holds the same decimals: that event's row is the one the untouched tree gives
    live = [l for l in open(str(tmp_path / "ctl.live_summary")).read().splitlines() if l.startswith("ev007\t")]
    assert live and live[0] in dev.decode().splitlines()


def run(args, **env):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=600)


def test_miso_run_then_pack_then_summarize_on_reference_test_data(tmp_path):
    with gzip.open(os.path.join(DATA, "c2c12.Atp2b1.sam.gz"), "rt") as f:
        sam_text = f.read()
    aln = str(tmp_path / "c2c12.Atp2b1.sam")
    open(aln, "w").write(sam_text)
    idx, out = str(tmp_path / "indexed"), str(tmp_path / "out")
    settings = tmp_path / "settings.txt"
    settings.write_text("[data]\nfilter_results = True\nmin_event_reads = 20\n"
                        "[sampler]\nburn_in = 200\nlag = 4\nnum_iters = 1000\nnum_chains = 2\n")
    r = run(["-m", "miso_amd.index_gff", "--index", os.path.join(DATA, "Atp2b1.mm9.gff"), idx])
    assert r.returncode == 0, r.stdout
    r = run(["-m", "miso_amd.miso", "--run", idx, aln, "--output-dir", out, "--read-len", "36",
             "--settings-filename", str(settings), "-p", "1", "--seed", "31"])
    assert r.returncode == 0, r.stdout
    miso_file = os.path.join(out, "10", "ENSMUSG00000019943.miso")
    assert os.path.isfile(miso_file), r.stdout
    tables = {}
    for decoder in ("host", "device"):
        r = run(["-m", "miso_amd.samples_utils", "--summarize-samples", out, str(tmp_path / "before" / decoder)],
                MISO_TEXT_DECODE=decoder)
        assert r.returncode == 0, r.stdout
        tables["before", decoder] = open(str(tmp_path / "before" / decoder / "summary" / "out.miso_summary"), "rb").read()
    r = run(["-m", "miso_amd.miso_pack", "--pack", out])
    assert r.returncode == 0, r.stdout
    assert os.path.isfile(os.path.join(out, "10.miso_db")) and not os.path.exists(os.path.join(out, "10"))
    r = run(["-m", "miso_amd.miso_pack", "--view", os.path.join(out, "10.miso_db")])
    assert r.returncode == 0 and r.stdout.splitlines() == ["Database contains 1 events", "ENSMUSG00000019943"], r.stdout
    for decoder in ("host", "device"):
        r = run(["-m", "miso_amd.samples_utils", "--summarize-samples", out, str(tmp_path / "after" / decoder)],
                MISO_TEXT_DECODE=decoder)
        assert r.returncode == 0, r.stdout
        tables["after", decoder] = open(str(tmp_path / "after" / decoder / "summary" / "out.miso_summary"), "rb").read()
    assert len(set(tables.values())) == 1 and b"ENSMUSG00000019943" in tables["after", "device"]
