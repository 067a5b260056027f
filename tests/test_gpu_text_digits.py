"""GPU: csrc/text_digits.hpp text_digits -- the rounding behind summarize(as_text=True) -- on its own
(miso_selftest_text_digits) against the digits Python's "%.4f" prints, bit-exact with no exceptions, and the same values
through the product: a hand-written `.miso` event summarised with either decoder against the doubles through
SamplesBatch(...).summarize(as_text=True).

Before the routine decided |p - r| = 1/2 by the sign of the product's rounding error, the device printed the nearest
doubles to 5e-05, 0.00025, 0.00035, 0.00095 and 0.00645 (and their negatives) one digit off: 0, 2, 4, 10, 64 where
"%.4f" prints 1, 3, 3, 9, 65 (tests/test_text_digits_ref.py cross-checks that reference against decimal.Decimal)."""
import os

import numpy as np
import pytest

import _text_points as P
from _summary_ref import credible_interval, tree_mean
from miso_amd import capi, samples_utils, summary

pytestmark = pytest.mark.gpu


def test_text_digits_equal_format_on_every_point_set():
    """One launch over all sets (~1.5 million doubles): every decimal tie (k + 0.5) / 10^4 +- 6 ulps in both signs, the
    true binary ties j / 32 up to 2, every k / 10^4 +- 3 ulps, zeros, subnormals, values and ties up to 2 x 10^5, and
    10^6 random doubles of [0, 1]."""
    sets = [("decimal ties", P.decimal_ties()), ("binary ties", P.binary_ties()), ("grid", P.grid()), ("edges", P.edges()),
            ("random", P.random_unit())]
    v = np.concatenate([s for _, s in sets])
    assert len(sets[-1][1]) == 10 ** 6
    dev = capi.selftest_text_digits(v)
    want = P.digits_by_format(v)
    bad = np.nonzero(dev != want)[0]
    names = np.repeat([n for n, _ in sets], [len(s) for _, s in sets])
    print("text_digits: %d of %d doubles off" % (len(bad), len(v)))
    for i in bad[:40]:
        print("  %-12s %-24r %s device %d \"%%.4f\" %d" % (names[i], float(v[i]), float(v[i]).hex(), dev[i], want[i]))
    assert len(bad) == 0, [(float(v[i]), int(dev[i]), int(want[i])) for i in bad[:20]]


def test_the_tie_neighbours_by_name():
    v = np.array(P.TIE_NEIGHBOURS + tuple(-x for x in P.TIE_NEIGHBOURS))
    assert ["%.4f" % x for x in P.TIE_NEIGHBOURS] == ["0.0001", "0.0003", "0.0003", "0.0009", "0.0065"]
    assert capi.selftest_text_digits(v).tolist() == [1, 3, 3, 9, 65, -1, -3, -3, -9, -65]


# ---- the product path ----
S_EVENT = 100     # 0.95: the bounds are the order statistics 2 and 97


def _tie_event_columns():
    """Two columns of doubles.  Column 0: the five tie neighbours under 95 ordinary values -- the lower bound (rank 2)
    is 0.0003, where digits one off (0, 2, 4, 10, 64) would give 0.0004.  Column 1: the five above 95 zeros -- the
    upper bound (rank 97) is 0.0003 against 0.0004.  The digit sums are 81 + the ordinary rows' against 80 +."""
    rng = np.random.default_rng(77)
    ordinary = 0.05 + 0.9 * rng.random(S_EVENT - 5)
    c0 = np.concatenate([ordinary[:40], P.TIE_NEIGHBOURS, ordinary[40:]])
    c1 = np.concatenate([np.zeros(30), P.TIE_NEIGHBOURS[::-1], np.zeros(S_EVENT - 35)])
    return np.stack([c0, c1], axis=1)


def _write_event(path, cols):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("#isoforms=['a_b_c','a_c']\texon_lens=('a',100),('b',60),('c',100)\titers=%d\tburn_in=0\tlag=1\t"
                "percent_accept=100.00\tproposal_type=drift\tcounts=(0,1):40,(1,0):30,(1,1):30\t"
                "assigned_counts=0:55,1:45\tchrom=chr1\tstrand=+\tmRNA_starts=100,100\tmRNA_ends=599,599\n" % len(cols))
        f.write("sampled_psi\tlog_score\n")
        for i, row in enumerate(cols):
            f.write("%s\t%.4f\n" % (",".join("%.4f" % x for x in row), -100.0 - 0.25 * i))


def test_tie_neighbours_through_a_miso_file_and_through_as_text(tmp_path, monkeypatch):
    cols = _tie_event_columns()
    samples_dir = str(tmp_path / "ties")
    _write_event(os.path.join(samples_dir, "chr1", "tie_event.miso"), cols)
    text = open(os.path.join(samples_dir, "chr1", "tie_event.miso")).read()
    for s in ("0.0001", "0.0003", "0.0009", "0.0065"):
        assert ("\n%s," % s) in text and (",%s\t" % s) in text

    # what the file hands on, and its exact summary: bounds by credible_intervals.py's rule, mean = digit sum / (S 10^4)
    read = np.array([[float("%.4f" % x) for x in row] for row in cols])
    digits = np.array([[int(("%.4f" % x).replace(".", "")) for x in row] for row in cols])
    want = []
    for k in range(2):
        lo, hi = credible_interval(read[:, k], 0.95)
        want.append((int(digits[:, k].sum()) / (S_EVENT * 10000.0), lo, hi))
    assert want[0][1] == 0.0003 and want[1][2] == 0.0003

    got = {}
    written = summary.write_summary
    for decoder in ("host", "device"):
        seen = []
        monkeypatch.setattr(summary, "write_summary", lambda fn, rows, seen=seen: (seen.extend(rows), written(fn, rows))[1])
        monkeypatch.setenv("MISO_TEXT_DECODE", decoder)
        assert samples_utils.main(["--summarize-samples", samples_dir, str(tmp_path / "out" / decoder)]) == 0
        st = samples_utils.last_decode_stats
        assert st["decoder"] == decoder and st["fallback_events"] == []
        assert len(seen) == 1 and seen[0][0] == "tie_event"
        got[decoder] = [(float(seen[0][1][k]), float(seen[0][2][k]), float(seen[0][3][k])) for k in range(2)]
    monkeypatch.setattr(summary, "write_summary", written)

    b = capi.SamplesBatch([cols])
    b.summarize(0.95, as_text=True)
    m, lo, hi = b.summary(0)
    got["as_text"] = [(float(m[k]), float(lo[k]), float(hi[k])) for k in range(2)]
    for name, g in got.items():
        print(name, g)
    # Bounds: bit for bit in all three.  Mean: as_text gives the exact digit sum over S 10^4, correctly rounded; the file
    # routes sum the parsed doubles in the device's fixed order (tree_mean) -- each pinned to its own reference bit for bit,
    # the two references within 2 ulps of each other (5 + 95 additions of values that are themselves rounded), and one
    # number in the table's "%.2f".
    assert got["host"] == got["device"]
    for k in range(2):
        assert got["as_text"][k] == want[k], (k, got["as_text"][k], want[k])
        file_mean = tree_mean(read[:, k])
        assert abs(file_mean - want[k][0]) <= 2 * np.spacing(want[k][0])
        assert "%.2f" % file_mean == "%.2f" % want[k][0]
        for name in ("host", "device"):
            assert got[name][k] == (file_mean,) + want[k][1:], (name, k, got[name][k])
