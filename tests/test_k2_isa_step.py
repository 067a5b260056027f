"""What the compiler made of the two-isoform step AROUND the read loop in the headline's unit (CPU; reads the assembly the
build keeps, miso_amd/csrc/.isa/kernels_k2m_m0w8.s, and skips as tests/test_k2_isa_loop.py does when it is absent).

The kernel is short of scalar registers (.sgpr_spill_count), so a scalar that is set in front of a body's iteration loop
and read inside it comes back through `v_readlane_b32` in every iteration, and one that the loop updates goes out through
`v_writelane_b32` as well -- VALU instructions that compute nothing, on a step that is VALU-issue bound.  The step keeps
what it carries from iteration to iteration in vector registers (csrc/kernels_k2.inl: k2_lane_const, the recording block,
DetRoute in csrc/detmath_n.hpp); this test holds the static totals per iteration loop to what that build has.

A body's iteration loop is found from the read loop's trips (the single-block loops of tests/test_k2_isa_loop.py): the
backward branches whose span holds exactly one steady and one masked trip loop, overlapping spans merged -- one merged
span per body: twelve lane layouts behind the per-wavefront table, the same twelve and the workgroup-wide chain behind
the runs.  (The compiler does not mark the loop itself: its first iteration is peeled into a second entry.)

Static totals per iteration loop, cold blocks included (the parent's by the same finder, which finds 23 of its 25):

                                                     v_readlane_b32        v_writelane_b32
    all but the kernel's first body and   parent     97 .. 109             2 .. 14
    the workgroup-wide chain              now        25 .. 49              0 .. 8
    those two                             parent     208, 195              49, 45
                                          now        129, 115              30, 43

The four-lane body (the headline's quad-aligned one): 105 and 12 -> 39 and 4, `v_*` 1720 -> 1664; the three-lane body 109
and 14 -> 39 and 2; the two-lane body 109 and 12 -> 35 and 2 (tools/isa_range_count.py on the spans printed here).

The recording block -- the basic block with the sample's 16-byte store, and the blocks before and behind it -- has no
`v_writelane_b32` and no `v_readlane_b32`: the parent read `a.B`, `a.lag`, `a.C` and its two counters there and wrote the
counters back, 17 and 6 per iteration.

What is left inside the loops (hand-read in the four-lane body, docs/history.md 2026-10-20): the four-dword argument tuple
with the seed, in the Metropolis-Hastings draws every fourth iteration and in the cold rescans behind the read loop; the
exact threshold routine's spilled constants; `prio_by_progress` under `balance == 2`.  None of them is on the path of an
iteration without draws, special cases or flagged trips."""
import collections
import re

from test_k2_isa_loop import BIT_OPS, PATH, _trips

LABEL = re.compile(r"(\.LBB\d+_\d+):")
BODIES = 25                    # twelve lane layouts behind the per-wavefront table, the same and the workgroup-wide chain behind the runs
MAX_BODY_LINES = 3500
# A body's lane layout is read off its cross-lane traffic, which no change to the step's scalars touches: (DPP moves,
# ds_bpermute_b32, v_div_scale_f64, s_barrier) of its iteration loop -> lanes per chain.  Every layout has two bodies, one per
# entry path, in the order of the file.  Per body (v_readlane_b32, v_writelane_b32): THIS build's own totals, which the test
# holds, and the parent's (None: that loop is not found in the parent's assembly).
LAYOUTS = {
    #  signature        lanes    this build            the parent
    (0, 0, 14, 0):     (1,      [(49, 0), (49, 0)],    [None, None]),         # (found in part: without the block that stores)
    (0, 16, 36, 0):    (2,      [(35, 2), (35, 2)],    [(109, 12), (101, 2)]),
    (0, 30, 28, 0):    (3,      [(39, 2), (25, 8)],    [(109, 14), (101, 4)]),
    (24, 5, 28, 0):    (4,      [(39, 4), (39, 4)],    [(105, 12), (97, 4)]),
    (0, 32, 28, 0):    (5,      [(39, 2), (25, 8)],    [(109, 14), (101, 4)]),
    (0, 33, 28, 0):    (6,      [(39, 2), (45, 8)],    [(109, 14), (105, 6)]),
    (24, 6, 28, 0):    (8,      [(39, 4), (39, 4)],    [(105, 14), (97, 4)]),
    (0, 37, 28, 0):    (10,     [(39, 2), (29, 8)],    [(109, 14), (105, 6)]),
    (24, 15, 28, 0):   (12,     [(45, 8), (29, 8)],    [(109, 14), (105, 6)]),
    (24, 7, 28, 0):    (16,     [(39, 4), (39, 4)],    [(105, 14), (97, 4)]),
    (24, 8, 28, 0):    (32,     [(39, 4), (39, 4)],    [(105, 14), (101, 6)]),
    (24, 9, 28, 0):    (64,     [(129, 30), (39, 4)],  [(208, 49), (101, 6)]),
    (24, 9, 28, 4):    (512,    [(115, 43)],           [(195, 45)]),          # the workgroup-wide chain
}


def _word(line):
    s = line.strip()
    if not s or s[0] in ";." or s.startswith("//") or s.endswith(":"):
        return None
    return s.split()


def _iteration_loops(lines):
    """[(first, last)] line spans (0-based, inclusive), one per body: merged spans of the backward branches that enclose a
    steady and a masked trip of the read loop"""
    labels = {}
    for i, l in enumerate(lines):
        m = LABEL.match(l.strip())
        if m:
            labels[m.group(1)] = i
    spans = []
    for j, l in enumerate(lines):
        w = _word(l)
        if w and w[0].startswith(("s_cbranch", "s_branch")) and labels.get(w[1].rstrip(","), j) < j:
            spans.append((labels[w[1].rstrip(",")], j))
    steady, masked = [], []
    for lo, hi in spans:
        if any(LABEL.match(lines[i].strip()) for i in range(lo + 1, hi)):
            continue
        c = collections.Counter(w[0] for w in map(_word, lines[lo:hi + 1]) if w)
        if c["v_pk_sub_u16"] != 8 or c["v_mad_u64_u32"] != 24:
            continue
        bit_ops = sum(v for k, v in c.items() if k.startswith(BIT_OPS))
        (steady if bit_ops < 35 + 16 else masked).append(lo)
    def trips_in(lo, hi):
        s, m = [x for x in steady if lo < x < hi], [x for x in masked if lo < x < hi]
        return len(s) == 1 and len(m) == 1 and s[0] < m[0]
    # (exactly one of each, the steady trips first: the Gibbs step in front of a body's loop has trip loops of its own.  At
    # most MAX_BODY_LINES: a body's loop is under 3100 lines; a branch back from a block that two bodies share spans 4500
    # and more, from behind one body's trips to the end of the next)
    cand = sorted((lo, hi) for lo, hi in spans if hi - lo <= MAX_BODY_LINES and trips_in(lo, hi))
    merged = []
    for lo, hi in cand:
        if merged and lo <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(merged[-1][1], hi))
        else:
            merged.append((lo, hi))
    assert all(trips_in(lo, hi) for lo, hi in merged), merged
    return merged, len(steady)


def _blocks(lines, lo, hi):
    """[[line index, ...]] basic blocks of a span, cut at labels and behind branches"""
    out, cur = [], []
    for i in range(lo, hi + 1):
        if LABEL.match(lines[i].strip()) and cur:
            out.append(cur)
            cur = []
        w = _word(lines[i])
        if w:
            cur.append(i)
            if w[0].startswith(("s_cbranch", "s_branch")):
                out.append(cur)
                cur = []
    if cur:
        out.append(cur)
    return out


def body_table(path=PATH):
    """per body: {lines, v_readlane_b32, v_writelane_b32, v_*, the recording block's count and its lane reads and writes}"""
    lines = open(path).read().split("\n")
    loops, n_steady = _iteration_loops(lines)
    rows = []
    for lo, hi in loops:
        c = collections.Counter(w[0] for w in map(_word, lines[lo:hi + 1]) if w)
        blocks = _blocks(lines, lo, hi)
        rec = [k for k, b in enumerate(blocks) if any(_word(lines[i])[0] == "global_store_dwordx4" for i in b)]
        rec_ops = collections.Counter()
        for k in rec:
            for b in blocks[max(k - 1, 0):k + 2]:
                rec_ops += collections.Counter(_word(lines[i])[0] for i in b)
        sig = (sum(v for k, v in c.items() if k.endswith("_dpp")), c["ds_bpermute_b32"], c["v_div_scale_f64"], c["s_barrier"])
        rows.append(dict(first=lo + 1, last=hi + 1, readlane=c["v_readlane_b32"], writelane=c["v_writelane_b32"], sig=sig,
                         valu=sum(v for k, v in c.items() if k.startswith("v_")), n_rec=len(rec),
                         rec_readlane=rec_ops["v_readlane_b32"], rec_writelane=rec_ops["v_writelane_b32"]))
    return rows, n_steady


def test_iteration_loops_reload_and_write_back_fewer_scalars_than_the_parent():
    steady, _ = _trips()                                  # (skips when the build kept no assembly)
    rows, n_steady = body_table()
    assert n_steady == len(steady)                        # the same trips as tests/test_k2_isa_loop.py finds
    assert len(rows) == BODIES, len(rows)
    seen = collections.defaultdict(list)
    for r in rows:
        print(r)
        assert r["sig"] in LAYOUTS, r                     # every body is one of the known lane layouts
        seen[r["sig"]].append(r)
    assert set(seen) == set(LAYOUTS), sorted(set(LAYOUTS) - set(seen))
    for sig, (lanes, own, parent) in LAYOUTS.items():
        assert len(seen[sig]) == len(own), (lanes, seen[sig])
        for r, (rd, wr), was in zip(seen[sig], own, parent):
            # held to the body's own totals: one reload group coming back (a 4-dword tuple, a mask pair) fails here
            assert r["readlane"] <= rd and r["writelane"] <= wr, (lanes, r, (rd, wr))
            if was is not None:                           # and every body reads back fewer scalars than the parent's did
                assert r["readlane"] < was[0], (lanes, r, was)


def test_headline_bodies_write_back_no_more_than_the_parent():
    """the bodies behind the per-wavefront table -- the headline's: the first of each layout in the file -- write no more
    scalars back than the parent's did, layout by layout.  (Behind the runs, five layouts' loops hold 8 v_writelane_b32 where
    the parent's held 4 or 6: a constant's pair in the FULL exp routine's clamps (three call sites) and the draws' mask,
    off the ordinary path; their
    reads fell from 101 .. 105 to 25 .. 45.)"""
    _trips()
    rows, _ = body_table()
    first = {}
    for r in rows:
        first.setdefault(r["sig"], r)
    for sig, (lanes, own, parent) in LAYOUTS.items():
        if parent[0] is not None:
            assert first[sig]["writelane"] <= parent[0][1], (lanes, first[sig], parent[0])


def test_recording_block_touches_no_spilled_scalar():
    _trips()
    rows, _ = body_table()
    assert sum(r["n_rec"] >= 1 for r in rows) >= BODIES - 2, rows     # (two loops are found without the block that stores)
    for r in rows:
        assert r["rec_writelane"] == 0 and r["rec_readlane"] == 0, r


if __name__ == "__main__":
    import sys
    for row in body_table(*sys.argv[1:2])[0]:
        print(row)
