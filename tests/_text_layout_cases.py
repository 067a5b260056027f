"""Sample text planted on the device decoder's four granularities (csrc/kernels_text.hip): the 8-byte word of its
cursor, the 16-byte span of a thread, the 4096-byte tile of a workgroup, the chunk of whole events.

A family is a list of event bodies with one sample count S (a batch has one n_samples), the isoform count to pass for
each, and `marks`: the bytes a case was built around, as (event, byte index, the byte, (tile, thread, span byte)) with the
coordinates that hold when the family is decoded as ONE chunk.  Everything is placed by arithmetic on field lengths:
decimals pad a field byte by byte, a row's length is the sum of its fields, an event's length sets the next event's
phase.  tests/test_text_layout_cases.py shows that the cases are what they claim; tests/test_gpu_text_layout.py runs them.
"""
from collections import namedtuple

from _text_layout_ref import EPSI, EROW, ESCORE, SPAN, TILE

Family = namedtuple("Family", "name S bodies K prefix marks")

SCORES = [b"nan", b"inf", b"-inf", b"1234.5", b"-123456.78"]      # three literals, a plain and a negative decimal
LONGEST_SCORE = max(len(s) for s in SCORES)


def field(n, v):
    """A psi field of exactly n bytes (1 .. 24) of the fast grammar, its digits taken from v: n <= 2 digits alone,
    else `0.` and n - 2 decimals, of which at most the last 15 are significant."""
    assert 1 <= n <= 24
    if n <= 2:
        return b"%0*d" % (n, v % 10 ** n)
    d = n - 2
    sig = min(d, 15)
    return b"0." + b"0" * (d - sig) + b"%0*d" % (sig, v % 10 ** sig)


def mix(i):
    """Distinct digits for the i-th field (Knuth's multiplicative hash, 15 digits)."""
    return (i + 1) * 2654435761 * 1000003 % 10 ** 15


def row(L, K, score, v0, lf=True):
    """A row of exactly L bytes, the LF counted: K fields of near-equal length, a TAB, the score."""
    F = L - (K + 1) - len(score)
    assert K <= F <= 24 * K, (L, K, score)
    base, extra = divmod(F, K)
    psi = b",".join(field(base + (k < extra), mix(v0 + k)) for k in range(K))
    out = psi + b"\t" + score + (b"\n" if lf else b"")
    assert len(out) == (L if lf else L - 1)
    return out


def split(total, n):
    """n near-equal lengths that sum to total."""
    base, extra = divmod(total, n)
    return [base + (i < extra) for i in range(n)]


def rows(lengths, K, v0, score0=0, scores=None):
    """Rows of the given lengths; row j's score is scores[j] if given, else SCORES in turn from score0."""
    return b"".join(row(L, K, (scores or {}).get(j, SCORES[(score0 + j) % len(SCORES)]), v0 + j * K)
                    for j, L in enumerate(lengths))


def psi_bytes(L, K, score):
    """The bytes before the TAB in row(L, K, score, .)."""
    return L - 2 - len(score)


# ---- phases: every begin phase x every span byte of the second line start; `-inf` at every byte of the word ----
def phase_bodies():
    bodies, pos = [], 0
    order = [(p, L1) for p in range(SPAN) for L1 in range(17, 33)]
    for i, (p, L1) in enumerate(order):
        assert pos % SPAN == p
        nxt = order[i + 1][0] if i + 1 < len(order) else 0
        L2 = 17 + (5 * i) % 16
        L3 = 17 + (nxt - (pos + L1 + L2 + 17)) % SPAN
        bodies.append(rows([L1, L2, L3], 2, 6 * i, score0=3 * i + i // 5))
        pos += len(bodies[-1])
    return bodies


def phases():
    b = phase_bodies()
    return Family("phases", 3, b, [2] * len(b), b"", {})


# two header lines that would decode as rows of two isoforms if they were taken for text of the first event
PREFIX = b"0.125,0.875\t-1.5\n0.1875,0.8125\t-2.25\n"


def prefix():
    b = phase_bodies()
    assert len(PREFIX) == 37
    return Family("prefix", 3, b, [2] * len(b), PREFIX, {})


# ---- tile_edges: one event of four tiles per variant, one byte planted on a tile's last or first byte ----
def tile_edges():
    K, S, Lr = 5, 160, 100
    bodies, marks, pos = [], [], 0
    # (name, score of the planted row, which byte of that row goes to `where` relative to the tile boundary B)
    variants = [("lf_last_start_first", b"nan", "start", 0), ("start_last", b"inf", "start", -1),
                ("tab_last", b"1234.5", "tab", -1), ("minus_inf_1_3", b"-inf", "minus", -1),
                ("minus_inf_2_2", b"-inf", "minus", -2), ("minus_inf_3_1", b"-inf", "minus", -3)]
    for n, (name, score, what, where) in enumerate(variants):
        ph = pos % SPAN
        b = 1 + n % 3                                   # the boundary between tile b - 1 and tile b
        B = TILE * b - ph                               # the event's byte that is tile b's byte 0
        T = 4 * TILE - ph - 100 - 17 * n                # the event's length: four tiles
        in_row = {"start": 0, "tab": psi_bytes(Lr, K, score), "minus": psi_bytes(Lr, K, score) + 1}[what]
        P = B + where - in_row                          # where the planted row starts
        r = S * P // T
        body = rows(split(P, r) + [Lr] + split(T - P - Lr, S - r - 1), K, 1000 * n, score0=n, scores={r: score})
        assert len(body) == T
        e = len(bodies)
        at = B + where
        if what == "start":
            marks.append((name, e, at - 1, b"\n", ((at - 1 + ph) // TILE, (at - 1 + ph) % TILE // SPAN, (at - 1 + ph) % SPAN)))
            marks.append((name, e, at, b"0", ((at + ph) // TILE, (at + ph) % TILE // SPAN, (at + ph) % SPAN)))
        else:
            marks.append((name, e, at, {"tab": b"\t", "minus": b"-"}[what], (b - 1, 255, SPAN + where)))
        bodies.append(body)
        pos += T
    return Family("tile_edges", S, bodies, [K] * len(bodies), b"", {"bytes": marks})


# ---- long_rows: rows longer than a tile ----
def long_rows():
    K, S = 256, 3
    L = K * 24 + K + len(b"-123456.78") + 1             # 256 fields of 24 bytes: 22 decimals, 15 significant digits
    long_event = rows([L] * S, K, 0, scores={0: b"-123456.78", 1: b"-123456.78", 2: b"-123456.78"})
    short_event = rows([K + K + 4] * S, K, 5000, scores={0: b"nan", 1: b"inf", 2: b"1.5"})      # one-byte fields
    filler = rows([21, 22, 23], 2, 9000)
    bodies = [filler, long_event, short_event, long_event]
    return Family("long_rows", S, bodies, [2, K, K, K], b"", {})


# ---- tile_counts: events of exactly 63, 64, 65, 128 and 129 tiles (the scan's carry after 64 tiles) ----
TILE_COUNTS = [63, 64, 65, 128, 129]


def tile_counts():
    K, S = 20, 1100
    # what the last tile holds: a part, all 4096 bytes, the final LF alone, half, seven bytes
    in_last = [TILE - 1000, TILE, 1, TILE // 2, 7]
    bodies, pos = [], 0
    for n, (tiles, last) in enumerate(zip(TILE_COUNTS, in_last)):
        ph = pos % SPAN
        T = TILE * (tiles - 1) + last - ph
        bodies.append(rows(split(T, S), K, 100000 * n, score0=n))
        assert len(bodies[-1]) == T
        pos += T
    return Family("tile_counts", S, bodies, [K] * len(bodies), b"", {})


# ---- tiny: events shorter than a span, empty events and events of LFs only between them ----
TINY_LENGTHS = [4, 4, 4, 5, 5, 6, 15, 7, 4, 4, 8, 9, 10, 4, 11, 12, 13, 14]
TINY_EMPTY = {3: b"", 28: b"", 29: b"", 10: b"\n", 20: b"\n\n", 30: b"\n" * 17, 78: b"", 103: b"\n", 153: b"", 199: b""}
TINY_NO_LF = {7, 32, 57, 58, 82, 107, 132, 157, 182}


def tiny():
    bodies = []
    for i in range(200):
        if i in TINY_EMPTY:
            bodies.append(TINY_EMPTY[i])
            continue
        L = TINY_LENGTHS[i % len(TINY_LENGTHS)]
        score = [b"0", b"-1", b"nan", b"inf", b"-inf", b"-1.50"][i % 6]
        if len(score) > L - 3:
            score = b"0"
        bodies.append(row(L, 1, score, i, lf=i not in TINY_NO_LF))
    return Family("tiny", 1, bodies, [1] * len(bodies), b"", {"empty": sorted(TINY_EMPTY), "no_lf": sorted(TINY_NO_LF)})


# ---- ends: a row cut off at the event's end must not read on into the next event ----
# (the cut last row, the first bytes of the next event, that event's isoforms, the cut event's status)
ENDS = [(b"0.5,0.", b"7,", 2, EPSI),               # read on: 0.5,0.7,...
        (b"0.5,0", b"5,", 2, EROW),                # read on: 0.5,05,...
        (b"0.5,0.5\t", b"1", 2, ESCORE),
        (b"0.5,0.5\t-", b"1", 2, ESCORE),
        (b"0.5,0.5\t-in", b"7", 2, ESCORE),
        (b"0.5,0.5\t-1", b"25,", 2, 0),            # the last LF missing; read on: a score -125 and then a comma
        (b"0.5,0.5\t-1.5", b"-", 2, 0),            # a full last row without LF, then a sign
        (b"0.5,0.", b"7\t", 1, EPSI),              # read on: a whole row 0.5,0.7<TAB>score, silently
        (b"0.5,0", b"5\t", 1, EROW)]               # read on: a whole row 0.5,05<TAB>score, silently
ENDS_S = 3


def cut_event(cut, shift, v0):
    """Two whole rows of two isoforms, the first padded by `shift` bytes (the cut then stands at another byte of the
    word), and the cut row."""
    return rows([24 + shift, 21], 2, v0, score0=v0) + cut


def after_cut(first, K, v0):
    """A valid event of ENDS_S rows that begins with the bytes `first`."""
    if first.endswith(b"\t"):
        head = first + b"-2.5\n"
    elif first.endswith(b","):
        head = first + b"0.375\t-2.5\n"
    else:
        head = first + (b".5,0.625\t-3\n" if first[-1:].isdigit() else b"0.5,0.625\t-3\n")
    assert head.split(b"\t")[0].count(b",") + 1 == K
    return head + rows([20 + K, 22 + K], K, v0, score0=v0 + 1)


def ends():
    bodies, Ks, pairs, pos = [], [], [], 0
    for byte in range(8):                               # the cut event ends at this byte of the 8-byte word
        for n, (cut, first, K, status) in enumerate(ENDS):
            pairs.append((len(bodies), first, status))
            shift = (byte - (pos + len(cut_event(cut, 0, 0)))) % 8
            bodies += [cut_event(cut, shift, 40 * byte + 4 * n), after_cut(first, K, 40 * byte + 4 * n + 2)]
            Ks += [2, K]
            pos += len(bodies[-2]) + len(bodies[-1])
    return Family("ends", ENDS_S, bodies, Ks, b"", {"pairs": pairs})


def ends_last():
    """The same cut rows as the last bytes of the whole text: only the buffer's padding follows."""
    fams = []
    for n, (cut, _, _, status) in enumerate(ENDS[:7]):
        bodies = [after_cut(b"7,", 2, 4 * n), cut_event(cut, n, 4 * n + 2)]
        fams.append(Family("ends_last_%d" % n, ENDS_S, bodies, [2, 2], b"", {"pairs": [(1, None, status)]}))
    return fams


# ---- blank_lines: empty lines are ignored wherever they stand ----
def blank_lines():
    K, S, L = 20, 12, 408
    bodies, marks, pos = [], [], 0

    def lines(lengths, v0):
        return [row(n, K, SCORES[(v0 + j) % len(SCORES)], v0 + j * K) for j, n in enumerate(lengths)]

    def add(name, body, run=None):
        nonlocal pos
        if run is not None:
            marks.append((name, len(bodies), run[0], run[1]))
        bodies.append(body)
        pos += len(body)

    plain = lines([L] * S, 0)
    add("none", b"".join(plain))
    add("leading", b"\n" + b"".join(plain))
    add("leading_two", b"\n\n" + b"".join(plain))
    add("interior", b"".join(plain[:3]) + b"\n" + b"".join(plain[3:7]) + b"\n\n\n" + b"".join(plain[7:]))
    add("trailing", b"".join(plain) + b"\n\n")
    add("doubled", b"".join(r + b"\n" for r in plain))
    add("no_final_lf", b"\n" + b"".join(r + b"\n" for r in plain)[:-2])
    # 20 LFs that begin at span byte 14: they touch three threads, and the one in the middle sees nothing else
    head = 2 * L + (14 - (pos + 2 * L)) % SPAN
    ls = lines(split(head, 2) + [L] * (S - 2), 500)
    add("span_run", b"".join(ls[:2]) + b"\n" * 20 + b"".join(ls[2:]), run=(head, 20))
    # 20 LFs over the first tile boundary of the event: ten on either side
    head = TILE - pos % SPAN - 10
    ls = lines(split(head, 10) + [L] * (S - 10), 900)
    add("tile_run", b"".join(ls[:10]) + b"\n" * 20 + b"".join(ls[10:]), run=(head, 20))
    return Family("blank_lines", S, bodies, [K] * len(bodies), b"", {"runs": marks})


def strip_blank(body):
    """The same rows without the empty lines, every row LF-terminated."""
    return b"".join(ln + b"\n" for ln in body.split(b"\n") if ln)


_CACHE = {}


def families():
    """Every family by name, built once."""
    if not _CACHE:
        for f in [phases(), tile_edges(), long_rows(), tile_counts(), tiny(), ends(), blank_lines(), prefix()] + ends_last():
            _CACHE[f.name] = f
    return _CACHE


_REFERENCE = {}


def reference(fam):
    """[(status, samples or None)] of the family's events by tests/_text_layout_ref.py, computed once and never changed."""
    if fam.name not in _REFERENCE:
        from _text_layout_ref import decode
        out = [decode(b, K, fam.S) for b, K in zip(fam.bodies, fam.K)]
        for _, s in out:
            if s is not None:
                s.setflags(write=False)
        _REFERENCE[fam.name] = out
    return _REFERENCE[fam.name]


def offsets_of(fam):
    offs = [len(fam.prefix)]
    for b in fam.bodies:
        offs.append(offs[-1] + len(b))
    return offs
