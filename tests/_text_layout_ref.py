"""The `.miso` sample text by the rules of include/miso_amd.h (the miso_text_shape / miso_batch_from_miso_text comment),
in plain Python: what a body decodes to, what shape it has, and where each of its bytes lies in the device decoder's
buffers (chunk, tile, thread, span byte, byte of the 8-byte word).  Nothing here is taken from the kernels' code but the
four sizes the layout is made of."""
import re
from collections import namedtuple
from fractions import Fraction

import numpy as np

EPSI, EROW, ESCORE, ECOUNT = 1, 2, 4, 8          # include/miso_amd.h MISO_TEXT_*
WORD, SPAN, TILE = 8, 16, 4096                    # Cursor's load, one thread's bytes, one workgroup's bytes
DEFAULT_CHUNK = 64 << 20

_PLAIN = re.compile(rb"-?[0-9]+(\.[0-9]+)?\Z")
_SCORE = re.compile(rb"(-?[0-9]+(\.[0-9]+)?|nan|inf|-inf)\Z")


def lines_of(body):
    """The non-empty lines of a body; the last LF may be missing."""
    return [ln for ln in bytes(body).split(b"\n") if ln]


def psi_value(field):
    """A psi field of the fast grammar as its correctly rounded double, None for any other field: -?digits[.digits],
    at most 15 significant digits (leading zeros not counted), at most 22 decimals; all digits as an integer over
    10^decimals, the sign last ("-0.0000" is -0.0)."""
    if not _PLAIN.match(field):
        return None
    neg = field.startswith(b"-")
    whole, _, frac = field.lstrip(b"-").partition(b".")
    digits = whole + frac
    if len(digits.lstrip(b"0")) > 15 or len(frac) > 22:
        return None
    v = float(Fraction(int(digits), 10 ** len(frac)))
    return -v if neg else v


def row_status(line, K, out=None):
    """One non-empty line: the first thing wrong with it, read from the left (0: a row of K psi fields, a TAB and a log
    score).  out: a list of K slots for the values."""
    psi, tab, score = line.partition(b"\t")
    fields = psi.split(b",")
    for k, f in enumerate(fields):
        v = psi_value(f)
        if v is None:
            return EPSI
        if out is not None and k < K:
            out[k] = v
    if not tab or len(fields) != K:
        return EROW
    return 0 if _SCORE.match(score) else ESCORE


def decode(body, K, S):
    """(status, samples [S, K] or None): status is the sum of the MISO_TEXT_* bits the rows before row S earned, plus
    ECOUNT for another number of non-empty lines than S; the samples only for status 0."""
    lines = lines_of(body)
    status = 0 if len(lines) == S else ECOUNT
    samples = np.zeros((S, K), dtype=np.float64)
    for r, ln in enumerate(lines[:S]):
        vals = [0.0] * K
        status |= row_status(ln, K, vals)
        samples[r] = vals
    return status, (samples if status == 0 else None)


def shape(body):
    """(isoforms, non-empty lines): the commas before the first TAB of the first non-empty line plus one, 0 without one."""
    lines = lines_of(body)
    if not lines:
        return 0, 0
    return lines[0].split(b"\t")[0].count(b",") + 1, len(lines)


class Where(namedtuple("Where", "chunk begin aligned tiles length")):
    """One event in the decoder's buffers: its chunk, its first byte relative to the chunk's base, the 16-byte boundary
    at or before it (from which its tiles are counted), its tiles and its length."""
    __slots__ = ()

    def at(self, i):
        """(tile, thread, span byte, byte mod 8) of the event's byte i."""
        d = self.begin - self.aligned + i
        return d // TILE, (d % TILE) // SPAN, d % SPAN, (self.begin + i) % WORD


def layout(offsets, chunk_bytes=0):
    """The host's chunk rule restated: a chunk starts with an event and takes the following ones while the text from
    its first byte to theirs' end is at most C bytes (chunk_bytes <= 0: 64 MiB); the chunk's base is its first event's
    offset.  Returns ([Where per event], number of chunks)."""
    C = max(chunk_bytes if chunk_bytes > 0 else DEFAULT_CHUNK, 1)
    n = len(offsets) - 1
    out, chunks, e = [], 0, 0
    while e < n:
        last = e + 1
        while last < n and offsets[last + 1] - offsets[e] <= C:
            last += 1
        for i in range(e, last):
            begin, length = int(offsets[i] - offsets[e]), int(offsets[i + 1] - offsets[i])
            aligned = begin & ~(SPAN - 1)
            out.append(Where(chunks, begin, aligned, max(1, -(-(begin - aligned + length) // TILE)), length))
        chunks += 1
        e = last
    return out, chunks


def line_starts(body):
    """The byte indices at which a non-empty line of the body starts."""
    starts, i = [], 0
    for ln in bytes(body).split(b"\n"):
        if ln:
            starts.append(i)
        i += len(ln) + 1
    return starts
