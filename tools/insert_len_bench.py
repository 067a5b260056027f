"""Time `pe_utils --compute-insert-len` on a synthetic paired-end BAM (profiles/insert_len.txt).

Writes a coordinate-sorted BAM of --pairs read pairs (2 x --pairs records: fragments ~ N(250, 30^2), 50-bp single-M
mates, most inside exons of 1-3 kb on four chromosomes, some outside, some with an unmapped mate) and its GFF of exons,
then runs the tool once; the stage times (decode, record pass, grouping, pair pass, write) come on stderr.

    python tools/insert_len_bench.py --pairs 10000000 --dir /tmp/ilb
"""
import argparse
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

READ = 50
CHROMS = ("chr1", "chr2", "chr3", "chr4")
CHROM_LEN = 200_000_000


def reg2bin(beg, end):
    """SAM spec v1 section 5.3, vectorised."""
    end = end - 1
    out = np.zeros(len(beg), np.uint16)
    done = np.zeros(len(beg), bool)
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        hit = ~done & ((beg >> shift) == (end >> shift))
        out[hit] = base + (beg[hit] >> shift)
        done |= hit
    return out


def synth(n_pairs, seed):
    rng = np.random.default_rng(seed)
    n_exons = 40000
    ex_chrom = rng.integers(0, len(CHROMS), n_exons)
    ex_len = rng.integers(1000, 3001, n_exons)
    ex_start = np.sort(rng.choice(CHROM_LEN // 4000, n_exons, replace=False)) * 4000 + 1   # 1-based, apart
    frag = np.maximum(np.rint(rng.normal(250.0, 30.0, n_pairs)).astype(np.int64), READ + 10)
    e = rng.integers(0, n_exons, n_pairs)
    left = ex_start[e] - 1 + (rng.random(n_pairs) * (ex_len[e] - frag)).astype(np.int64)
    outside = rng.random(n_pairs) < 0.15                      # pairs between the exons
    left[outside] += 3000
    chrom = ex_chrom[e]
    right = left + frag - READ
    mate_unmapped = rng.random(n_pairs) < 0.02
    gff = ["##gff-version 3\n"] + ["%s\tbench\texon\t%d\t%d\t.\t+\t.\tID=e%d\n"
                                   % (CHROMS[ex_chrom[k]], ex_start[k], ex_start[k] + ex_len[k] - 1, k)
                                   for k in range(n_exons)]
    # records: left mates (99, or 73 with an unmapped mate) and right mates (147, or 133 unmapped)
    n = 2 * n_pairs
    ref = np.concatenate([chrom, chrom]).astype(np.int32)
    pos = np.concatenate([left, right]).astype(np.int32)
    flag = np.concatenate([np.where(mate_unmapped, 73, 99), np.where(mate_unmapped, 133, 147)]).astype(np.uint16)
    pair = np.concatenate([np.arange(n_pairs), np.arange(n_pairs)])
    order = np.lexsort((pos, ref))
    ref, pos, flag, pair = ref[order], pos[order], flag[order], pair[order]
    rec = np.zeros(n, dtype=np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"),
                                      ("bin", "<u2"), ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"),
                                      ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"), ("name", "S12"),
                                      ("cigar", "<u4")]))
    rec["bs"] = rec.itemsize - 4
    rec["ref"], rec["pos"], rec["lname"], rec["mapq"] = ref, pos, 12, 50
    rec["bin"] = reg2bin(pos.astype(np.int64), pos.astype(np.int64) + READ)
    rec["ncig"], rec["flag"] = 1, flag
    rec["nref"], rec["npos"] = ref, -1
    rec["name"] = np.char.add(b"p", np.char.zfill(pair.astype("S10"), 10))
    rec["cigar"] = (READ << 4) | 0      # (an unmapped mate keeps its CIGAR: its span is pos + 1 all the same)
    return rec, "".join(gff)


def write_bam(rec, path, threads):
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % (c, CHROM_LEN) for c in CHROMS).encode()
    head = bytearray(b"BAM\x01") + struct.pack("<i", len(text)) + text + struct.pack("<i", len(CHROMS))
    for c in CHROMS:
        head += struct.pack("<i", len(c) + 1) + c.encode() + b"\0" + struct.pack("<i", CHROM_LEN)
    raw = bytes(head) + rec.tobytes()
    step = 65280

    def block(i):
        data = raw[i:i + step]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        comp = co.compress(data) + co.flush()
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25)
                + comp + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    with ThreadPoolExecutor(threads) as pool, open(path, "wb") as out:
        for b in pool.map(block, range(0, len(raw), step)):
            out.write(b)
        out.write(block(len(raw)))   # the empty EOF block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--dir", required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    bam, gff = os.path.join(a.dir, "bench.bam"), os.path.join(a.dir, "bench_exons.gff")
    t0 = time.time()
    rec, gff_text = synth(a.pairs, a.seed)
    write_bam(rec, bam, a.threads)
    open(gff, "w").write(gff_text)
    print("wrote %s: %d records, %.0f MB, in %.1f s" % (bam, len(rec), os.path.getsize(bam) / 1e6, time.time() - t0),
          flush=True)
    from miso_amd import pe_utils
    t0 = time.time()
    pe_utils.compute_insert_len([bam], gff, os.path.join(a.dir, "out"), device=a.device)
    print("compute_insert_len: %.2f s end to end" % (time.time() - t0), flush=True)
    print(open(os.path.join(a.dir, "out", "bench.bam.insert_len")).readline().strip())


if __name__ == "__main__":
    main()
