"""numpy restatement of csrc/k2_count.hpp from its definition, and the cases tests/test_k2_count_host.py (the plain functions
compiled for the host) and tests/test_gpu_k2_count.py (the device's assembly statements) share.

A 16-bit half x is BELOW the high-half threshold th iff x < th and ON it iff x == th; the loop's per-half class is
c = 2 below + on.  th = 0xFFFF (and the clamped th = 65536) runs the loop one lower, as th = 0xFFFE: c = 0 is then a half of
0xFFFF, c = 1 a half of 0xFFFE, c = 2 anything else.  At that one th this module restates the header's RULE, not the
definition: the per-word cases cannot tell a wrong choice of P there.  What checks th = 0xFFFF against the definition is
tests/test_k2_count_host.py test_threshold_ffff_rule and, end to end against the checker, tests/test_gpu_k2_threshold_ends.py."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 0xFFFF
EDGE_TH = (0, 1, 2, 0x7FFF, 0x8000, 0xFFFD, 0xFFFE, 0xFFFF)
MAX_BLOCKS = 8191                 # k2_count.hpp K2_COUNT_MAX_BLOCKS
INVS = np.array([0, 0xFFFF, 0xFFFF0000, 0xFFFFFFFF], np.uint32)


def build_host(tmp_dir):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_dir), "k2_count_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "miso_amd", "csrc"),
                           os.path.join(ROOT, "tools", "k2_count_host.cpp"), "-o", exe])
    return exe


def run_host(prog, mode, words, tmp_path):
    src, dst = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    np.concatenate([np.asarray(a).astype(np.uint32, copy=False).ravel() for a in words]).tofile(src)
    subprocess.check_call([prog, mode, src, dst])
    return np.fromfile(dst, np.uint32)


def half_class(th, x):
    """c per half, from the definition"""
    th, x = np.asarray(th, np.int64), np.asarray(x, np.int64)
    the = np.minimum(th, TOP - 1)
    return (2 * (x < the) + (x == the)).astype(np.uint32)


def word_class(th, u):
    u = np.asarray(u, np.uint32)
    return half_class(th, u & np.uint32(0xFFFF)) | (half_class(th, u >> np.uint32(16)) << np.uint32(16))


def seq_expected(th, start, u, inv):
    """(acc, o) per sequence: acc the two 16-bit sums of c side by side (asserted not to carry), o the OR of c"""
    start = np.asarray(start, np.int64)
    n = len(start) - 1
    ln = np.diff(start)
    c = word_class(np.repeat(np.asarray(th, np.int64), ln), u) & ~np.asarray(inv, np.uint32)
    seg = np.repeat(np.arange(n), ln)
    lo = np.bincount(seg, weights=(c & np.uint32(0xFFFF)).astype(np.float64), minlength=n).astype(np.int64)
    hi = np.bincount(seg, weights=(c >> np.uint32(16)).astype(np.float64), minlength=n).astype(np.int64)
    assert lo.max(initial=0) < 65536 and hi.max(initial=0) < 65536
    o = np.zeros(n, np.uint32)
    for bit in (0x1, 0x2, 0x10000, 0x20000):
        o |= np.where(np.bincount(seg, weights=((c & np.uint32(bit)) != 0).astype(np.float64), minlength=n) > 0, bit, 0).astype(np.uint32)
    return (lo | (hi << 16)).astype(np.uint32), o


def near_values(th):
    """th - 2 .. th + 2 (kept inside a half) and 0, 1, 0xFFFE, 0xFFFF: nine halves per th"""
    th = np.asarray(th, np.int64)
    cols = [np.clip(th + d, 0, 0xFFFF) for d in (-2, -1, 0, 1, 2)] + [np.full_like(th, v) for v in (0, 1, 0xFFFE, 0xFFFF)]
    return np.stack(cols, axis=1)


def edge_sequences(rng):
    """(th, start, u, inv=0): every th against the halves next to it and at both ends (twelve words per th, every value in
    a low half and in a high half), then every x against EDGE_TH (two words, four halves per sequence)"""
    th_all = np.arange(65536, dtype=np.int64)
    near = near_values(th_all)                                             # [65536, 9]
    lows = np.concatenate([near, near[:, [2, 0, 4]]], axis=1)              # low halves of twelve words ...
    highs = np.concatenate([near[:, ::-1], near[:, [3, 2, 1]]], axis=1)    # ... and their high halves: the same values, turned round
    u_a = (lows | (highs << 16)).astype(np.uint32)                         # [65536, 12]
    ths, us, lens = [th_all], [u_a.ravel()], [np.full(65536, 12)]
    x = np.arange(65536, dtype=np.int64)
    for th in EDGE_TH:
        xs = rng.permutation(x)
        w = (x | (xs << 16)).astype(np.uint32).reshape(-1, 2)              # every x in a low half, every x in a high half
        ths.append(np.full(len(w), th))
        us.append(w.ravel())
        lens.append(np.full(len(w), 2))
    th = np.concatenate(ths)
    u = np.concatenate(us)
    start = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    return th.astype(np.uint32), start, u, np.zeros(len(u), np.uint32)


def random_sequences(rng, n):
    """n sequences of 2 .. 40 words (a multiple of two) with about 1 % of halves on or next to the threshold; a third of
    them at th 0, 0xFFFE, 0xFFFF; random masks"""
    ln = 2 * rng.integers(1, 21, n)
    th = rng.integers(0, 65536, n)
    pick = rng.random(n)
    th = np.where(pick < 0.1, 0, np.where(pick < 0.2, 0xFFFE, np.where(pick < 0.33, 0xFFFF, th)))
    start = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    tw = np.repeat(th, ln)
    u = rng.integers(0, 1 << 32, len(tw), dtype=np.uint64)
    for shift in (0, 16):
        hit = rng.random(len(tw)) < 0.01
        val = np.clip(tw + rng.integers(-1, 2, len(tw)), 0, 0xFFFF).astype(np.uint64)
        u = np.where(hit, (u & np.uint64(0xFFFFFFFF ^ (0xFFFF << shift))) | (val << np.uint64(shift)), u)
    inv = INVS[rng.integers(0, 4, len(tw))]
    inv = np.where(rng.random(len(tw)) < 0.7, np.uint32(0), inv)
    return th.astype(np.uint32), start, u.astype(np.uint32), inv.astype(np.uint32)
