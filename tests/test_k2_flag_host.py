"""CPU: the read loop's bookkeeping functions (csrc/k2_flag.hpp) compiled for the host (tools/k2_flag_host.cpp) against the
numpy restatement of their definitions (tests/_k2_flag_ref.py): the named cases of tests/test_gpu_k2_flag.py and about 10^6
random trips; the partial block's mask for every (rem, word)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _k2_flag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("k2_flag") / "k2_flag_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "miso_amd", "csrc"),
                           os.path.join(ROOT, "tools", "k2_flag_host.cpp"), "-o", exe])
    return exe


def _run(prog, mode, words, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.asarray(a).astype(np.uint32, copy=False).ravel() for a in words]).tofile(src)
    subprocess.check_call([prog, mode, src, dst])
    return np.fromfile(dst, np.uint32)


def test_flag_read_out_on_a_million_random_trips(prog, tmp_path):
    m, k, start = R.flag_cases(np.random.default_rng(223), 50000)
    assert len(m) >= 1000000
    want_code, want_pos = R.flag_expected(m, k, start)
    n = len(start) - 1
    out = _run(prog, "flag", [[n, len(m)], start, m, k], tmp_path)
    code, pos = out[:n].astype(np.int32), out[n:]
    bad = np.nonzero(code != want_code)[0]
    assert len(bad) == 0, [(int(i), int(code[i]), int(want_code[i])) for i in bad[:5]]
    one = want_code == R.ONE
    assert one.sum() > 1000 and (want_code == R.MANY).sum() > 100
    assert np.array_equal(pos[one].astype(np.int64), want_pos[one])


def test_partial_block_mask(prog, tmp_path):
    rem, w = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(8), np.arange(4)))
    got = _run(prog, "part", [[len(rem)], rem, w], tmp_path)
    assert np.array_equal(got, R.part_inv_expected(rem, w)), (got, R.part_inv_expected(rem, w))
