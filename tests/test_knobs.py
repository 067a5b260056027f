"""CPU: the planner's MISO_* tuning knobs (miso_amd/csrc/knobs.hpp) as Knobs::from_env() reads them, seen through
miso_selftest_knobs: one NAME=value line per knob that is set.  The four kinds the planner relies on keep apart -- present
whatever the value, unset / 0 / non-zero, a number whose presence matters, a plain number -- nothing is cached between
calls, nothing else under csrc/ reads the environment, and every knob a test sets is a field of the struct."""
import glob
import os
import re

import pytest

from miso_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "miso_amd", "csrc")

# MISO_* names the tests put into the environment that are NOT the planner's: the Python front end's -- Knobs neither
# reads nor reports them.  Only a name that Python code under miso_amd/ reads itself may stand here
# (test_the_front_end_names_are_the_front_ends_own); a knob of the planner belongs into the struct, never into this list.
FRONT_END = {"MISO_AMD_LIB", "MISO_EXACT", "MISO_DISPATCH", "MISO_TEXT_DECODE", "MISO_COLLAPSED"}


def test_the_front_end_names_are_the_front_ends_own():
    py = "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "miso_amd", "*.py")))
    csrc = "".join(open(f).read() for f in glob.glob(os.path.join(CSRC, "*.h*")) + glob.glob(os.path.join(CSRC, "*.cpp")))
    for n in FRONT_END:
        assert re.search(r"[\"']%s[\"']" % n, py), n
        assert '"%s"' % n not in csrc, n


@pytest.fixture
def clean_env(monkeypatch):
    """every MISO_* name out of the environment; put back afterwards"""
    for k in list(os.environ):
        if k.startswith("MISO_"):
            monkeypatch.delenv(k)
    return monkeypatch


def test_nothing_set_nothing_reported(clean_env):
    assert capi.selftest_knobs() == {}


def test_present_whatever_the_value(clean_env):
    clean_env.setenv("MISO_NO_COOP", "0")          # "=0" still switches cooperation off
    assert capi.selftest_knobs() == {"MISO_NO_COOP": "1"}
    clean_env.setenv("MISO_NO_COOP", "")
    assert capi.selftest_knobs() == {"MISO_NO_COOP": "1"}


def test_unset_zero_and_nonzero_are_three_states(clean_env):
    seen = [capi.selftest_knobs().get("MISO_K2_MULTI")]
    for v in ("0", "1"):
        clean_env.setenv("MISO_K2_MULTI", v)
        seen.append(capi.selftest_knobs().get("MISO_K2_MULTI"))
    assert seen == [None, "0", "1"]
    clean_env.setenv("MISO_PE_LANES8", "2")        # this one has a third value
    assert capi.selftest_knobs()["MISO_PE_LANES8"] == "2"


def test_a_number_whose_presence_matters(clean_env):
    clean_env.setenv("MISO_LDS_MAX_KB", "96")
    assert capi.selftest_knobs() == {"MISO_LDS_MAX_KB": "96"}
    clean_env.setenv("MISO_LDS_MAX_KB", "80")      # the default's own value, set: still reported as set
    assert capi.selftest_knobs() == {"MISO_LDS_MAX_KB": "80"}
    clean_env.setenv("MISO_K2_TARGET", "1e12")
    assert float(capi.selftest_knobs()["MISO_K2_TARGET"]) == 1e12


def test_lists(clean_env):
    clean_env.setenv("MISO_K2_COST", "50,1,2,3,4")
    clean_env.setenv("MISO_GENERAL_LANES_BY_CLASS", "4:16,12:32")
    got = capi.selftest_knobs()
    assert [float(x) for x in got["MISO_K2_COST"].split(",")] == [50.0, 1.0, 2.0, 3.0, 4.0]
    assert got["MISO_GENERAL_LANES_BY_CLASS"] == "4:16,12:32"
    clean_env.setenv("MISO_K2_COST", "50,1")        # what parses overrides, the rest of the cost model stays
    clean_env.setenv("MISO_GENERAL_LANES_BY_CLASS", "x")
    got = capi.selftest_knobs()
    assert [float(x) for x in got["MISO_K2_COST"].split(",")] == [50.0, 1.0]
    assert got["MISO_GENERAL_LANES_BY_CLASS"] == ""  # present (the planner's default of 16 lanes for every class), no pair


def test_plain_numbers_and_their_clamps(clean_env):
    """Clamps that do not depend on the batch are from_env()'s: MISO_WAVE_SLOTS is at least 64 there, and upload() takes
    the field as it is.  (Those that do -- nc_max, count - 1, the t_32 rule -- stay where the value is used.)"""
    clean_env.setenv("MISO_WAVE_SLOTS", "8")
    clean_env.setenv("MISO_PE_SHARE", "2.5")
    clean_env.setenv("MISO_PE_T_SMALL", "0")
    clean_env.setenv("MISO_COOP_DRAWS", "100")
    clean_env.setenv("MISO_PE_ALL_ORDER", "1")     # the default's own value
    got = capi.selftest_knobs()
    assert got == {"MISO_WAVE_SLOTS": "64", "MISO_PE_SHARE": "2.5", "MISO_PE_T_SMALL": "0", "MISO_COOP_DRAWS": "256",
                   "MISO_PE_ALL_ORDER": "1"}
    clean_env.setenv("MISO_WAVE_SLOTS", "4096")
    assert capi.selftest_knobs()["MISO_WAVE_SLOTS"] == "4096"


def test_no_caching_between_calls(clean_env):
    clean_env.setenv("MISO_LANES_PER_CHAIN", "1")
    assert capi.selftest_knobs() == {"MISO_LANES_PER_CHAIN": "1"}
    clean_env.setenv("MISO_LANES_PER_CHAIN", "64")
    clean_env.setenv("MISO_NO_PE_DELTA", "1")
    assert capi.selftest_knobs() == {"MISO_LANES_PER_CHAIN": "64", "MISO_NO_PE_DELTA": "1"}
    clean_env.delenv("MISO_LANES_PER_CHAIN")
    assert capi.selftest_knobs() == {"MISO_NO_PE_DELTA": "1"}


def test_a_short_buffer_is_cut_not_overrun(clean_env):
    import ctypes
    clean_env.setenv("MISO_LANES_PER_CHAIN", "64")
    need = capi.lib().miso_selftest_knobs(None, 0)
    assert need == len("MISO_LANES_PER_CHAIN=64\n") + 1
    buf = ctypes.create_string_buffer(b"\xff" * 16, 16)
    assert capi.lib().miso_selftest_knobs(buf, 8) == need
    assert buf.raw[:8] == b"MISO_LA\0" and buf.raw[8:] == b"\xff" * 8


def test_the_environment_is_read_in_one_place():
    """under csrc/, getenv is called in knobs.hpp and in the three units the struct leaves alone: the alignment reader's
    library, the lane planner's debug line, the C ABI's load-time record of the hardware queues"""
    users = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        if path.endswith((".hip", ".cpp", ".hpp", ".inl", ".h")) and "getenv(" in open(path).read():
            users.add(os.path.basename(path))
    assert users == {"knobs.hpp", "alnio.cpp", "plan.cpp", "capi.hip"}
    # ... and the C ABI's are its load-time reads only
    capi_src = open(os.path.join(CSRC, "capi.hip")).read()
    assert set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', capi_src)) == {"MISO_HW_QUEUES_IN_EFFECT", "GPU_MAX_HW_QUEUES"}
    assert capi_src.count("getenv(") == 2


def env_names_of_the_tests():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        if os.path.abspath(path) == os.path.abspath(__file__):   # (this file's own names: the cases above)
            continue
        src = open(path).read()
        names |= set(re.findall(r"\b(MISO_[A-Z0-9_]*[A-Z0-9])=", src))              # dict(MISO_X="1"), _env(MISO_X=..)
        names |= set(re.findall(r"[\"'](MISO_[A-Z0-9_]*[A-Z0-9])[\"']", src))       # os.environ["MISO_X"], setenv("MISO_X", ..)
    return names


def test_every_knob_the_tests_set_is_a_field(clean_env):
    names = env_names_of_the_tests()
    assert len(names - FRONT_END) >= 30, sorted(names)   # (the collection found the suite's knobs at all)
    for n in names:
        clean_env.setenv(n, "1")
    got = capi.selftest_knobs()
    assert sorted(names - FRONT_END - set(got)) == []
    assert not FRONT_END & set(got)
