"""What the compiler made of the single-end two-isoform read loop in the headline's unit (CPU; reads the assembly the build
keeps, miso_amd/csrc/.isa/kernels_k2m_m0w8.s, as tests/test_k2_isa.py does, and skips the same way when it is absent).

A trip of the read loop is a single-block loop -- a block that ends in a branch to its own label -- holding eight
`v_pk_sub_u16` (two Philox blocks of four words) and 24 `v_mad_u64_u32` (their generator); every lane layout's body has one
for the steady trips and one for the masked trips of the tail, so there are as many of the one kind as of the other.  The
masked trips carry the tail's masks: at least two more bit operations per word than the steady trips' 35 (eight `x ^ th`,
the generator's, the flag's).

Steady trips (the loop's always-taken path):
* no `v_cmp*` and no `v_cndmask*`: the trip flag is two sums (csrc/k2_flag.hpp), not a compare and a select on VCC;
* at most one `s_nop`: two words' packed operations share one asm statement (the parent: 1, 6 or 8 per trip; now 0);
* `v_*` instructions: the parent's trip had 97, and 100 in the two bodies that also copy three loop-carried registers.
  Now 96 and 99: at most 97, and at most 99 in at most two bodies."""
import collections
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "miso_amd", "csrc", ".isa", "kernels_k2m_m0w8.s")
BIT_OPS = ("v_bitop3_b32", "v_xor_b32", "v_and_b32", "v_or_b32", "v_and_or_b32", "v_or3_b32", "v_bfi_b32", "v_cndmask_b32",
           "v_not_b32", "v_xnor_b32", "v_xad_u32")


def _single_block_loops(path):
    """[[mnemonic, ...]] of every block that ends in a conditional branch to its own label"""
    out, label, ops = [], None, []
    with open(path) as f:
        for line in f:
            s = line.strip()
            m = re.match(r"(\.LBB\d+_\d+):", s)
            if m:
                label, ops = m.group(1), []
                continue
            if label is None or not s or s[0] in ";." or s.startswith("//"):
                continue
            word = s.split()
            ops.append(word[0])
            if word[0].startswith("s_cbranch"):
                if word[1].rstrip(",") == label:
                    out.append(ops)
                label = None
    return out


def _trips():
    if not os.path.exists(PATH):
        hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc on this machine and no assembly kept by a build")
        pytest.skip("the build kept no assembly of the two-isoform units (make -C miso_amd/csrc)")
    steady, masked = [], []
    for ops in _single_block_loops(PATH):
        c = collections.Counter(ops)
        if c["v_pk_sub_u16"] != 8 or c["v_mad_u64_u32"] != 24:
            continue
        bit_ops = sum(v for k, v in c.items() if k.startswith(BIT_OPS))
        (steady if bit_ops < 35 + 16 else masked).append(c)
    return steady, masked


def _count(c, prefix):
    return sum(v for k, v in c.items() if k.startswith(prefix))


def test_steady_trips_have_no_compare_no_select_and_no_padding():
    steady, masked = _trips()
    assert len(steady) >= 40 and len(steady) == len(masked), (len(steady), len(masked))     # every lane layout's body has both
    over = 0
    for c in steady:
        assert _count(c, "v_cmp") == 0 and _count(c, "v_cndmask") == 0, dict(c)
        assert c["s_nop"] <= 1, dict(c)
        valu = _count(c, "v_")
        assert valu <= 99, dict(c)
        over += valu > 97
    assert over <= 2, over
    print("steady trips, v_* per trip:", sorted(collections.Counter(_count(c, "v_") for c in steady).items()))
    print("masked trips, v_* per trip:", sorted(collections.Counter(_count(c, "v_") for c in masked).items()))
