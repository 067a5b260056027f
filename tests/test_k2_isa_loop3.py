"""The sums of the single-end two-isoform read loop in the headline's unit as the compiler left them (CPU; reads the kept
miso_amd/csrc/.isa/kernels_k2m_m0w8.s with the loop finder and the skip rule of tests/test_k2_isa_loop.py).

A steady trip is two Philox blocks, four pairs of words.  Each pair adds its two classes to the packed counters with ONE
`v_add3_u32` and ors them into the trip's flag word with ONE `v_or3_b32` (the trip's first pair: a plain `v_or_b32` of the
two): three operations per word where a plain add and a plain or per word made four (csrc/k2_count.hpp).

Steady trips:
* 4 `v_add3_u32`, at least 3 `v_or3_b32`, and no plain `v_add_u32` besides the two block-index adds;
* `v_*` instructions: 87 (90 in the two bodies that also copy three loop-carried registers) with four operations per word;
  now 80 and 83: at most 81, and at most 83 in at most two bodies;
* no `s_nop`, no `v_cmp*`, no `v_cndmask*`;
* as many steady as masked trips: every lane layout's body has one of each."""
import collections

import test_k2_isa_loop as L


def test_steady_trips_sum_with_three_input_add_and_or():
    steady, masked = L._trips()
    assert len(steady) >= 40 and len(steady) == len(masked), (len(steady), len(masked))
    over = 0
    for c in steady:
        assert c["v_add3_u32"] == 4, dict(c)
        assert c["v_or3_b32"] >= 3, dict(c)
        assert L._count(c, "v_add_u32") <= 2, dict(c)              # the block indices of the trip's two blocks
        assert c["s_nop"] == 0 and L._count(c, "v_cmp") == 0 and L._count(c, "v_cndmask") == 0, dict(c)
        valu = L._count(c, "v_")
        assert valu <= 83, dict(c)
        over += valu > 81
    assert over <= 2, over
    print("steady trips, v_* per trip:", sorted(collections.Counter(L._count(c, "v_") for c in steady).items()))
    print("masked trips, v_* per trip:", sorted(collections.Counter(L._count(c, "v_") for c in masked).items()))
