"""The model check's class table on the host: miso_batch_set_model_check + miso_batch_add_event +
miso_batch_model_check_table.  No GPU.  miso_gene_assignment_matrix is the authority for classes and their order."""
import numpy as np
import pytest

from miso_amd import capi

GENE = ([(1, 100), (201, 250), (351, 450)], [(0, 1, 2), (0, 2)])
# read length 36, overhang 1, by hand: starts 66..100 of exon 1 on the skipping junction = 35 -> (0,1); starts 66..100 on the
# inclusion junction + 201..250 (exon 2 and its junction to exon 3) = 85 -> (1,0); starts 1..65 and 351..415 = 130 -> (1,1)
BY_HAND = [((0, 1), 35), ((1, 0), 85), ((1, 1), 130)]
READ = {(1, 1): (1, "36M"), (1, 0): (205, "36M"), (0, 1): (80, "21M250N15M"), "none": (120, "36M")}


def _key(pattern, K):
    return tuple((int(pattern) >> k) & 1 for k in range(K))


def _table_as_matrix(t, K):
    return np.array([[m if (int(p) >> k) & 1 else 0 for k in range(K)] for p, m in zip(t["pattern"], t["m"])], dtype=np.float64)


def test_the_gene_by_hand_and_by_the_assignment_matrix():
    g = capi.Gene(*GENE)
    b = capi.Batch(36, model_check=True)
    b.add_event(g, [1], ["36M"])
    t = b.model_check_table(0)
    assert t["status"] == "ok"
    assert [(_key(p, 2), int(m)) for p, m in zip(t["pattern"], t["m"])] == BY_HAND
    assert np.array_equal(_table_as_matrix(t, 2), g.assignment_matrix(36))
    # every isoform's classes add up to its effective length (250 - 36 + 1, 200 - 36 + 1)
    assert list(_table_as_matrix(t, 2).sum(0)) == [215.0, 165.0]


def test_planted_reads_are_counted_by_class():
    g = capi.Gene(*GENE)
    b = capi.Batch(36, model_check=True)
    pos, cig = [], []
    for key, count in (((0, 1), 3), ((1, 0), 5), ((1, 1), 7), ("none", 1)):
        pos += [READ[key][0]] * count
        cig += [READ[key][1]] * count
    b.add_event(g, pos, cig)
    t = b.model_check_table(0)
    assert list(t["n"]) == [3, 5, 7] and t["num_reads"] == 15 and t["num_off_model"] == 0


def test_reads_the_positions_cannot_produce():
    """num_off_model counts the reads whose non-empty pattern is no column.  Through miso_batch_add_event no such read can be
    planted today, and this test pins why: the matcher (csrc/host.cpp match_iso) uses a read only if its CIGAR covers the
    read length, and clips it to the read length -- so a usable read IS a window of read-length bases at its position, and
    its pattern is that window's class.  Isoform B is one exon [1001, 1200]; A shares its first 120 bases, C its last 121;
    every window of 36 inside B lies on A or C as well, so (0,1,0) is no class.  A read of 100 aligned bases in the middle
    would lie on B alone -- it is clipped to its first 36 and counted with (1,1,0).  Soft clips and deletions count as
    covered bases likewise; a read shorter than the read length and a read in an intron are compatible with no isoform
    and are in neither N nor num_off_model."""
    g = capi.Gene([(1, 100), (1001, 1120), (1301, 1400), (1001, 1200), (1080, 1200)], [(1, 2), (3,), (0, 4)])
    cols = g.assignment_matrix(36)
    assert not any(tuple(row > 0) == (False, True, False) for row in cols)
    b = capi.Batch(36, model_check=True)
    pos = [1050, 1010, 1100, 1100, 1100, 500, 1010]
    cig = ["100M", "36M", "5S31M", "20M5D11M", "36M", "36M", "20M"]
    assert tuple(g.match_iso([1050], ["100M"], 36)[0]) == (1.0, 1.0, 0.0)
    b.add_event(g, pos, cig)
    t = b.model_check_table(0)
    by_key = {_key(p, 3): int(n) for p, n in zip(t["pattern"], t["n"]) if n}
    assert by_key == {(1, 1, 0): 2, (0, 1, 1): 3}
    assert t["num_reads"] == 5 and t["num_off_model"] == 0


def test_three_isoforms_in_the_matrix_column_order():
    g = capi.Gene([(1, 100), (201, 250), (351, 450), (551, 650)], [(0, 1, 2, 3), (0, 2, 3), (0, 3)])
    b = capi.Batch(36, model_check=True)
    b.add_event(g, [1, 560, 360], ["36M", "36M", "36M"])
    t = b.model_check_table(0)
    want = g.assignment_matrix(36)
    assert len(want) >= 5 and np.array_equal(_table_as_matrix(t, 3), want)
    by_key = {_key(p, 3): int(n) for p, n in zip(t["pattern"], t["n"])}
    assert by_key[(1, 1, 1)] == 2 and by_key[(1, 1, 0)] == 1 and t["num_reads"] == 3


def test_guards():
    with pytest.raises(capi.InternalError):
        capi.Batch(36, paired=True, mean=250.0, var=900.0, model_check=True)        # MISO_EINVAL
    with pytest.raises(NotImplementedError):
        capi.Batch(36, overhang=2, model_check=True)                                # the matrix's own limit
    b = capi.Batch(36, model_check=True)
    b.add_problem(np.array([[1.0, 0.0], [1.0, 1.0]]), [250, 200], [3, 2])
    t = b.model_check_table(0)
    assert t["status"] == "no_gene" and len(t["n"]) == 0 and t["num_reads"] == 0
    off = capi.Batch(36)
    off.add_event(capi.Gene(*GENE), [1], ["36M"])
    with pytest.raises(capi.InternalError):
        off.model_check_table(0)


def test_the_raw_call_has_no_cpu_path():
    if capi.device_count() > 0:       # (with a device the call runs: tests/test_gpu_model_check.py)
        return
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.model_check([2], [[2, 1, 3]], [[35, 85, 130]], [[1, 1, 1]], [np.full((4, 2), 0.5)])
