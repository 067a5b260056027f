"""CPU: the host side of the replicate-group comparison -- samples_utils.plan_group_comparison on hand-made listings, the
`--compare-groups` command line, and capi.compare_groups without a device."""
import pytest

from miso_amd import capi, samples_utils
from miso_amd.samples_utils import plan_group_comparison


def listing(*events):
    return [tuple(e) for e in events]


def ev(name, K=2, S=100, ok=True, nbytes=1000):
    return (name, K, S, ok, nbytes)


def test_plan_masks_route_and_chunks():
    g1 = [listing(ev("a"), ev("b"), ev("c"), ev("d", S=50), ev("e", K=3), ev("f"), ev("only1")),
          listing(ev("a"), ev("c"), ev("d", S=50), ev("e", K=3), ev("f", ok=False), ev("only1")),
          listing(ev("a"), ev("b"), ev("c", S=60), ev("d", S=50), ev("e", K=3), ev("f"))]
    g2 = [listing(ev("a"), ev("b"), ev("c"), ev("d", S=50), ev("e", K=2), ev("f"), ev("only2")),
          listing(ev("a"), ev("b"), ev("c"), ev("e", K=3), ev("f"))]
    plan = plan_group_comparison(g1, g2, chunk_bytes=10 ** 9)
    # c: another S in one sample; e: another K in one sample -- exactly the shape disagreements
    assert plan["pair_route"] == ["c", "e"]
    assert plan["fallback"] == ["f"]                         # not decodable in one sample
    assert plan["pairs_of"]["c"] == [(i, j) for i in range(3) for j in range(2)]
    assert plan["pairs_of"]["f"] == [(i, j) for i in range(3) for j in range(2)]
    got = {tuple(c["names"]): (c["S"], c["present1"], c["present2"], c["K"], c["bytes"]) for c in plan["chunks"]}
    assert got == {("a",): (100, (0, 1, 2), (0, 1), [2], 5000),
                   ("b",): (100, (0, 2), (0, 1), [2], 4000),          # sample 1 of group 1 lacks b: masked out
                   ("d",): (50, (0, 1, 2), (0,), [2], 4000)}          # sample 1 of group 2 lacks d
    # events of one group only are in no pair
    everything = [n for c in plan["chunks"] for n in c["names"]] + plan["pair_route"] + plan["fallback"]
    assert sorted(everything) == ["a", "b", "c", "d", "e", "f"]


def test_plan_chunk_bounds():
    names = ["ev%03d" % i for i in range(50)]
    g1 = [listing(*[ev(n, nbytes=100 + i) for i, n in enumerate(names)]) for _ in range(3)]
    g2 = [listing(*[ev(n, nbytes=300) for n in names]) for _ in range(2)]
    per_event = [3 * (100 + i) + 2 * 300 for i in range(50)]
    bound = 5000
    plan = plan_group_comparison(g1, g2, chunk_bytes=bound)
    assert plan["pair_route"] == [] and plan["fallback"] == [] and plan["pairs_of"] == {}
    seen = []
    for k, c in enumerate(plan["chunks"]):
        assert c["present1"] == (0, 1, 2) and c["present2"] == (0, 1) and c["S"] == 100
        assert c["bytes"] == sum(per_event[names.index(n)] for n in c["names"]) <= bound
        assert len(c["K"]) == len(c["names"])
        if k + 1 < len(plan["chunks"]):                      # ... and no chunk could have taken the next event too
            nxt = plan["chunks"][k + 1]["names"][0]
            assert c["bytes"] + per_event[names.index(nxt)] > bound
        seen += c["names"]
    assert seen == names and len(plan["chunks"]) > 5
    # an event larger than the bound is a chunk of its own
    plan = plan_group_comparison([listing(ev("big", nbytes=900), ev("small", nbytes=10))],
                                 [listing(ev("big", nbytes=900), ev("small", nbytes=10))], chunk_bytes=100)
    assert [c["names"] for c in plan["chunks"]] == [["big"], ["small"]]
    # the size may be left out of a listing
    plan = plan_group_comparison([[("x", 2, 10, True)]], [[("x", 2, 10, True)]])
    assert [c["names"] for c in plan["chunks"]] == [["x"]] and plan["chunks"][0]["bytes"] == 0


def test_plan_keeps_sample_counts_apart():
    g1 = [listing(ev("a", S=100), ev("b", S=200), ev("c", S=100))]
    g2 = [listing(ev("a", S=100), ev("b", S=200), ev("c", S=100))]
    plan = plan_group_comparison(g1, g2)
    assert [(c["S"], c["names"]) for c in plan["chunks"]] == [(100, ["a", "c"]), (200, ["b"])]


def test_group_labels_default_to_base_names_and_must_not_collide():
    l1, l2 = samples_utils.group_labels(["/x/ctl1", "/x/ctl2/"], ["/y/kd1"])
    assert (l1, l2) == (["ctl1", "ctl2"], ["kd1"])
    assert samples_utils.group_labels(["/x/a", "/y/a"], ["/z/b"], ["a1", "a2"], ["b"]) == (["a1", "a2"], ["b"])
    with pytest.raises(ValueError, match="a_vs_b"):
        samples_utils.group_labels(["/x/a", "/y/a"], ["/z/b"])              # two pairs -> a_vs_b
    with pytest.raises(ValueError, match="x_vs_y"):
        samples_utils.group_labels(["/1", "/2"], ["/3"], ["x", "x"], ["y"])
    with pytest.raises(ValueError, match="2 directories and 1 labels"):
        samples_utils.group_labels(["/x/a", "/x/b"], ["/z/c"], ["only"], ["c"])
    with pytest.raises(ValueError, match="1 directories and 2 labels"):
        samples_utils.group_labels(["/x/a", "/x/b"], ["/z/c"], ["a", "b"], ["c", "d"])
    with pytest.raises(ValueError, match="no sample directory"):
        samples_utils.group_labels([], ["/z/c"])


def test_command_line_parsing(tmp_path, capsys):
    d = [str(tmp_path / n) for n in ("c1", "c2", "c3", "k1", "k2")]
    dirs1, dirs2, out, l1, l2 = samples_utils.parse_group_args([",".join(d[:3]), ",".join(d[3:]), str(tmp_path / "out")])
    assert (dirs1, dirs2, out) == (d[:3], d[3:], str(tmp_path / "out"))
    assert (l1, l2) == (["c1", "c2", "c3"], ["k1", "k2"])
    _, _, _, l1, l2 = samples_utils.parse_group_args([",".join(d[:3]), d[3], "o"], ["a,b,c", "z"])
    assert (l1, l2) == (["a", "b", "c"], ["z"])
    # errors end the run before anything is read: the directories do not even exist
    for argv, msg in ((["--compare-groups", d[0] + "," + d[1], d[3], "o", "--group-labels", "a", "z"], "2 directories and 1 labels"),
                      (["--compare-groups", str(tmp_path / "p" / "s") + "," + str(tmp_path / "q" / "s"), d[3], "o"], "s_vs_k1"),
                      (["--group-labels", "a", "b"], "--compare-groups")):
        with pytest.raises(SystemExit) as e:
            samples_utils.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err
    with pytest.raises(ValueError, match="s_vs_k1"):
        samples_utils.output_group_comparisons([str(tmp_path / "p" / "s"), str(tmp_path / "q" / "s")], [d[3]], str(tmp_path / "o"))
    assert not (tmp_path / "o").exists()


def test_compare_groups_needs_a_device():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    b = capi.Batch(36, iters=50, burn=10, lag=1, chains=1)
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.compare_groups([b], [b])
    lib = capi.lib()
    assert hasattr(lib, "miso_batch_compare_groups")
    assert lib.miso_batch_compare_groups(None, 1, None, 1, capi.C.c_double(0.3), 0, None, 0, None) != capi.MISO_SUCCESS
