"""Host-side facts behind tests/test_gpu_describe_align.py.

The reversed block map of describe_kernel (orbslam2_amd/csrc/orbfe_common.hpp: xcd_map_of / xcd_map_of_magic with reverse), restated
in Python as tests/test_host_divisions.py restates the magic division: every (image, block) exactly once, every image on the XCDs
it had, every XCD's images in the opposite order.  And the launch plans the GPU cases rely on, from the planner itself
(tests/asan/plan_harness.cpp): at the widths under test a three-level pyramid reads level 0 in place only without the pyramid tail."""
import itertools

from tests.test_host_divisions import magic_host, xcd_split_log2


def xcd_grid(blocks_per_unit, n_units):
    lg = xcd_split_log2(n_units)
    per_xcd = (blocks_per_unit + (1 << lg) - 1) >> lg
    side = 8 >> lg
    return per_xcd * ((n_units + side - 1) // side) * 8


def xcd_map(bid, blocks_per_unit, n_units, reverse):
    """xcd_map_of_magic: (unit, blk) of workgroup bid, or None where the kernel returns at once"""
    lg = xcd_split_log2(n_units)
    xcd, jb = bid & 7, bid >> 3
    magic, per_xcd, _ = magic_host(blocks_per_unit, n_units)
    rnd = (jb * magic) >> 32 if magic else jb // per_xcd
    assert rnd == jb // per_xcd
    ru = ((n_units + (8 >> lg) - 1) >> (3 - lg)) - 1 - rnd if reverse else rnd
    unit = ru * (8 >> lg) + (xcd >> lg)
    blk = ((jb - rnd * per_xcd) << lg) + (xcd & ((1 << lg) - 1))
    return (unit, blk) if unit < n_units and blk < blocks_per_unit else None


def test_reversed_map_visits_every_block_once_in_the_opposite_image_order():
    for n, bpu in itertools.product(list(range(1, 18)) + [64, 128], (1, 2, 3, 7, 19, 128)):
        grid = xcd_grid(bpu, n)
        fwd = [xcd_map(b, bpu, n, False) for b in range(grid)]
        rev = [xcd_map(b, bpu, n, True) for b in range(grid)]
        want = sorted((u, k) for u in range(n) for k in range(bpu))
        assert sorted(x for x in fwd if x) == want and sorted(x for x in rev if x) == want, (n, bpu)
        for xcd in range(8):
            f = [x for x in fwd[xcd::8] if x]
            r = [x for x in rev[xcd::8] if x]
            # the same images on this XCD, taken in the opposite order, each image's blocks in their own order
            fu, ru = [u for u, _ in f], [u for u, _ in r]
            assert sorted(set(fu)) == sorted(set(ru)), (n, bpu, xcd)
            assert list(dict.fromkeys(ru)) == list(dict.fromkeys(fu))[::-1], (n, bpu, xcd)
            assert fu == sorted(fu) and ru == sorted(ru, reverse=True), (n, bpu, xcd)
            for u in set(fu):
                assert [k for v, k in f if v == u] == [k for v, k in r if v == u], (n, bpu, xcd, u)


def test_plans_of_the_describe_align_cases(tmp_path):
    from tests.test_gpu_describe_align import H, NF, NL, PLANS, WIDTHS
    from tests.test_plan_host import _line, facts, run_harness
    knob_sets = {"default": "-"}
    knob_sets.update({name: ",".join("%s=%s" % kv for kv in env.items()) for name, env in PLANS.items()})
    lines = [_line("w%d/%s" % (w, name), w, H, NF, nl=NL, knobs=ks, mi=9) for w in WIDTHS for name, ks in knob_sets.items()]
    f = facts(run_harness(lines, tmp_path).stdout)
    for w in WIDTHS:
        assert f["w%d/default" % w]["tail_first"] == 1 and f["w%d/default" % w]["inplace_ok"] == 0  # the tail reads a copied level 0
        assert f["w%d/in_place" % w]["inplace_ok"] == 1 and f["w%d/in_place" % w]["levels"][1][0] == 1
        assert f["w%d/pitched" % w]["inplace_ok"] == 0
