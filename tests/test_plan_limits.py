"""Every switching predicate of orbfe_build_plan at the value where it flips (tests/plan_limits.LIMITS), on the planner the library
links (tests/asan/plan_harness, ASan + UBSan): the geometry just inside and the one just outside each limit get the quadtree plan,
sort buffer, roots and FAST cells -- or the refusal -- the table states; the two LDS-to-HBM thresholds are found by bisection and
must be the pinned ones.  tests/test_gpu_plan_limits.py runs the same rows on the GPU.  The three guards that the reference's 30-px
cell rule keeps from ever failing (w_cell <= 64, h_cell <= 64, cell_cap <= 4095) are shown dead by a sweep over every level size."""
import numpy as np
import pytest

from tests import plan_limits as PL
from tests.test_plan_host import run_harness

ERR_UNSUPPORTED = -5


def quadtree(stdout):
    """case name -> rc, refusal text, and the fields of the harness's "quadtree" line"""
    out = {}
    for ln in stdout.splitlines():
        t = ln.split()
        if not t:
            continue
        if t[0] == "case":
            cur = out[t[1]] = dict(rc=int(t[3]), err=None)
        elif t[0] == "err":
            cur["err"] = ln[4:]
        elif t[0] == "quadtree":
            ints = lambda s: [int(v) for v in s.split(",")]
            assert t[2::2] == ["plan", "max_nodes", "sort_cap", "n_ini", "n_cells"], ln
            out[t[1]].update(plan=int(t[3]), max_nodes=int(t[5]), sort_cap=int(t[7]), n_ini=ints(t[9]), n_cells=ints(t[11]))
    return out


def check_side(name, side, got):
    if side["refused"] is not None:
        assert (got["rc"], got["err"]) == (ERR_UNSUPPORTED, side["refused"]), (name, got)
        return
    assert got["rc"] == 0, (name, got)
    assert (got["plan"], got["sort_cap"]) == (side["plan"], side["sort_cap"]), (name, got)
    for k in ("n_ini", "n_cells"):
        assert side[k] is None or got[k] == side[k], (name, k, got)


def test_both_sides_of_every_limit(tmp_path):
    cases = PL.sides()
    assert len(cases) == 2 * len(PL.LIMITS) - sum(r["outside"] is None for r in PL.LIMITS)
    got = quadtree(run_harness([PL.harness_line(name, side["geom"]) for name, _, side in cases], tmp_path).stdout)
    assert len(got) == len(cases)
    for name, _, side in cases:
        check_side(name, side, got[name])
    assert {s["plan"] for _, _, s in cases if s["refused"] is None} == {0, 1, 2, 3}  # every plan has a row
    for r in PL.LIMITS:  # a pair differs in one parameter only, and (except the 2-level roots row, whose far side the census fixed) by one
        if r["outside"] is None:
            continue
        a, b = r["inside"]["geom"], r["outside"]["geom"]
        diff = [k for k in a if a[k] != b[k]]
        assert len(diff) == 1, r["name"]
        assert b[diff[0]] - a[diff[0]] == (19 if r["name"] == "roots_level1" else 1), r["name"]


def test_one_pixel_beyond_the_two_level_roots_row(tmp_path):
    """the inside geometry of roots_level1 is the widest with 4 roots on level 1: one more column gives 5"""
    g = dict(PL.LIMITS[1]["inside"]["geom"])
    assert PL.LIMITS[1]["name"] == "roots_level1"
    g["width"] += 1
    got = quadtree(run_harness([PL.harness_line("next", g)], tmp_path).stdout)["next"]
    assert (got["plan"], got["n_ini"]) == (2, [4, 5])


@pytest.mark.parametrize("r", [r for r in PL.LIMITS if r["bisect"]], ids=lambda r: r["name"])
def test_lds_to_hbm_thresholds_by_bisection(r, tmp_path):
    """the largest nfeatures that keeps the inside answer, found over the harness, is the pinned one"""
    def inside(nf):
        g = dict(r["inside"]["geom"], nfeatures=nf)
        got = quadtree(run_harness([PL.harness_line("probe", g)], tmp_path).stdout)["probe"]
        return got["rc"] == 0 and got["plan"] == r["inside"]["plan"]
    lo, hi = r["bisect"]
    assert inside(lo) and not inside(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if inside(mid) else (lo, mid)
    assert (lo, hi) == (r["inside"]["geom"]["nfeatures"], r["outside"]["geom"]["nfeatures"])


def test_sort_fill_geometries_are_planned_on_both_table_placements(tmp_path):
    lines, want = [], {}
    for g, cap, _ in PL.SORT_FILL:
        for plan, knobs in ((1, "-"), (3, "ORBFE_OCTREE=2")):
            name = "fill%d/%d" % (cap, plan)
            lines.append(PL.harness_line(name, dict(g, knobs=knobs)))
            want[name] = (plan, cap)
    got = quadtree(run_harness(lines, tmp_path).stdout)
    assert {n: (v["plan"], v["sort_cap"]) for n, v in got.items()} == want
    assert all(v["max_nodes"] > v["sort_cap"] // 2 for v in got.values())


# ---- the guards no geometry reaches ----
def cell_axis(n, edge, skip_margin):
    """orbfe_plan.cpp:176-200 along one axis for level sizes n (array): cells, cell size, and the largest (interior + 1) / 2 of a
    cell that gets a FAST call (skip_margin: 6 along x, 3 along y -- the reference's two different early-outs)"""
    min_b = edge - 3
    max_b = n - edge + 3
    extent = (max_b - min_b).astype(np.float32)
    n_c = (extent / np.float32(30)).astype(np.int64)
    ok = (n_c >= 1) & (max_b > min_b)
    n_c1 = np.where(ok, n_c, 1)
    cell = np.ceil(extent / n_c1.astype(np.float32)).astype(np.int64)
    half = np.zeros_like(n)
    for j in range(int(n_c1.max())):
        ini = min_b + j * cell
        mx = np.minimum(ini + cell + 6, max_b)
        inner = mx - ini - 6
        live = ok & (j < n_c1) & ~(ini >= max_b - skip_margin) & (inner > 0)
        half = np.where(live, np.maximum(half, (inner + 1) // 2), half)
    return np.where(ok, n_c, 0), np.where(ok, cell, 0), half


@pytest.mark.parametrize("edge", [19, 24])
def test_cell_size_guards_cannot_fail(edge):
    """w_cell <= 64, h_cell <= 64 and cell_cap <= 4095 (orbfe_plan.cpp:240-241) for every level width and height from 33 to 32767:
    an extent of 30 k .. 30 k + 29 px is cut into k cells, so a cell is at most 59 px (one cell of a 59-px extent).  That single
    cell ends at the border, 6 px of it are FAST's margin: 53 interior px, 27 survivors of a strict 3 x 3 NMS per axis; from two
    cells on a cell is at most 45 px.  So cell_cap is at most 27 x 27 = 729."""
    n = np.arange(33, 32768, dtype=np.int64)
    ncx, wc, hx = cell_axis(n, edge, 6)
    ncy, hc, hy = cell_axis(n, edge, 3)
    assert np.array_equal(ncx, ncy) and np.array_equal(wc, hc)
    assert wc.max() == 59 and wc.max() < 60  # at extent 59: level size 59 + 2 * edge - 6
    assert int(n[np.argmax(wc)]) == 59 + 2 * edge - 6
    print("edge %d: max w_cell %d, max cc %d" % (edge, wc.max(), int(hx.max()) * int(hy.max())))
    assert hx.max() == 27 and hy.max() == 27
    assert int(hx.max()) * int(hy.max()) <= 900  # cc = ((iw + 1) / 2) * ((ih + 1) / 2) of one cell: the two factors are independent
    assert (ncx[wc > 0] >= 1).all()
