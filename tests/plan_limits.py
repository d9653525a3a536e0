"""The limits of the launch planner (orbslam2_amd/csrc/orbfe_plan.cpp, orbfe_build_plan) as straddling pairs of geometries.

Test infrastructure: one table, LIMITS, read by tests/test_plan_limits.py (the planner itself on the CPU, through
tests/asan/plan_harness) and by tests/test_gpu_plan_limits.py (the same geometries through the HIP pipeline against the oracle), so
that the host facts and the GPU cases cannot drift apart.  A row names the predicate and its line in orbfe_plan.cpp, a geometry
just inside the limit, one just outside it (None for the sort-buffer rows, which have no far side), and what the planner must
answer for each: the quadtree plan orbfe_quadtree_plan() returns (0 / 1: bucket-pyramid kernel, node tables in LDS / HBM scratch;
2 / 3: generic kernel, node tables in LDS / HBM scratch), the sort buffer of the "largest node first" phase, per-level roots and
FAST cells where the predicate reads them -- or the text of the refusal (ORBFE_ERR_UNSUPPORTED).

All geometries: FAST 20 / 7, patch 31, edge threshold 19, scale factor 1.2 unless the geometry says otherwise.
"""
from __future__ import annotations

REFUSED_LDS = "nfeatures too large for the quadtree LDS budget"
REFUSED_CAPACITY = "nfeatures too large (keypoint capacity 65536 > 65535)"
REFUSED_SIDE = "image larger than 32767 px"


def geom(width, height, nfeatures, nlevels=1, scale_factor=1.2, knobs="-"):
    """knobs: "-" or NAME=VALUE[,NAME=VALUE] as a harness line carries them"""
    return dict(width=width, height=height, nfeatures=nfeatures, nlevels=nlevels, scale_factor=scale_factor, knobs=knobs)


def accepted(g, plan, sort_cap, n_ini=None, n_cells=None):
    return dict(geom=g, plan=plan, kernel=3 if plan < 2 else 1, sort_cap=sort_cap, n_ini=n_ini, n_cells=n_cells, refused=None)


def refused(g, text):
    return dict(geom=g, plan=None, kernel=None, sort_cap=None, n_ini=None, n_cells=None, refused=text)


def row(name, predicate, line, inside, outside, bisect=None):
    """bisect: (lo, hi) -- nfeatures values on either side between which tests/test_plan_limits.py finds the flip by bisection"""
    return dict(name=name, predicate=predicate, line=line, inside=inside, outside=outside, bisect=bisect)


LIMITS = [
    # bucket-pyramid kernel: at most 4 roots on every level
    row("roots", "n_ini <= 4", 235,
        accepted(geom(211, 72, 300), 0, 512, n_ini=[4]), accepted(geom(212, 72, 300), 2, 512, n_ini=[5])),
    row("roots_level1", "n_ini <= 4 (level 1 alone over the limit)", 235,
        accepted(geom(281, 92, 300, nlevels=2), 0, 256, n_ini=[4, 4]), accepted(geom(300, 92, 300, nlevels=2), 2, 256, n_ini=[4, 5])),
    # ... and at most 4096 FAST cells per level (the quota puts both sides on HBM node tables)
    row("cells", "n_cells <= 4096", 241,
        accepted(geom(3901, 992, 3000), 1, 4096, n_cells=[4096]), accepted(geom(3902, 992, 3000), 3, 4096, n_cells=[4128])),
    # node tables of the bucket-pyramid kernel: LDS up to 150 KB, then HBM scratch
    row("pyramid_tables", "orbfe_octree3_lds_bytes(max_nodes, sort_cap, false) > 150 * 1024", 248,
        accepted(geom(320, 240, 2377), 0, 4096), accepted(geom(320, 240, 2378), 1, 4096), bisect=(2000, 3000)),
    # node tables of the generic kernel: forced into LDS by ORBFE_OCTREE=1 (refused beyond 150 KB) ...
    row("generic_tables_forced", "orbfe_octree_lds_bytes(cfg) > 150 * 1024 under ORBFE_OCTREE=1", 259,
        accepted(geom(320, 240, 2043, knobs="ORBFE_OCTREE=1"), 2, 2048), refused(geom(320, 240, 2044, knobs="ORBFE_OCTREE=1"), REFUSED_LDS),
        bisect=(1500, 3000)),
    # ... and by default on a geometry with 8 roots: LDS, then HBM scratch
    row("generic_tables", "orbfe_octree_lds_bytes(cfg) > 150 * 1024", 258,
        accepted(geom(960, 150, 2043), 2, 2048, n_ini=[8]), accepted(geom(960, 150, 2044), 3, 4096, n_ini=[8]), bisect=(1500, 3000)),
    # 16-bit keypoint indices downstream (stereo keys, row lists, slot and order words): sel_total 65535 / 65536
    row("capacity", "sel_total > 65535", 231,
        accepted(geom(1300, 800, 65531), 1, 65536), refused(geom(1300, 800, 65532), REFUSED_CAPACITY)),
    row("capacity_8_levels", "sel_total > 65535 (8 levels)", 231,
        accepted(geom(1241, 376, 65503, nlevels=8), 1, 16384), refused(geom(1241, 376, 65504, nlevels=8), REFUSED_CAPACITY)),
    # 16-bit coordinates (octree_generic_kernel keeps node rectangles in short; x | y << 16 candidate words)
    # (481 and 535 roots: a quota below four times that ends on a full pass, far above the quota; 20000 features end in the sorted phase)
    row("width", "p.width > 32767", 230,
        accepted(geom(32767, 100, 20000, nlevels=2), 3, 16384, n_ini=[481, 535]), refused(geom(32768, 100, 20000, nlevels=2), REFUSED_SIDE)),
    row("height", "p.height > 32767", 230,
        accepted(geom(100, 32767, 3000, nlevels=2), 0, 2048, n_ini=[1, 1]), refused(geom(100, 32768, 3000, nlevels=2), REFUSED_SIDE)),
    # the sort buffer of the "largest node first" phase: every power of two the planner accepts above 4096
    row("sort_cap_8192", "orbfe_sort_cap(max_nodes)", 233, accepted(geom(420, 300, 6000), 1, 8192), None),
    row("sort_cap_16384", "orbfe_sort_cap(max_nodes)", 233, accepted(geom(600, 420, 12000), 1, 16384), None),
    row("sort_cap_32768", "orbfe_sort_cap(max_nodes)", 233, accepted(geom(800, 500, 20000), 1, 32768), None),
    row("sort_cap_65536", "orbfe_sort_cap(max_nodes)", 233, accepted(geom(1100, 640, 40000), 1, 65536), None),
]

# The sort-buffer rows above do not fill their buffers: the phase sorts the multi-point nodes it starts from, and with plain noise
# that node count is a power of four times the roots (3378, 4082, 8075 and 22712 keys for the four rows, tests/octree_passes.trace).
# These geometries start the phase from a node count between half the buffer and the quota, so the bitonic network runs at the full
# buffer size: three roots (3 * 4^6 = 12288, 3 * 4^7 = 49152 nodes), or two roots with the right quarter of the image flat
# (0.75 * 2 * 4^6 = 6144, 0.75 * 2 * 4^7 = 24576).  (geometry, sort buffer, fraction of the candidate region that carries noise)
SORT_FILL = [
    (geom(840, 450, 7500), 8192, 0.75),
    (geom(1300, 430, 15000), 16384, 1.0),
    (geom(1500, 760, 30000), 32768, 0.75),
    (geom(2560, 850, 60000), 65536, 1.0),
]


def sides(rows=None):
    """(id, row, side) of every side of every row"""
    return [("%s-%s" % (r["name"], which), r, r[which]) for r in (LIMITS if rows is None else rows) for which in ("inside", "outside")
            if r[which] is not None]


def harness_line(name, g, max_images=2):
    """the case line of tests/asan/plan_harness for a geometry"""
    return "%s %d %d %d %.9g %d 20 7 31 15 19 %d %s" % (name, g["width"], g["height"], g["nfeatures"], g["scale_factor"], g["nlevels"],
                                                         max_images, g["knobs"])


def context_args(g):
    """keyword arguments of api.Context / oracle.Extractor (minus width and height for the latter) and the knobs as a dict"""
    kw = dict(width=g["width"], height=g["height"], nfeatures=g["nfeatures"], nlevels=g["nlevels"], scale_factor=g["scale_factor"])
    knobs = dict(kv.split("=") for kv in g["knobs"].split(",")) if g["knobs"] != "-" else {}
    return kw, knobs
