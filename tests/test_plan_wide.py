"""The planner accepts the geometries that neither the bucket-pyramid quadtree kernel nor the generic kernel's LDS node tables
fit (more than 4 roots or more than 4096 FAST cells per level, and a per-level quota beyond ~1800 nodes): the generic kernel then
keeps its node tables in HBM scratch.  Run on the CPU under AddressSanitizer + UBSan by tests/asan/plan_harness.cpp, like
tests/test_plan_host.py; ORBFE_OCTREE=2 forces that form for any geometry, ORBFE_OCTREE=1 keeps the LDS form and its refusal."""
from tests.test_plan_host import MAX_IMAGES, _line, blocks, run_harness

# name, width, height, nfeatures, levels: refused ("nfeatures too large for the quadtree LDS budget") before the HBM node tables
WIDE = [("uhd12k", 3840, 2160, 12000, 8),      # 126 x 70 FAST cells at level 0
        ("pano8_10k", 4096, 512, 10000, 8),    # 8 to 9 roots
        ("strip2048", 2048, 256, 10000, 8),    # 9 roots
        ("strip1600", 1600, 200, 2500, 1),     # 9 roots
        ("strip960", 960, 150, 2200, 1)]       # 8 roots
REFUSAL = "err nfeatures too large for the quadtree LDS budget"
HBM_TRACE = "orbfe: generic quadtree kernel: node tables in HBM scratch, "


def _hbm_lines(stderr):
    return [ln for ln in stderr.splitlines() if ln.startswith(HBM_TRACE)]


def test_wide_geometries_are_planned_at_every_batch_size(tmp_path):
    lines = [_line("%s/m%d" % (n, mi), w, h, nf, nl=nl, mi=mi) for n, w, h, nf, nl in WIDE for mi in MAX_IMAGES]
    got = blocks(run_harness(lines, tmp_path).stdout)
    assert len(got) == len(WIDE) * len(MAX_IMAGES)
    for name, b in got.items():
        assert b[0] == "case %s rc 0" % name, b[:2]
        assert b[3].split()[1] == "0", b[3]  # flags: not the bucket-pyramid kernel


def test_wide_geometries_take_the_hbm_node_tables(tmp_path):
    """The trace line of the HBM form appears for exactly the plans that choose it, with the scratch bytes per image."""
    names = [n for n, *_ in WIDE]
    lines = [_line(n, w, h, nf, nl=nl, knobs="ORBFE_HOST_TRACE=1") for n, w, h, nf, nl in WIDE]
    r = run_harness(lines, tmp_path)
    hbm = _hbm_lines(r.stderr)
    assert len(hbm) == len(names), r.stderr[-2000:]
    for ln in hbm:
        assert int(ln[len(HBM_TRACE):].split()[0]) > 150 * 1024 and ln.endswith(" bytes per image"), ln
    # plans that fit LDS (or the bucket-pyramid kernel) print no such line
    r = run_harness([_line("uhd8k", 3840, 2160, 8000, knobs="ORBFE_HOST_TRACE=1"), _line("kitti", 1241, 376, 2000, knobs="ORBFE_HOST_TRACE=1"),
                     _line("kitti_lds", 1241, 376, 2000, knobs="ORBFE_HOST_TRACE=1,ORBFE_OCTREE=1")], tmp_path)
    assert _hbm_lines(r.stderr) == []


def test_octree_knob_values(tmp_path):
    small = dict(w=640, h=480, nf=2500, nl=1)
    lines = [_line("forced_hbm", knobs="ORBFE_OCTREE=2", **small), _line("forced_lds", knobs="ORBFE_OCTREE=1", **small),
             _line("default", **small), _line("forced_hbm_trace", knobs="ORBFE_OCTREE=2,ORBFE_HOST_TRACE=1", **small),
             _line("kitti_hbm", 1241, 376, 2000, knobs="ORBFE_OCTREE=2,ORBFE_HOST_TRACE=1"), _line("kitti", 1241, 376, 2000)]
    r = run_harness(lines, tmp_path)
    got = blocks(r.stdout)
    assert got["forced_hbm"][0].endswith("rc 0") and got["forced_hbm"][3].split()[1] == "0"
    assert got["forced_lds"] == ["case forced_lds rc -5", REFUSAL]  # today's refusal, today's text
    assert got["default"][0].endswith("rc 0") and got["default"][3].split()[1] == "1"  # the bucket-pyramid kernel owns this shape
    assert len(_hbm_lines(r.stderr)) == 2  # forced_hbm_trace, kitti_hbm
    # the knob changes the quadtree kernel and nothing else: config bytes and every table but the flags line are the default plan's
    assert got["kitti_hbm"][3].split()[1] == "0" and got["kitti"][3].split()[1] == "1"
    strip = lambda b: [ln for ln in b[1:] if not ln.startswith(("flags", "cfg"))]
    assert strip(got["kitti_hbm"]) == strip(got["kitti"])


def test_lds_plans_of_large_geometries_are_unchanged(tmp_path):
    got = blocks(run_harness([_line("uhd8k", 3840, 2160, 8000), _line("pano8_9k", 4096, 512, 9000)], tmp_path).stdout)
    assert got["uhd8k"][0].endswith("rc 0") and got["uhd8k"][3].startswith("flags 0 109456 0 2048 ")
    assert got["pano8_9k"][0].endswith("rc 0") and got["pano8_9k"][3].startswith("flags 0 121488 0 2048 ")
