"""The ORBFE_* environment knobs of the launch plan (orbslam2_amd/csrc/orbfe_plan.h, PlanKnobs).  tools/r05_fullsuite.sh runs the
suite with some of them set; a test that relies on a particular plan clears the ones it does not set itself."""

PLAN_KNOBS = ("ORBFE_NO_INPLACE", "ORBFE_NO_PAIR", "ORBFE_NO_TAIL", "ORBFE_PYR_LDS", "ORBFE_NO_FUSE", "ORBFE_NO_PROC_ORDER",
              "ORBFE_OCTREE", "ORBFE_BLUR_RIDE_FROM")


def clear_plan_knobs(monkeypatch, keep=()):
    for k in PLAN_KNOBS:
        if k not in keep:
            monkeypatch.delenv(k, raising=False)
