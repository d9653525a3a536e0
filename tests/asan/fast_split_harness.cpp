// TEST-ONLY: the FAST launch ranges of liborbfe.so's planner (orbfe_fast_launches, orbslam2_amd/csrc/orbfe_plan.cpp) on the CPU under
// AddressSanitizer + UBSan.  Reads the case lines of plan_harness.cpp.  For every accepted plan and every (side_blur, blur_first)
// that run_chain can pass -- the blur of level 0 rides aside only when the pyramid's launches blur nothing, i.e. blur_first == 0 --
// prints the single launch and the split launches AS fast_cell_kernel DECODES THEM (fast_range_encode -> fast_range_decode):
//   plan NAME nlevels N cells C tiles T cut CC tcut TC min_images M
//   launches NAME side_blur S blur_first B single c0 c1 t0 t1 split K c0 c1 t0 t1 [c0 c1 t0 t1]
// tests/test_fast_split_host.py checks the sets.
#include "../../orbslam2_amd/csrc/orbfe_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static const char *k_knobs[] = {"ORBFE_NO_INPLACE", "ORBFE_NO_PAIR", "ORBFE_NO_TAIL", "ORBFE_PYR_LDS", "ORBFE_NO_FUSE", "ORBFE_NO_PROC_ORDER",
                                "ORBFE_OCTREE", "ORBFE_BLUR_RIDE_FROM", "ORBFE_HOST_TRACE", "ORBFE_FAST_SPLIT"};

static int g_bad = 0;
static void decoded(const DeviceConfig &c, const FastRange &r)
{
    int vc = 0, vt = 0;
    if (!fast_range_encode(r.c0, r.c1, c.cells_total, &vc) || !fast_range_encode(r.t0, r.t1, c.blur_tiles_total, &vt)) { printf(" UNENCODABLE"); g_bad++; return; }
    int c0, c1, t0, t1;
    fast_range_decode(vc, c.cells_total, c0, c1);
    fast_range_decode(vt, c.blur_tiles_total, t0, t1);
    printf(" %d %d %d %d", c0, c1, t0, t1);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: fast_split_harness cases.txt\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char line[1024];
    int n_cases = 0;
    while (fgets(line, sizeof(line), f)) {
        char name[256], knobs[512];
        orbfe_params p;
        memset(&p, 0, sizeof(p));
        int max_images = 0;
        if (sscanf(line, "%255s %d %d %d %f %d %d %d %d %d %d %d %511s", name, &p.width, &p.height, &p.nfeatures, &p.scale_factor,
                   &p.nlevels, &p.ini_th_fast, &p.min_th_fast, &p.patch_size, &p.half_patch_size, &p.edge_threshold, &max_images, knobs) != 13)
            continue;
        p.max_images = max_images;
        p.fx = p.fy = 0.7f * (float)p.width; p.cx = 0.5f * (float)p.width; p.cy = 0.5f * (float)p.height; p.bf = 0.2f * (float)p.width;
        for (const char *k : k_knobs) unsetenv(k);
        if (strcmp(knobs, "-") != 0)
            for (char *kv = strtok(knobs, ","); kv; kv = strtok(nullptr, ",")) {
                char *eq = strchr(kv, '=');
                if (eq) { *eq = 0; setenv(kv, eq + 1, 1); }
            }
        HostPlan *P = new HostPlan();
        char err[512] = "";
        const int rc = orbfe_build_plan(p, max_images, PlanKnobs::from_env(), P, err, sizeof(err));
        printf("case %s rc %d\n", name, rc);
        if (rc == ORBFE_OK) {
            const DeviceConfig &c = P->cfg;
            const int nl = c.nlevels;
            printf("plan %s nlevels %d cells %d tiles %d cut %d tcut %d min_images %d ride_from %d ride_min %d fuse %d\n", name, nl, c.cells_total, c.blur_tiles_total,
                   nl >= 2 ? c.lv[1].cell_off : -1, nl >= 2 ? c.lv[1].blur_tile_off : -1, P->fast_split_min_images, P->blur_ride_from, P->blur_ride_min_images, (int)P->fuse_blur);
            for (int side_blur = 0; side_blur < 2; side_blur++)
                for (int bf = 0; bf <= (side_blur ? 0 : nl); bf++) {
                    FastRange one[2], two[2];
                    const int n1 = orbfe_fast_launches(c, false, side_blur != 0, bf, one);
                    const int n2 = orbfe_fast_launches(c, true, side_blur != 0, bf, two);
                    if (n1 != 1) { printf("VIOLATION %s single launch count %d\n", name, n1); g_bad++; }
                    printf("launches %s side_blur %d blur_first %d single", name, side_blur, bf);
                    decoded(c, one[0]);
                    printf(" split %d", n2);
                    for (int k = 0; k < n2; k++) decoded(c, two[k]);
                    printf("\n");
                }
        }
        delete P;
        n_cases++;
    }
    fclose(f);
    printf("fast split harness ok %d cases %d violations\n", n_cases, g_bad);
    return 0;
}
