// TEST-ONLY: the launch planner of liborbfe.so (orbslam2_amd/csrc/orbfe_plan.cpp, the translation unit the library links) on
// the CPU under AddressSanitizer + UBSan.  Reads cases, one per line:
//   name width height nfeatures scale_factor nlevels ini_th min_th patch_size half_patch edge_threshold max_images knobs
// (knobs: "-" or NAME=VALUE,NAME=VALUE of the ORBFE_* environment knobs, set before PlanKnobs::from_env()).  Prints per case
// the status and FNV-1a digests of the config, the per-level tables and every named device table (tests/test_plan_host.py
// compares them with tests/golden/plan_digests.json), a "facts" line with the launch choices of an accepted plan (tail, pair and
// ride thresholds, level 0 in place, per level rs_direct / rs_rw / pp_ok), a "quadtree" line (the plan number orbfe_quadtree_plan()
// returns, max_nodes, the sort buffer, per level n_ini and n_cells), and a VIOLATION line for every coverage invariant an
// accepted plan breaks.
// --dump NAME[,NAME]: also print those tables' words (cell_info, cell_aux).
#include "../../orbslam2_amd/csrc/orbfe_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static const char *k_knobs[] = {"ORBFE_NO_INPLACE", "ORBFE_NO_PAIR", "ORBFE_NO_TAIL", "ORBFE_PYR_LDS", "ORBFE_NO_FUSE",
                                "ORBFE_NO_PROC_ORDER", "ORBFE_OCTREE", "ORBFE_BLUR_RIDE_FROM", "ORBFE_HOST_TRACE"};

static unsigned long long fnv(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    const unsigned char *b = (const unsigned char *)data;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
template <typename T> static void tab(const char *name, const std::vector<T> &v)
{
    printf("tab %s %zu %016llx\n", name, v.size() * sizeof(T), fnv(v.data(), v.size() * sizeof(T)));
}

static int g_bad = 0;
static void violation(const char *cs, const char *what, int l)
{
    printf("VIOLATION %s %s level %d\n", cs, what, l);
    g_bad++;
}

// the invariants the planner's comments state
static void check(const char *cs, const orbfe_params &p, const HostPlan &P)
{
    const DeviceConfig &c = P.cfg;
    int cell = 0, cand = 0, sel = 0, part = 0;
    for (int l = 0; l < c.nlevels; l++) { // per-image ranges follow each other and add up to the totals
        const LevelInfo &L = c.lv[l];
        if (L.cell_off != cell || L.cand_off != cand || L.sel_off != sel) violation(cs, "offsets", l);
        cell += L.n_cells; cand += (L.cand_cap + 3) & ~3; sel += L.sel_cap;
        if (L.bk_part_off != part || L.bk_part_off % 4 || L.bk_part_n % 4) violation(cs, "bk_emap alignment", l); // 16-byte quads
        part += L.bk_part_n;
        if (l > 0 && (L.rs_xtab_off % 4 || L.rs_xtab_n % 4)) violation(cs, "rs_tab alignment", l);
    }
    if (c.cells_total != (cell > 0 ? cell : 1) || c.cand_total != (cand > 0 ? cand : 4) || c.sel_total != sel) violation(cs, "totals", -1);
    if (c.bk_part_total != part || P.bk_emap.size() % 8 || P.bk_emap.size() < (size_t)part) violation(cs, "bk_part_total", -1);
    for (size_t k = 0; k < P.cell_aux.size(); k += 2)
        if (P.cell_info[2 * k] & 0x100u && ((P.cell_aux[k] >> 17) & 0x7fu) < 1) violation(cs, "lane map", (int)(P.cell_info[2 * k] & 0xff));
    if (c.tail_n) { // every extended column of every tail level is computed by some strip, strips in order
        if ((int)P.tail_plan.size() != c.tail_strips * ORBFE_TAIL_MAX * 4) violation(cs, "tail plan size", c.tail_first);
        for (int st = 0; st < c.tail_n; st++) {
            int covered = 0;
            for (int sj = 0; sj < c.tail_strips; sj++) {
                const int *e = &P.tail_plan[((size_t)sj * ORBFE_TAIL_MAX + st) * 4];
                if (e[0] > covered || e[1] > 64) violation(cs, "tail strip gap", c.tail_first + st);
                covered = std::max(covered, e[0] + 4 * e[1]);
            }
            if (covered != c.lv[c.tail_first + st].rs_xtab_n) violation(cs, "tail coverage", c.tail_first + st);
        }
    } else if (!P.tail_plan.empty()) violation(cs, "unused tail plan", -1);
    for (int l = 1; l + 1 < c.nlevels; l++) { // pair plan: the stored ranges partition level l, each inside its tile's window
        const LevelInfo &D = c.lv[l];
        if (!D.pp_ok) continue;
        const int n[2] = {D.pp_ntx, D.pp_nty}, off[2] = {D.pp_xoff, D.pp_yoff}, end[2] = {D.rs_xtab_n >> 2, D.rs_ytab_n}, cap[2] = {64, 16};
        for (int a = 0; a < 2; a++) {
            int prev = 0;
            for (int t = 0; t < n[a]; t++) {
                const int *e = &P.pair_plan[(size_t)(off[a] + t) * 4];
                if (e[2] != prev || e[3] < e[2] || e[0] > e[2] || e[0] + e[1] < e[3] || e[1] > cap[a] || e[0] < 0 || e[0] + e[1] > end[a])
                    violation(cs, a ? "pair rows" : "pair columns", l);
                prev = e[3];
            }
            if (prev != end[a]) violation(cs, a ? "pair row partition" : "pair column partition", l);
        }
    }
    (void)p;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: plan_harness cases.txt [--dump cell_info,cell_aux]\n"); return 2; }
    const std::string dump = argc > 3 && !strcmp(argv[2], "--dump") ? argv[3] : "";
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
        if (rc != ORBFE_OK) {
            printf("err %s\n", err);
        } else {
            const int nl = P->cfg.nlevels;
            printf("cfg %016llx\n", fnv(&P->cfg, sizeof(P->cfg)));
            std::vector<float> lv;
            for (const float *a : {P->scale, P->inv_scale, P->sigma2, P->inv_sigma2}) lv.insert(lv.end(), a, a + nl);
            printf("levels %016llx %016llx\n", fnv(lv.data(), lv.size() * sizeof(float)), fnv(P->feats, sizeof(int32_t) * nl));
            printf("flags %d %zu %d %d %d %d %d %d\n", P->use_octree3, P->ot3_lds, P->ot3_nodes_in_hbm, P->ot_sort_cap, P->fuse_blur,
                   P->blur_ride_from, P->blur_ride_min_images, P->inplace_ok);
            tab("rs_tab", P->rs_tab); tab("rs_blk", P->rs_blk); tab("tail_plan", P->tail_plan); tab("pair_plan", P->pair_plan);
            tab("cell_info", P->cell_info); tab("cell_aux", P->cell_aux); tab("fast_lane_tab", P->fast_lane_tab);
            tab("bk_tab", P->bk_tab); tab("bk_off", P->bk_off); tab("bk_emap", P->bk_emap); tab("blur_tile_info", P->blur_tile_info);
            tab("slot_level", P->slot_level); tab("patch_uv", P->patch_uv); tab("mom_tab", P->mom_tab);
            // the plan facts the GPU tests are chosen for (tests/test_plan_host.py); not part of the digests
            printf("facts %s tail_first %d tail_n %d tail_max_images %d pp_max_images %d blur_ride_min_images %d blur_ride_from %d inplace_ok %d",
                   name, P->cfg.tail_first, P->cfg.tail_n, P->cfg.tail_max_images, P->cfg.pp_max_images, P->blur_ride_min_images,
                   P->blur_ride_from, (int)P->inplace_ok);
            for (int l = 1; l < nl; l++) printf(" L%d %d,%d,%d", l, P->cfg.lv[l].rs_direct, P->cfg.lv[l].rs_rw, P->cfg.lv[l].pp_ok);
            printf("\n");
            // the capacities the call-sequence scenes are chosen against (tests/test_call_sequences.py); not part of the digests either
            printf("caps %s sel_total %d row_cap %d\n", name, P->cfg.sel_total, P->cfg.row_cap);
            // the quadtree kernel and table placement (what orbfe_quadtree_plan() will return) and the geometry its predicates read
            // (tests/plan_limits.py); not part of the digests
            printf("quadtree %s plan %d max_nodes %d sort_cap %d n_ini", name, P->use_octree3 ? (P->ot3_nodes_in_hbm ? 1 : 0) : (P->otg_nodes_in_hbm ? 3 : 2),
                   P->cfg.max_nodes, P->ot_sort_cap);
            for (int l = 0; l < nl; l++) printf("%c%d", l ? ',' : ' ', P->cfg.lv[l].n_ini);
            printf(" n_cells");
            for (int l = 0; l < nl; l++) printf("%c%d", l ? ',' : ' ', P->cfg.lv[l].n_cells);
            printf("\n");
            check(name, p, *P);
            for (const char *t : {"cell_info", "cell_aux"}) {
                if (dump.find(t) == std::string::npos) continue;
                const std::vector<uint32_t> &v = !strcmp(t, "cell_info") ? P->cell_info : P->cell_aux;
                printf("dump %s %s", name, t);
                for (uint32_t w : v) printf(" %x", w);
                printf("\n");
            }
        }
        delete P;
        n_cases++;
    }
    fclose(f);
    printf("plan harness ok %d cases %d violations\n", n_cases, g_bad);
    return 0;
}
