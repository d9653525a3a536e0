// orbfe_plan.cpp -- the tables and launch plans of a context (orbfe_plan.h), computed on the host from its parameters.
//
// Builds the level / cell / quota tables exactly as ORBextractor::ORBextractor and ComputePyramid do (reference
// src/ORBextractor.cc:405-464,921-946), and the plans of the kernels' launches.  Compiled as plain C++ under contract Q4
// (-ffp-contract=off -fno-fast-math): the resize and scale arithmetic must round exactly as the reference's does.
#include "orbfe_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int plan_fail(char *err, size_t err_len, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt); vsnprintf(err, err_len, fmt, ap); va_end(ap);
    return code;
}

PlanKnobs PlanKnobs::from_env()
{
    PlanKnobs k;
    auto first = [](const char *name) { const char *v = getenv(name); return v ? v[0] : '\0'; };
    auto tri = [&](const char *name) { const char f = first(name); return f == '1' ? 1 : (f == '0' ? 0 : -1); };
    k.no_inplace = first("ORBFE_NO_INPLACE") == '1';
    k.no_pair = tri("ORBFE_NO_PAIR");
    k.no_tail = tri("ORBFE_NO_TAIL");
    k.pyr_lds = first("ORBFE_PYR_LDS") == '1';
    k.no_fuse = first("ORBFE_NO_FUSE") == '1';
    k.no_proc_order = first("ORBFE_NO_PROC_ORDER") == '1';
    { const char *v = getenv("ORBFE_OCTREE"); k.octree_generic = v && atoi(v) == 1; k.octree_generic_hbm = v && atoi(v) == 2; }
    { const char *v = getenv("ORBFE_BLUR_RIDE_FROM"); if (v && v[0] >= '0' && v[0] <= '9') k.blur_ride_from = atoi(v); }
    k.fast_split = tri("ORBFE_FAST_SPLIT");
    k.host_trace = getenv("ORBFE_HOST_TRACE") != nullptr;
    return k;
}

int orbfe_fast_launches(const DeviceConfig &c, bool split, bool side_blur, int blur_first, FastRange out[2])
{
    auto tile_off = [&](int l) { return l < c.nlevels ? c.lv[l].blur_tile_off : c.blur_tiles_total; };
    const int cut = c.nlevels >= 2 ? c.lv[1].cell_off : 0; // the planner orders cells and blur tiles by level: level 0's are the prefix
    if (!split || cut <= 0 || cut >= c.cells_total) {
        out[0] = FastRange{0, c.cells_total, tile_off(blur_first), c.blur_tiles_total};
        return 1;
    }
    out[0] = FastRange{0, cut, 0, side_blur ? tile_off(1) : 0};
    out[1] = FastRange{cut, c.cells_total, tile_off(side_blur && blur_first < 1 ? 1 : blur_first), c.blur_tiles_total};
    return 2;
}

// lo / hi: the smallest and largest source index in the entries [i0, i1) of a resize table (both halves of each word)
static void src_hull(const std::vector<uint32_t> &tab, int off, int i0, int i1, int &lo, int &hi)
{
    lo = INT_MAX; hi = -1;
    for (int i = i0; i < i1; i++) { const int a = (int)(tab[off + i] & 0xffffu), b = (int)(tab[off + i] >> 16); lo = std::min(lo, std::min(a, b)); hi = std::max(hi, std::max(a, b)); }
}

static int cv_round_f(float v) { return (int)lrintf(v); }

// OpenCV 4.5.5 getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED (see oracle for provenance)
static void gaussian_taps_q8(int ksize, double sigma, int *taps)
{
    double g[64];
    double scale2x = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < ksize; i++) {
        double x = (double)i - (double)(ksize - 1) * 0.5;
        g[i] = exp(scale2x * x * x);
        sum += g[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < ksize; i++) g[i] *= sum;
    int n2 = ksize / 2;
    double err = 0.0;
    long acc = 0;
    for (int i = 0; i < n2; i++) {
        double adj = g[i] * 256.0 + err;
        long v0 = lrint(adj);
        err = adj - (double)v0;
        taps[i] = (int)v0;
        taps[ksize - 1 - i] = (int)v0;
        acc += 2 * v0;
    }
    taps[n2] = (int)(256 - acc);
}

// Tables of ORBextractor::ORBextractor (src/ORBextractor.cc:405-464), the per-level geometry of ComputePyramid /
// ComputeKeyPointsOctTree / DistributeOctTree, then the device tables and launch plans.
int orbfe_build_plan(const orbfe_params &p, int max_images, const PlanKnobs &knobs, HostPlan *plan, char *err, size_t err_len)
{
    HostPlan &P = *plan;
    DeviceConfig &c = P.cfg;
    memset(&c, 0, sizeof(c));
    c.nlevels = p.nlevels;
    c.width = p.width; c.height = p.height;
    c.edge_threshold = p.edge_threshold;
    c.min_border = p.edge_threshold - 3;
    c.ini_th = p.ini_th_fast; c.min_th = p.min_th_fast;
    {   // integers 0 .. 255 as IEEE half precision (exact): 0 -> 0, else exponent e = floor(log2 t) biased by 15, mantissa t's bits below the leading one
        auto half_bits = [](int t) -> uint32_t {
            if (t <= 0) return 0u;
            int e = 0;
            while ((t >> (e + 1)) != 0) e++;
            return (uint32_t)(((e + 15) << 10) | (((t << (10 - e)) & 0x3ff)));
        };
        c.ini_th_h2 = half_bits(c.ini_th) * 0x10001u; c.min_th_h2 = half_bits(c.min_th) * 0x10001u;
    }
    c.half_patch = p.half_patch_size;
    c.bf = p.bf; c.fx = p.fx;
    c.mb = p.fx != 0.f ? p.bf / p.fx : 0.f; // mb := mbf / fx
    c.in_cn = 1; c.in_coef[0] = c.in_coef[1] = c.in_coef[2] = 0; c.in_shift = 15;
    c.in_image_bytes = (size_t)p.width * p.height;
    c.rm_on = 0; c.rm_sw = c.rm_sh = 0; c.rm_xy[0] = c.rm_xy[1] = nullptr; c.rm_a[0] = c.rm_a[1] = nullptr;
    c.n_dist = 0; for (int i = 0; i < 5; i++) c.dist[i] = 0.f;
    c.cam[0] = p.fx; c.cam[1] = p.fy; c.cam[2] = p.cx; c.cam[3] = p.cy;

    const double sf_d = (double)p.scale_factor; // member is double, initialised from float
    P.scale[0] = 1.0f; P.sigma2[0] = 1.0f;
    for (int i = 1; i < p.nlevels; i++) {
        P.scale[i] = (float)((double)P.scale[i - 1] * sf_d);
        P.sigma2[i] = P.scale[i] * P.scale[i];
    }
    for (int i = 0; i < p.nlevels; i++) {
        P.inv_scale[i] = 1.0f / P.scale[i];
        P.inv_sigma2[i] = 1.0f / P.sigma2[i];
    }
    const float factor = (float)(1.0 / sf_d);
    float n_desired = (float)p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)p.nlevels));
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; l++) {
        P.feats[l] = cv_round_f(n_desired);
        sum += P.feats[l];
        n_desired *= factor;
    }
    P.feats[p.nlevels - 1] = p.nfeatures - sum > 0 ? p.nfeatures - sum : 0;

    const int hp = p.half_patch_size;
    const int vmax = (int)floor((double)((float)hp * sqrtf(2.f) / 2 + 1));
    const int vmin = (int)ceil((double)((float)hp * sqrtf(2.f) / 2));
    const double hp2 = (double)(hp * hp);
    for (int v = 0; v <= vmax; ++v) c.umax[v] = (int)lrint(sqrt(hp2 - (double)(v * v)));
    for (int v = hp, v0 = 0; v >= vmin; --v) {
        while (c.umax[v0] == c.umax[v0 + 1]) ++v0;
        c.umax[v] = v0;
        ++v0;
    }
    gaussian_taps_q8(7, 2.0, c.taps);

    size_t pyr_off = 0, blur_off = 0;
    int cell_off = 0, cand_off = 0, sel_off = 0, tile_off = 0, cell_cap = 1, max_nodes = 8;
    for (int l = 0; l < p.nlevels; l++) {
        LevelInfo &L = c.lv[l];
        L.scale = P.scale[l]; L.inv_scale = P.inv_scale[l];
        L.w = cv_round_f((float)p.width * L.inv_scale);
        L.h = cv_round_f((float)p.height * L.inv_scale);
        if (L.w < 1 || L.h < 1) return plan_fail(err, err_len, ORBFE_ERR_UNSUPPORTED, "level %d is empty (%dx%d)", l, L.w, L.h);
        // reflect-101 margin: 4 px left, >= 12 px right, 3 rows above/below (see orbfe_pyramid.hip)
        L.pitch = (L.w + 16 + 63) & ~63;
        L.pyr_off = (int)(pyr_off + (size_t)3 * L.pitch + 4);
        pyr_off += ((size_t)L.pitch * (L.h + 6) + 255) & ~(size_t)255;
        // blurred copy: 32 x 4 px tiles (one 128-B line each), only the image itself (describe never leaves it by more than
        // the 2 px its aligned 40-byte patch rows overshoot: one spare tile column)
        L.blur_off = (int)blur_off;
        L.blur_tx = (L.w + 31) / 32 + 1;
        blur_off += (size_t)L.blur_tx * ((L.h + 3) / 4 + 1) * 128; // + one tile row: describe stages 40 rows from a multiple of 4 (up to row h + 1; loaded, never used)
        if (l > 0) {
            L.rs_scale_x = 1.0 / ((double)L.w / (double)c.lv[l - 1].w);
            L.rs_scale_y = 1.0 / ((double)L.h / (double)c.lv[l - 1].h);
        }
        L.scaled_patch = (int)((float)p.patch_size * L.scale);
        L.quota = P.feats[l];
        const int min_b = c.min_border;
        const int max_bx = L.w - p.edge_threshold + 3, max_by = L.h - p.edge_threshold + 3;
        const float width = (float)(max_bx - min_b), height = (float)(max_by - min_b);
        L.n_cols = (int)(width / 30.f);
        L.n_rows = (int)(height / 30.f);
        L.cell_off = cell_off; L.cand_off = cand_off;
        int cand_cap = 0;
        if (L.n_cols >= 1 && L.n_rows >= 1 && max_bx > min_b && max_by > min_b) {
            L.w_cell = (int)ceilf(width / (float)L.n_cols);
            L.h_cell = (int)ceilf(height / (float)L.n_rows);
            L.n_cells = L.n_cols * L.n_rows;
            for (int i = 0; i < L.n_rows; i++) {
                const int ini_y = min_b + i * L.h_cell;
                int my = ini_y + L.h_cell + 6;
                if (ini_y >= max_by - 3) continue;
                if (my > max_by) my = max_by;
                for (int j = 0; j < L.n_cols; j++) {
                    const int ini_x = min_b + j * L.w_cell;
                    int mx = ini_x + L.w_cell + 6;
                    if (ini_x >= max_bx - 6) continue;
                    if (mx > max_bx) mx = max_bx;
                    const int iw = mx - ini_x - 6, ih = my - ini_y - 6;
                    if (iw <= 0 || ih <= 0) continue;
                    const int cc = ((iw + 1) / 2) * ((ih + 1) / 2); // 3x3 strict NMS survivors bound
                    cand_cap += cc;
                    if (cc > cell_cap) cell_cap = cc;
                }
            }
            L.n_ini = (int)roundf(width / height);
            if (L.n_ini < 1) L.n_ini = 1; // reference would index an empty vector; documented guard
            L.hx = width / (float)L.n_ini;
        } else {
            L.n_cols = L.n_rows = 0; L.w_cell = L.h_cell = 0; L.n_cells = 0;
            L.n_ini = 1; L.hx = 1.f;
        }
        L.cand_cap = cand_cap;
        cell_off += L.n_cells;
        cand_off += (cand_cap + 3) & ~3;
        L.sel_off = sel_off;
        L.sel_cap = (L.quota + 3 > 4 * L.n_ini ? L.quota + 3 : 4 * L.n_ini) + 1;
        sel_off += L.sel_cap;
        if (L.sel_cap + 1 > max_nodes) max_nodes = L.sel_cap + 1;
        L.blur_tile_off = tile_off;
        L.blur_tiles_x = (L.w + 255) / 256;
        L.blur_tiles_y = (L.h + ORBFE_BLUR_ROWS - 1) / ORBFE_BLUR_ROWS;
        tile_off += L.blur_tiles_x * L.blur_tiles_y;
    }
    c.pyr_bytes = pyr_off;
    c.blur_bytes = blur_off + 256;
    c.cells_total = cell_off > 0 ? cell_off : 1;
    c.cand_total = cand_off > 0 ? cand_off : 4;
    c.sel_total = sel_off;
    c.cell_cap = cell_cap;
    c.blur_tiles_total = tile_off;
    c.max_nodes = max_nodes;
    if (p.width > 32767 || p.height > 32767) return plan_fail(err, err_len, ORBFE_ERR_UNSUPPORTED, "image larger than 32767 px");
    if (c.sel_total > 65535) return plan_fail(err, err_len, ORBFE_ERR_UNSUPPORTED, "nfeatures too large (keypoint capacity %d > 65535)", c.sel_total);
    {
        const int sc = orbfe_sort_cap(c.max_nodes);
        bool roots_ok = true;
        for (int l = 0; l < p.nlevels; l++) roots_ok = roots_ok && c.lv[l].n_ini <= 4;
        int max_cand = 0;
        for (int l = 0; l < p.nlevels; l++) { roots_ok = roots_ok && c.lv[l].cand_cap <= (1 << 20); max_cand = c.lv[l].cand_cap > max_cand ? c.lv[l].cand_cap : max_cand; }
        P.ot_sort_cap = sc;
        {
            bool ok3 = roots_ok && c.cell_cap <= 4095; // key fields: 12-bit cell, 12-bit slot; bucket partials: 12-bit count
            for (int l = 0; l < p.nlevels; l++) ok3 = ok3 && c.lv[l].n_cells <= 4096 && c.lv[l].w_cell <= 64 && c.lv[l].h_cell <= 64; // one lane per cell column / row
            // the counts of the two deepest pyramid depths are 16 bit: a depth-4 node (1 / 256 of a root) holds at most one strict-NMS
            // survivor per 2 x 2 px (always true within the cell-count limit above: <= 4096 cells of <= 64 x 64 px per level)
            for (int l = 0; l < p.nlevels; l++) {
                const long rw = (long)(c.lv[l].w - p.edge_threshold + 3) - c.min_border, rh = (long)(c.lv[l].h - p.edge_threshold + 3) - c.min_border;
                if (rw > 0 && rh > 0) ok3 = ok3 && ((rw / c.lv[l].n_ini / 16 + 2) / 2 + 1) * ((rh / 16 + 2) / 2 + 1) <= 65535;
            }
            P.ot3_nodes_in_hbm = orbfe_octree3_lds_bytes(c.max_nodes, sc, false) > 150 * 1024;
            P.ot3_lds = orbfe_octree3_lds_bytes(c.max_nodes, sc, P.ot3_nodes_in_hbm);
            // ORBFE_OCTREE=1 (test knob): the generic node-parallel kernel (the fallback beyond the bucket-pyramid kernel's limits) with
            // its node tables in LDS; ORBFE_OCTREE=2: the same kernel with its node tables in HBM scratch
            P.use_octree3 = ok3 && P.ot3_lds <= 150 * 1024 && !knobs.octree_generic && !knobs.octree_generic_hbm;
        }
        // the generic kernel's node tables: LDS while they fit, else HBM scratch (any quota up to the keypoint capacity); the forced LDS
        // form of ORBFE_OCTREE=1 refuses instead
        P.otg_nodes_in_hbm = false; P.otg_scratch_bytes = 0;
        if (!P.use_octree3) {
            if (knobs.octree_generic_hbm || (orbfe_octree_lds_bytes(c) > 150 * 1024 && !knobs.octree_generic)) P.otg_nodes_in_hbm = true;
            else if (orbfe_octree_lds_bytes(c) > 150 * 1024)
                return plan_fail(err, err_len, ORBFE_ERR_UNSUPPORTED, "nfeatures too large for the quadtree LDS budget");
            // best response of a node: score << 24 | position inside the node, and a root may hold every candidate of its level
            for (int l = 0; l < p.nlevels; l++)
                if (c.lv[l].cand_cap >= (1 << 24))
                    return plan_fail(err, err_len, ORBFE_ERR_UNSUPPORTED, "level %d: %d candidate slots exceed the 2^24 in-node positions of the generic quadtree kernel", l, c.lv[l].cand_cap);
        }
        // scratch of octree_generic_kernel<true>, also what orbfe_create allocates when the bucket-pyramid kernel cannot be prepared
        // at run time and the LDS tables would not fit
        if (P.otg_nodes_in_hbm) {
            P.otg_scratch_bytes = orbfe_otg_level_off(c, c.nlevels);
            if (knobs.host_trace) fprintf(stderr, "orbfe: generic quadtree kernel: node tables in HBM scratch, %zu bytes per image\n", P.otg_scratch_bytes);
        }
    }
    // the tables and launch plans of that geometry
    // the XCD-aware block maps divide jb = blockIdx.x / 8 through a float reciprocal that is exact for jb < 2^21 (small_div,
    // orbfe_common.hpp), i.e. below 2^24 workgroups per launch; xcd_grid may round a launch up to twice blocks x images, so
    // the limit on blocks x images is 2^23
    if (((size_t)c.cells_total / 4 + 1 + (size_t)c.blur_tiles_total / 4 + 1) * (size_t)max_images >= ((size_t)1 << 23) || // FAST's launch may carry blur tiles too
        ((size_t)c.sel_total / 4 + 1) * (size_t)max_images >= ((size_t)1 << 23))
        return plan_fail(err, err_len, ORBFE_ERR_CAPACITY, "max_images %d: more than 2^23 workgroups per launch", max_images);
    {   // stereo row lists (vRowIndices, src/Frame.cc:474-491): fixed capacity per row, ~4x the mean occupancy
        // (a right keypoint is listed in ~2 * 2 * scale + 1 rows); a fuller row makes stereo_match_kernel scan all keypoints
        c.row_cap = std::min(std::max((int)(4.0 * c.sel_total * 10.0 / p.height), 64), c.sel_total);
    }
    {   // cv::resize tables (resize.cpp: xofs/ialpha, yofs/ibeta) over the margin-extended domain of each level
        std::vector<uint32_t> tab;
        auto reflect = [](int q, int len) { if (len == 1) return 0; while (q < 0 || q >= len) q = q < 0 ? -q : 2 * len - 2 - q; return q; };
        for (int l = 1; l < p.nlevels; l++) {
            LevelInfo &D = c.lv[l];
            const LevelInfo &S = c.lv[l - 1];
            const int nx = (D.w + 12 + 3) & ~3, ny = D.h + 6;
            while (tab.size() % 4) tab.push_back(0);
            D.rs_xtab_off = (int)tab.size(); D.rs_xtab_n = nx;
            tab.resize(tab.size() + 2 * (size_t)nx, 0);
            for (int i = 0; i < nx; i++) {
                const int dx = reflect(i - 4, D.w);
                float fx = (float)(((double)dx + 0.5) * D.rs_scale_x - 0.5);
                int sx = (int)floorf(fx);
                fx -= (float)sx;
                if (sx < 0) { fx = 0.f; sx = 0; }
                if (sx >= S.w - 1) { fx = 0.f; sx = S.w - 1; }
                const int a0 = (int)lrintf((1.f - fx) * 2048.f), a1 = (int)lrintf(fx * 2048.f);
                const int sx1 = sx + 1 < S.w ? sx + 1 : S.w - 1;
                tab[D.rs_xtab_off + i] = (uint32_t)sx | ((uint32_t)sx1 << 16);
                tab[D.rs_xtab_off + nx + i] = (uint32_t)a0 | ((uint32_t)a1 << 16);
            }
            {   // pyr_resize_direct_kernel: the two source bytes of every column as a v_perm_b32 selector into the 8 bytes that
                // start at the leftmost source byte of the column's 4-column word, and that byte's offset per word
                D.rs_dtab_off = (int)tab.size();
                tab.resize(tab.size() + (size_t)nx + nx / 4, 0);
                bool direct = true;
                for (int wd = 0; wd < nx / 4; wd++) {
                    int lo = INT_MAX;
                    for (int j = 0; j < 4; j++) {
                        const uint32_t e = tab[D.rs_xtab_off + 4 * wd + j];
                        lo = std::min(lo, std::min((int)(e & 0xffffu), (int)(e >> 16)));
                    }
                    tab[D.rs_dtab_off + nx + wd] = (uint32_t)lo;
                    if (resize_word_base(wd, D.w, D.rs_scale_x, S.w) != lo) direct = false; // the kernel computes this offset
                    for (int j = 0; j < 4; j++) {
                        const uint32_t e = tab[D.rs_xtab_off + 4 * wd + j];
                        const int o0 = (int)(e & 0xffffu) - lo, o1 = (int)(e >> 16) - lo;
                        if (o0 > 7 || o1 > 7) direct = false;
                        tab[D.rs_dtab_off + 4 * wd + j] = 0x0c000c00u | (uint32_t)(o0 & 7) | ((uint32_t)(o1 & 7) << 16);
                    }
                }
                D.rs_direct = direct && ORBFE_PYR_RB > 0 && !knobs.pyr_lds;
                if (knobs.host_trace) fprintf(stderr, "orbfe: level %d cv::resize: %s kernel\n", l, D.rs_direct ? "direct (aligned 96-bit row loads)" : "LDS-staged");
            }
            D.rs_ytab_off = (int)tab.size(); D.rs_ytab_n = ny;
            tab.resize(tab.size() + 2 * (size_t)ny, 0);
            for (int i = 0; i < ny; i++) {
                const int dy = reflect(i - 3, D.h);
                float fy = (float)(((double)dy + 0.5) * D.rs_scale_y - 0.5);
                int sy = (int)floorf(fy);
                fy -= (float)sy;
                const int b0 = (int)lrintf((1.f - fy) * 2048.f), b1 = (int)lrintf(fy * 2048.f);
                const int sy0 = sy < 0 ? 0 : (sy > S.h - 1 ? S.h - 1 : sy);
                const int sy1 = sy + 1 < 0 ? 0 : (sy + 1 > S.h - 1 ? S.h - 1 : sy + 1);
                tab[D.rs_ytab_off + i] = (uint32_t)sy0 | ((uint32_t)sy1 << 16);
                tab[D.rs_ytab_off + ny + i] = (uint32_t)b0 | ((uint32_t)b1 << 16);
            }
            for (int v = 0; v < 3; v++) { // source-row span of the worst block of 16 / 8 / 4 output rows
                const int rows = 16 >> v;
                int worst = 1;
                for (int y0 = 0; y0 < ny; y0 += rows) {
                    int lo, hi;
                    src_hull(tab, D.rs_ytab_off, y0, std::min(y0 + rows, ny), lo, hi);
                    worst = std::max(worst, hi - lo + 1);
                }
                D.rs_src_rows[v] = worst;
            }
        }
        {   // per-block source-row range of the resize launches (pyr_resize_kernel stages it before it has read any row table)
            std::vector<uint32_t> blk;
            for (int l = 1; l < p.nlevels; l++) {
                LevelInfo &D = c.lv[l];
                const int src_words = (c.lv[l - 1].w + 3) / 4, ny = D.h + 6;
                const size_t rowp = ((size_t)src_words * 4 + 15) & ~(size_t)15; // staged row pitch (pyr_resize_kernel)
                D.rs_rw = D.rs_src_rows[0] * rowp <= 60 * 1024 ? 4 : (D.rs_src_rows[1] * rowp <= 60 * 1024 ? 2 : 1);
                D.rs_blk_off = (int)blk.size();
                const int rows = 4 * D.rs_rw;
                for (int y0 = 0; y0 < ny; y0 += rows) {
                    int lo, hi;
                    src_hull(tab, D.rs_ytab_off, y0, std::min(y0 + rows, ny), lo, hi);
                    blk.push_back((uint32_t)lo | ((uint32_t)(hi - lo + 1) << 16));
                }
            }
            if (blk.empty()) blk.push_back(0);
            P.rs_blk.swap(blk);
        }
        {   // plan of the fused pyramid tail (pyr_tail_kernel): a workgroup owns a strip of ORBFE_TAIL_COLS extended columns of
            // the LAST level over all its rows and computes, level by level in LDS, exactly the columns of the previous tail
            // levels that strip needs (plus the margin columns at the image's left / right, which no later level reads);
            // columns shared by neighbouring strips (one or two per level) are computed twice
            c.tail_first = 0; c.tail_n = 0; c.tail_strips = 0; c.tail_lds_bytes = 0;
            const int nst = p.nlevels >= 4 ? 3 : (p.nlevels == 3 ? 2 : 0);
            P.fuse_blur = !knobs.no_fuse;
            if (knobs.blur_ride_from >= 0) { P.blur_ride_from = knobs.blur_ride_from; P.blur_ride_min_images = 1; } // given explicitly: for every batch size
            c.tail_max_images = knobs.no_tail == 0 ? INT_MAX : 63; // ORBFE_NO_TAIL=0: the tail at every batch size (A/B)
            if (nst >= 2 && knobs.no_tail != 1) {
                const int F = p.nlevels - nst, Lz = p.nlevels - 1;
                const int strips = (c.lv[Lz].rs_xtab_n + ORBFE_TAIL_COLS - 1) / ORBFE_TAIL_COLS;
                std::vector<int> plan((size_t)strips * ORBFE_TAIL_MAX * 4, 0);
                int max_wd[ORBFE_TAIL_MAX] = {0, 0, 0}, max_src = 0;
                bool ok = true;
                for (int sj = 0; sj < strips; sj++) {
                    int x0 = sj * ORBFE_TAIL_COLS, n = std::min(ORBFE_TAIL_COLS, c.lv[Lz].rs_xtab_n - x0);
                    for (int st = nst - 1; st >= 0; st--) {
                        const int l = F + st;
                        int *e = &plan[((size_t)sj * ORBFE_TAIL_MAX + st) * 4];
                        e[0] = x0; e[1] = n >> 2;
                        max_wd[st] = std::max(max_wd[st], n >> 2);
                        if (n >> 2 > 64) ok = false; // one lane per 4-pixel word of a strip row
                        int lo, hi;
                        src_hull(tab, c.lv[l].rs_xtab_off, x0, x0 + n, lo, hi); // interior columns of level l - 1 (sources of extended columns [x0, x0 + n))
                        if (st == 0) {
                            e[2] = lo & ~3; e[3] = (((hi | 3) + 1) - (lo & ~3)) >> 2; // staged words of level F - 1 (4-aligned interior start)
                            max_src = std::max(max_src, e[3]);
                            break;
                        }
                        // columns of level l - 1 this strip computes: the needed interior columns (+ PYR_MX as extended index)
                        // rounded out to words, and the margin columns for the first / last strip
                        x0 = sj == 0 ? 0 : ((lo + 4) & ~3);
                        const int x1 = sj == strips - 1 ? c.lv[l - 1].rs_xtab_n : std::min(c.lv[l - 1].rs_xtab_n, ((hi + 4) | 3) + 1);
                        n = x1 - x0;
                    }
                }
                for (int st = 0; st < nst && ok; st++) { // every extended column of every tail level is computed by some strip
                    int covered = 0;
                    for (int sj = 0; sj < strips; sj++) {
                        const int *e = &plan[((size_t)sj * ORBFE_TAIL_MAX + st) * 4];
                        if (e[0] > covered) ok = false;
                        covered = std::max(covered, e[0] + 4 * e[1]);
                    }
                    if (covered != c.lv[F + st].rs_xtab_n) ok = false;
                }
                size_t off = 0;
                for (int st = 0; st < nst; st++) { c.tail_lds_y[st] = (int)off; off += (size_t)2 * c.lv[F + st].rs_ytab_n * 4; }
                off = (off + 15) & ~(size_t)15;
                c.tail_lds_src = (int)off;
                off += (size_t)c.lv[F - 1].h * max_src * 4;
                for (int st = 0; st + 1 < nst; st++) {
                    c.tail_lds_buf[st] = (int)off;
                    off += (size_t)(c.lv[F + st].h + 6) * max_wd[st] * 4;
                }
                if (ok && F >= 1 && off <= 64 * 1024) {
                    c.tail_first = F; c.tail_n = nst; c.tail_strips = strips; c.tail_src_words = max_src;
                    for (int st = 0; st < nst; st++) c.tail_words[st] = max_wd[st];
                    c.tail_lds_bytes = (int)off;
                    if (knobs.host_trace) fprintf(stderr, "orbfe: pyramid tail: levels %d..%d, %d strips, %d bytes of LDS per workgroup\n", F, F + nst - 1, strips, (int)off);
                    P.tail_plan.swap(plan);
                }
            }
        }
        {   // plan of pyr_pair_kernel (levels l and l + 1 in one launch): tiles of TW words x TR extended rows of level l + 1; per tile
            // column the words of level l (extended) its sources lie in and the words it stores, per tile row the same for rows.
            // The stored ranges partition level l's extended domain; a tile computes the hull of both.
            std::vector<int> plan;
            const bool want = knobs.no_pair != 1;
            c.pp_max_images = knobs.no_pair == 0 ? INT_MAX : 63; // ORBFE_NO_PAIR=0: pairs at every batch size (A/B)
            for (int l = 1; l + 1 < p.nlevels; l++) {
                LevelInfo &D1 = c.lv[l];
                const LevelInfo &D2 = c.lv[l + 1];
                D1.pp_ok = 0;
                if (!want || !D1.rs_direct || !D2.rs_direct) continue;
                const int nw1 = D1.rs_xtab_n >> 2, ny1 = D1.rs_ytab_n, nw2 = D2.rs_xtab_n >> 2, ny2 = D2.rs_ytab_n;
                static const int k_tr[4] = {12, 11, 10, 8}, k_tw[6] = {48, 44, 40, 32, 24, 16};
                for (int ci = 0; ci < 24 && !D1.pp_ok; ci++) { // the largest tile whose level-l rectangle fits 64 words x 16 rows
                    const int TR = k_tr[ci / 6], TW = k_tw[ci % 6];
                    const int ntx = (nw2 + TW - 1) / TW, nty = (ny2 + TR - 1) / TR;
                    std::vector<int> px((size_t)ntx * 4), py((size_t)nty * 4);
                    bool ok = true;
                    int prev = 0;
                    for (int t = 0; t < ntx && ok; t++) { // columns: sources of extended columns [4 TW t, ...) of level l + 1
                        int lo, hi;
                        src_hull(tab, D2.rs_xtab_off, 4 * TW * t, std::min(4 * TW * (t + 1), D2.rs_xtab_n), lo, hi);
                        // the kernel's windows start at the word's computed first source byte and read 12 bytes from the 4-byte boundary below
                        const int need0 = (lo + 4) >> 2, need1 = ((hi + 4) >> 2) + 1; // extended words [need0, need1) of level l (interior column c = extended byte c + 4)
                        const int s0 = t == 0 ? 0 : std::max(prev, std::min(need0, prev)); // stores continue where the previous tile's ended
                        const int s1 = t == ntx - 1 ? nw1 : need1;
                        const int c0 = std::min(need0, s0), c1 = std::max(need1, s1);
                        if (t > 0 && need0 > prev) ok = false; // a gap nobody would store
                        px[4 * t] = c0; px[4 * t + 1] = c1 - c0; px[4 * t + 2] = s0; px[4 * t + 3] = std::max(s1, s0);
                        if (c1 - c0 > 64 || c0 < 0 || c1 > nw1) ok = false;
                        prev = std::max(s1, s0);
                    }
                    if (prev != nw1) ok = false;
                    prev = 0;
                    for (int t = 0; t < nty && ok; t++) {
                        int lo, hi;
                        src_hull(tab, D2.rs_ytab_off, TR * t, std::min(TR * (t + 1), ny2), lo, hi);
                        const int need0 = lo + 3, need1 = hi + 3 + 1; // extended rows of level l (interior row r = extended row r + 3)
                        const int s0 = t == 0 ? 0 : prev;
                        const int s1 = t == nty - 1 ? ny1 : need1;
                        if (t > 0 && need0 > prev) ok = false;
                        const int c0 = std::min(need0, s0), c1 = std::max(need1, s1);
                        py[4 * t] = c0; py[4 * t + 1] = c1 - c0; py[4 * t + 2] = s0; py[4 * t + 3] = std::max(s1, s0);
                        if (c1 - c0 > 16 || c0 < 0 || c1 > ny1) ok = false;
                        prev = std::max(s1, s0);
                    }
                    if (prev != ny1) ok = false;
                    if (!ok) continue;
                    D1.pp_ok = 1; D1.pp_ntx = ntx; D1.pp_nty = nty; D1.pp_tw = TW; D1.pp_tr = TR;
                    D1.pp_xoff = (int)plan.size() / 4; plan.insert(plan.end(), px.begin(), px.end());
                    D1.pp_yoff = (int)plan.size() / 4; plan.insert(plan.end(), py.begin(), py.end());
                }
                if (knobs.host_trace) fprintf(stderr, "orbfe: levels %d + %d in one launch: %s (%d x %d tiles of %d words x %d rows)\n", l, l + 1, D1.pp_ok ? "yes" : "no", D1.pp_ntx, D1.pp_nty, D1.pp_tw, D1.pp_tr);
            }
            if (plan.empty()) plan.resize(4, 0);
            P.pair_plan.swap(plan);
        }
        while (tab.size() % 4) tab.push_back(0);
        if (tab.empty()) tab.resize(4, 0);
        P.rs_tab.swap(tab);
    }
    std::vector<uint32_t> bk_tab_host;
    {   // FAST cell table: what fast_cell_kernel's prologue would otherwise derive per wave from a chain of dependent scalar loads
        // (level search over lv[].cell_off, a division by n_cols, the clipping of src/ORBextractor.cc:783-800)
        std::vector<uint32_t> ci((size_t)c.cells_total * 4, 0u), ca((size_t)c.cells_total * 2, 0u);
        std::vector<uint32_t> shapes, lane_tab; // tile w | h << 8 of every distinct cell shape; [shape][64][8]
        const int pw = orbfe_fast_tile_pitch(c) >> 2;
        for (int l = 0; l < p.nlevels; l++) {
            const LevelInfo &L = c.lv[l];
            const int max_bx = L.w - c.edge_threshold + 3, max_by = L.h - c.edge_threshold + 3;
            for (int k = 0; k < L.n_cells; k++) {
                const int i = k / L.n_cols, j = k - i * L.n_cols;
                const int ini_y = c.min_border + i * L.h_cell, ini_x = c.min_border + j * L.w_cell;
                int max_y = ini_y + L.h_cell + 6, max_x = ini_x + L.w_cell + 6;
                uint32_t *e = &ci[(size_t)(L.cell_off + k) * 4];
                e[0] = (uint32_t)l; e[3] = (uint32_t)k;
                if (ini_y >= max_by - 3 || ini_x >= max_bx - 6) continue; // src/ORBextractor.cc:788-798: no FAST call
                if (max_y > max_by) max_y = max_by;
                if (max_x > max_bx) max_x = max_bx;
                const int tw = max_x - ini_x, th = max_y - ini_y;
                if (tw - 6 <= 0 || th - 6 <= 0) continue;
                e[0] |= 1u << 8;
                e[1] = (uint32_t)ini_x | ((uint32_t)ini_y << 16);
                e[2] = (uint32_t)tw | ((uint32_t)th << 8);
                // the divisions of fast_cell_kernel's lane maps (its prologue: tile staging by 16-byte chunks, phase A by 4-pixel groups)
                const int iw = tw - 6, ih = th - 6;
                const int ng = (iw + 3) >> 2, dr = 64 / ng;
                // a wave covers at least one interior row (ng <= 64 groups); w_cell < 60 keeps ng <= 15, so no geometry reaches this
                if (dr < 1) return plan_fail(err, err_len, ORBFE_ERR_UNSUPPORTED, "level %d: FAST cell %d px wide exceeds the 64-lane row map", l, iw);
                const int r0_last = ((ih - 1) / dr) * dr;
                const int cpr = ((((tw + 3) >> 2)) + 3) >> 2, rpi = 64 / cpr;
                uint32_t *a = &ca[(size_t)(L.cell_off + k) * 2];
                size_t shape = 0;
                while (shape < shapes.size() && shapes[shape] != e[2]) shape++;
                if (shape == shapes.size()) { // phase A's per-lane constants for this tile size (fast_cell_kernel documents them)
                    shapes.push_back(e[2]);
                    for (int lane = 0; lane < 64; lane++) {
                        const int rl = lane / ng, jg = lane - rl * ng, c0 = 4 * jg;
                        const bool act = rl < dr, in_last = r0_last + rl < ih;
                        const uint32_t vm01 = (act ? 0x8000u : 0u) | (act && c0 + 1 < iw ? 0x80000000u : 0u);
                        const uint32_t vm23 = (act && c0 + 2 < iw ? 0x8000u : 0u) | (act && c0 + 3 < iw ? 0x80000000u : 0u);
                        const uint32_t row[8] = {vm01, vm23, in_last ? vm01 : 0u, in_last ? vm23 : 0u,
                                                 (uint32_t)(((rl + 1) << 8) + c0) * 0x10001u + 0x10000u, (uint32_t)(rl * pw + jg), 0u, 0u};
                        lane_tab.insert(lane_tab.end(), row, row + 8);
                    }
                }
                a[0] = (uint32_t)shape | ((uint32_t)dr << 17) | ((uint32_t)r0_last << 24);
                a[1] = (uint32_t)((65536 + cpr - 1) / cpr) | ((uint32_t)rpi << 17);
            }
        }
        if (lane_tab.empty()) lane_tab.resize(512, 0u);
        // bucket partials (fast_cell_kernel phase E -> octree3_kernel): the survivors of a cell fall into the bucket columns
        // X[first col] >> 16 .. X[last col] >> 16 and the rows Y[..] >> 16 likewise (the tables are monotone).  A cell whose
        // rectangle has at most 64 buckets accumulates them in LDS and stores the count and best key of each with plain
        // stores into its own entries of bk_part (one word each); bk_emap names the bucket and the cell of every entry.  Cells with larger rectangles
        // (the small levels, where a bucket is 3 px wide) have no entries: the quadtree kernel buckets their candidates.
        std::vector<uint32_t> off((size_t)c.cells_total, 0u);
        std::vector<uint32_t> emap;
        auto spread5 = [](unsigned v) { unsigned r = 0; for (int i = 0; i < 5; i++) r |= ((v >> i) & 1u) << (2 * i); return r; };
        // Quadtree bucket tables (orbfe_octree3.hip): root and path bits down to the level's bucket depth of every x / y of the
        // level's candidate region, with the reference's arithmetic (src/ORBextractor.cc:537-564 roots, :145-209 splits):
        //   X[x] = root << 2 depth | x path bits spread to the even positions | (root * 2^depth + column) << 16
        //   Y[y] = y path bits spread to the odd positions | row << 16
        // Bucket depth per level (round 4): 5, or 4 where some FAST cell of the level spans more than 64 depth-5 buckets (the small
        // levels, whose depth-5 buckets are ~3 px: their candidates were bucketed one by one inside the quadtree kernel, 14-18 us of
        // those workgroups, which ended the launch).  A quota of ~200 nodes over 4 roots splits down to depth 3-4; nodes deeper than
        // the level's bucket depth take the kernel's slow path as before.
        auto build_tabs = [&](const LevelInfo &L, int depth, std::vector<uint32_t> &X, std::vector<uint32_t> &Y) {
            const int region_w = (L.w - p.edge_threshold + 3) - c.min_border, region_h = (L.h - p.edge_threshold + 3) - c.min_border;
            X.clear(); Y.clear();
            for (int x = 0; x < region_w; x++) {
                int b = (int)((float)x / L.hx);
                b = b < 0 ? 0 : (b >= L.n_ini ? L.n_ini - 1 : b);
                int x0 = (int)(L.hx * (float)b), x1 = (int)(L.hx * (float)(b + 1));
                unsigned col = 0;
                for (int d = 0; d < depth; d++) {
                    const int mx = x0 + ((x1 - x0 + 1) >> 1);
                    const int cx = x < mx ? 0 : 1;
                    col = (col << 1) | (unsigned)cx;
                    if (cx) x0 = mx; else x1 = mx;
                }
                X.push_back(((unsigned)b << (2 * depth)) | spread5(col) | ((((unsigned)b << depth) + col) << 16));
            }
            for (int y = 0; y < region_h; y++) {
                int y0 = 0, y1 = region_h;
                unsigned row = 0;
                for (int d = 0; d < depth; d++) {
                    const int my = y0 + ((y1 - y0 + 1) >> 1);
                    const int cy = y < my ? 0 : 1;
                    row = (row << 1) | (unsigned)cy;
                    if (cy) y0 = my; else y1 = my;
                }
                Y.push_back((spread5(row) << 1) | (row << 16));
            }
        };
        auto max_cell_buckets = [&](const LevelInfo &L, const std::vector<uint32_t> &X, const std::vector<uint32_t> &Y) {
            int worst = 0;
            for (int k = 0; k < L.n_cells; k++) {
                const uint32_t *e = &ci[(size_t)(L.cell_off + k) * 4];
                if (!(e[0] & 0x100u)) continue;
                const int cx0 = (int)(e[1] & 0xffffu) - c.min_border, cy0 = (int)(e[1] >> 16) - c.min_border;
                const int iw = (int)(e[2] & 0xffu) - 6, ih = (int)((e[2] >> 8) & 0xffu) - 6;
                const int nb = ((int)(X[3 + cx0 + iw - 1] >> 16) - (int)(X[3 + cx0] >> 16) + 1) * ((int)(Y[3 + cy0 + ih - 1] >> 16) - (int)(Y[3 + cy0] >> 16) + 1);
                worst = std::max(worst, nb);
            }
            return worst;
        };
        {
            std::vector<uint32_t> X, Y;
            for (int l = 0; l < p.nlevels; l++) {
                LevelInfo &L = c.lv[l];
                L.bk_depth = ORBFE_BK_DEPTH;
                build_tabs(L, ORBFE_BK_DEPTH, X, Y);
                if (max_cell_buckets(L, X, Y) > 64) { // depth 4 where a FAST cell would span more than 64 depth-5 buckets (else the quadtree kernel buckets that level's candidates one by one)
                    std::vector<uint32_t> X4, Y4;
                    build_tabs(L, ORBFE_BK_DEPTH - 1, X4, Y4);
                    if (max_cell_buckets(L, X4, Y4) <= 64) { L.bk_depth = ORBFE_BK_DEPTH - 1; X.swap(X4); Y.swap(Y4); }
                }
                L.bk_xoff = (int)bk_tab_host.size(); bk_tab_host.insert(bk_tab_host.end(), X.begin(), X.end());
                L.bk_yoff = (int)bk_tab_host.size(); bk_tab_host.insert(bk_tab_host.end(), Y.begin(), Y.end());
                if (knobs.host_trace) fprintf(stderr, "orbfe: level %d quadtree bucket depth %d\n", l, L.bk_depth);
            }
            if (bk_tab_host.empty()) bk_tab_host.resize(4, 0);
        }
        for (int l = 0; l < p.nlevels; l++) {
            LevelInfo &L = c.lv[l];
            while (emap.size() % 4) emap.push_back(0); // octree3_kernel reads a level's entries as 128-bit quads: 16-byte aligned start, padded end (the padding's bk_part words stay zero: no cell owns them)
            L.bk_part_off = (int)emap.size();
            L.bk_points = 0;
            for (int k = 0; k < L.n_cells; k++) {
                const uint32_t *e = &ci[(size_t)(L.cell_off + k) * 4];
                off[L.cell_off + k] = (uint32_t)emap.size();
                if (!(e[0] & 0x100u)) continue; // no FAST call: no entries
                const int cx0 = (int)(e[1] & 0xffffu) - c.min_border, cy0 = (int)(e[1] >> 16) - c.min_border;
                const int iw = (int)(e[2] & 0xffu) - 6, ih = (int)((e[2] >> 8) & 0xffu) - 6;
                const uint32_t *tx = &bk_tab_host[L.bk_xoff + 3 + cx0], *ty = &bk_tab_host[L.bk_yoff + 3 + cy0];
                const int gx0 = (int)(tx[0] >> 16), gx1 = (int)(tx[iw - 1] >> 16), by0 = (int)(ty[0] >> 16), by1 = (int)(ty[ih - 1] >> 16);
                const int ncols = gx1 - gx0 + 1, nb = ncols * (by1 - by0 + 1);
                if (nb > 64) { off[L.cell_off + k] = ~0u; L.bk_points = 1; continue; }
                for (int j = 0; j < nb; j++) {
                    const unsigned gx = (unsigned)(gx0 + j % ncols), by = (unsigned)(by0 + j / ncols);
                    const int dp = L.bk_depth;
                    emap.push_back(((gx >> dp) << (2 * dp)) | spread5(gx & ((1u << dp) - 1u)) | (spread5(by) << 1) | ((uint32_t)k << 16));
                }
            }
            while (emap.size() % 4) emap.push_back(0);
            L.bk_part_n = (int)emap.size() - L.bk_part_off;
        }
        c.bk_part_total = (int)emap.size();
        while (emap.size() % 8 || emap.empty()) emap.push_back(0);
        P.cell_info.swap(ci); P.cell_aux.swap(ca); P.fast_lane_tab.swap(lane_tab); P.bk_off.swap(off); P.bk_emap.swap(emap);
    }
    P.bk_tab.swap(bk_tab_host);
    {   // blur tile table (blur_kernel): level, 256-column strip and first row of every wave's tile
        std::vector<uint32_t> ti((size_t)(c.blur_tiles_total > 0 ? c.blur_tiles_total : 1), 0u);
        for (int l = 0; l < p.nlevels; l++) {
            const LevelInfo &L = c.lv[l];
            for (int t = 0; t < L.blur_tiles_x * L.blur_tiles_y; t++)
                ti[L.blur_tile_off + t] = (uint32_t)l | ((uint32_t)(t % L.blur_tiles_x) << 8) | ((uint32_t)((t / L.blur_tiles_x) * ORBFE_BLUR_ROWS) << 16);
        }
        P.blur_tile_info.swap(ti);
    }
    {   // keypoint slot -> level
        std::vector<uint8_t> sl((size_t)c.sel_total + 4, 0); // + 4: read as whole 32-bit words of four slots (stereo_rowlist_kernel)
        for (int l = 0; l < p.nlevels; l++)
            for (int k = 0; k < c.lv[l].sel_cap; k++) sl[c.lv[l].sel_off + k] = (uint8_t)l;
        P.slot_level.swap(sl);
    }
    {   // describe_kernel's processing order (orbfe_octree3.hip step 4a): a node's bin = row bits | root | column bits of its quadrant path,
        // rows ~40 px tall (a patch is 31 - 40 rows), the remaining bits of the 256 bins for columns
        c.proc_order = !knobs.no_proc_order && P.use_octree3 && !P.ot3_nodes_in_hbm;
        for (int l = 0; l < p.nlevels; l++) {
            LevelInfo &L = c.lv[l];
            const int region_h = (L.h - p.edge_threshold + 3) - c.min_border;
            int rb = 0;
            while (rb < 3 && (region_h >> (rb + 1)) >= 28) rb++; // rows of 28 - 55 px (measured: 20 / 40-px minima cost describe_kernel 1 us, 14 / 112 px 3 - 5 us)
            L.po_rb = rb; L.po_cb = 6 - rb;
        }
    }
    {   // circular patch of IC_Angle (src/ORBextractor.cc:79-96): |v| <= hp, |u| <= umax[|v|]
        std::vector<int16_t> uv;
        const int hp = p.half_patch_size;
        for (int v = -hp; v <= hp; v++) {
            const int d = c.umax[v < 0 ? -v : v];
            for (int u = -d; u <= d; u++) uv.push_back((int16_t)((u & 0xff) | ((v & 0xff) << 8)));
        }
        while (uv.size() % 64) uv.push_back(0);
        c.patch_n = (int)uv.size();
        P.patch_uv.swap(uv);
    }
    {   // the same patch as byte-dot-product weights for describe_kernel (hp == 15): lane = 2 * row + half holds the 16 pixels
        // u = -15 + 16 * half .. of row v = row - 15 as four words (its one 128-bit load of the raw patch); per lane 12 words:
        // [0..3] weights (u + 16) inside the circle else 0, [4..7] weights 1 / 0, [8] v (three 128-bit loads per lane).
        // Lanes 62 / 63 (no row 31) and u = 16 get zero weights.
        std::vector<uint32_t> mt(12 * 64, 0u);
        if (p.half_patch_size == 15)
            for (int lane = 0; lane < 62; lane++) {
                const int r = lane >> 1, half = lane & 1, v = r - 15, um = c.umax[v < 0 ? -v : v];
                for (int k = 0; k < 4; k++) {
                    uint32_t wu = 0, w1 = 0;
                    for (int j = 0; j < 4; j++) {
                        const int u = 16 * half + 4 * k + j - 15;
                        if (u >= -um && u <= um) { wu |= (uint32_t)(u + 16) << (8 * j); w1 |= 1u << (8 * j); }
                    }
                    mt[(size_t)lane * 12 + k] = wu;
                    mt[(size_t)lane * 12 + 4 + k] = w1;
                }
                mt[(size_t)lane * 12 + 8] = (uint32_t)v;
            }
        P.mom_tab.swap(mt);
    }
    // level 0 read in place: ORBFE_NO_INPLACE=1 keeps the ingest copy
    P.inplace_ok = !knobs.no_inplace && c.nlevels >= 2 && c.lv[1].rs_direct && c.tail_first != 1 && p.width >= 16 && p.height >= 8;
    if (knobs.host_trace) fprintf(stderr, "orbfe: level 0 of packed grey input: %s\n", P.inplace_ok ? "read in place (no ingest launch)" : "copied by ingest16_kernel");
    // FAST's level 0 on the side stream beside the pyramid's launches (run_chain): from 64 images, the batch of the headline step, where
    // it is + 3.0 to + 3.2 % (profiles/fast_split.json).  Forced on, 8 pairs per step lose 5 - 6 % and one pair 12 - 13 %, and nothing
    // between was measured, so the threshold is never below the batch from which every blur rides.  Several chains in flight lose too
    // (three chains of 64 pairs - 8 %): such callers set ORBFE_FAST_SPLIT=0.  =1 / =0: at every batch size / never
    P.fast_split_min_images = p.nlevels < 2 || knobs.fast_split == 0 ? INT_MAX : (knobs.fast_split == 1 ? 1 : std::max(64, P.blur_ride_min_images));
    P.host_trace = knobs.host_trace;
    return ORBFE_OK;
}
