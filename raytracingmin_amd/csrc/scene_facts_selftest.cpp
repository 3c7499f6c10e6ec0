// scene_facts_selftest.cpp — a stand-alone run of the scene proofs and the host grid builder (rtm_scene_facts.cpp) with the
// loader (rtm_scene.cpp), built with AddressSanitizer and UBSan by `make scene_facts_selftest_asan`
// (tests/test_scene_facts_asan.py).  No device, no library: the two units are linked into this program.
//
//   scene_facts_selftest_asan <directory of the shipped scenes>
//
// The cases are the smallest at which this code can go wrong: every shipped scene; 0 and 1 spheres; 32 and 33 (the axis rows'
// cap); 63 and 64 (the emit mask's); a NaN and an infinite centre; -0.0 coordinates on axis spheres; the Cornell box with one
// wall moved by one ulp (no pairs, a smaller shared-K group) and with one wall of radius 100 at 1e6 (outside the envelope); a
// plane's row; the grid builder at 63 and 64 spheres and on three 2 000-sphere stress scenes.  The expected words are
// constants: what the test hooks of the library answered BEFORE this code became a unit of its own (rtm_debug_scene_facts,
// rtm_debug_zero_term_facts, rtm_debug_axis_rows, rtm_debug_wall_pairs, rtm_debug_grid_build), with the axis rows and the
// grid's tables folded into an FNV-1a hash of their bytes.  The shared-K group has no hook: its expected value is the largest
// set of equal K among those axis rows (tests/_axis_disc_rays.py: shared_k_bits).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <limits>
#include <string>
#include <vector>

#include "rtm_scene_facts.h"

using namespace rtm;

static int g_failures = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            ++g_failures;                                   \
            std::printf("FAIL line %d: %s — ", __LINE__, #cond); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
        }                                                   \
    } while (0)

static uint64_t fnv(const void* p, size_t bytes, uint64_t h = 14695981039346656037ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

struct Expect {
    const char* name;
    int rc[4];  // scene_facts_host, zero_term_facts_host, axis_rows_host, wall_pairs_host
    uint64_t facts[2], zero_term[2], pairs[2], rows_hash;
    unsigned shared_k;
};
static const Expect kExpect[] = {
    {"cornellBoxSetting.json", {0, 0, 0, 0}, {0x3e96ull, 0x3ull}, {0x1ull, 0x1ull}, {0x1ull, 0x2aull}, 0x8b4b838ee41ea437ull, 0x7eu},
    {"settingData.json", {0, 0, 0, 0}, {0x12ull, 0x3ull}, {0x1ull, 0x1ull}, {0x0ull, 0x0ull}, 0xca63965ee6147e0aull, 0x0u},
    {"simpleSetting1.json", {0, 0, 0, 0}, {0x294ull, 0x2ull}, {0x0ull, 0xffffffffffffffffull}, {0x0ull, 0x0ull}, 0xaa66215a50a41a2eull, 0x6u},
    {"simpleSetting2.json", {0, 0, 0, 0}, {0x14ull, 0x2ull}, {0x0ull, 0xffffffffffffffffull}, {0x0ull, 0x0ull}, 0x901ced129e1d9aa5ull, 0x6u},
    {"synthetic 0", {0, 0, 0, 0}, {0x0ull, 0x3ull}, {0x1ull, 0x0ull}, {0x0ull, 0x0ull}, 0xcbf29ce484222325ull, 0x0u},
    {"synthetic 1", {0, 0, 0, 0}, {0x1ull, 0x3ull}, {0x1ull, 0x0ull}, {0x0ull, 0x0ull}, 0xc4accb41fc1bbfcbull, 0x0u},
    {"synthetic 32", {0, 0, 0, 0}, {0x2525252525252525ull, 0x3ull}, {0x1ull, 0x80000000ull}, {0x0ull, 0x0ull}, 0x8f425f3bae47e588ull, 0x3u},
    {"synthetic 33", {0, 0, -1, -1}, {0x2525252525252525ull, 0x3ull}, {0x1ull, 0x100000000ull}, {0x0ull, 0x0ull}, 0x0ull, 0x0u},
    {"synthetic 63", {0, 0, -1, -1}, {0x2525252525252525ull, 0x3ull}, {0x1ull, 0x4000000000000000ull}, {0x0ull, 0x0ull}, 0x0ull, 0x0u},
    {"synthetic 64", {0, 0, -1, -1}, {0x2525252525252525ull, 0x3ull}, {0x0ull, 0xffffffffffffffffull}, {0x0ull, 0x0ull}, 0x0ull, 0x0u},
    {"nan centre", {0, 0, 0, 0}, {0x124ull, 0x1ull}, {0x1ull, 0x10ull}, {0x0ull, 0x0ull}, 0x13309a15bfab6194ull, 0x0u},
    {"infinite centre", {0, 0, 0, 0}, {0x105ull, 0x1ull}, {0x1ull, 0x10ull}, {0x0ull, 0x0ull}, 0x5c1e3ece8f340c32ull, 0x3u},
    {"negative zeros", {0, 0, 0, 0}, {0x125ull, 0x3ull}, {0x1ull, 0x10ull}, {0x0ull, 0x0ull}, 0xecc285524a937d3aull, 0x3u},
    {"cornell one ulp", {0, 0, 0, 0}, {0x3e96ull, 0x3ull}, {0x1ull, 0x1ull}, {0x0ull, 0x0ull}, 0xb518a24e621b0044ull, 0x7cu},
    {"cornell far wall", {0, 0, 0, 0}, {0x3e96ull, 0x3ull}, {0x1ull, 0x1ull}, {0x0ull, 0x0ull}, 0xd6bf5acc0e2599c7ull, 0x7cu},
};
// scene_load_json's answer for every file of the scenes directory that holds no sphere scene
static const struct {
    const char* name;
    int rc;
} kRefused[] = {{"planeRoom.json", RTM_ERR_INVALID_SCENE}};

struct GridExpect {
    uint64_t seed;
    size_t n;
    int rc;
    uint64_t info[6];  // cells, records, big, dim x, y, z
    uint64_t hash;     // pads, ranges, items, big, then info[6..11] (lo, h, reach, t_ok as bits)
};
static const GridExpect kGridExpect[] = {
    {1, 63, -8, {0, 0, 0, 0, 0, 0}, 0x0ull},
    {1, 64, 0, {125, 91, 0, 5, 5, 5}, 0x7bb67378d0b3d22dull},
    {1, 2000, 0, {3375, 4173, 0, 15, 15, 15}, 0x1e834dd4bfca1cc9ull},
    {2, 2000, 0, {3375, 4079, 0, 15, 15, 15}, 0xa739174618d1d274ull},
    {3, 2000, 0, {3375, 4121, 0, 15, 15, 15}, 0x3e18d3ea963cbc9eull},
};

// Sphere i of the synthetic scenes: a +c / -c pair on x, one on y, one off the axes, and so on; the last one is a black light
static std::vector<rtm_sphere> synthetic(size_t n) {
    std::vector<rtm_sphere> sp(n);
    for (size_t i = 0; i < n; ++i) {
        rtm_sphere& s = sp[i];
        std::memset(&s, 0, sizeof s);
        const double d = (double)i;
        switch (i % 4) {
            case 0: s.center[0] = 4.0 + d; s.radius = 1.0f; break;
            case 1: s.center[0] = -(4.0 + (d - 1.0)); s.radius = 1.0f; break;
            case 2: s.center[1] = 3.0 + d; s.radius = 0.5f; break;
            default: s.center[0] = d; s.center[1] = 1.0; s.center[2] = -d; s.radius = 0.25f * (float)(1 + i % 3); break;
        }
        const bool light = i == n - 1 && n > 1;
        const double col[3] = {0.25, 0.5, 0.75};
        for (int k = 0; k < 3; ++k) {
            s.color[k] = light ? 0.0 : col[k];
            s.emission[k] = light ? 5.0 : 0.0;
        }
    }
    return sp;
}

// The four small hooks against the constants, then scene_facts — what a scene object gets — against the hooks.
static void check_case(const char* name, const std::vector<rtm_sphere>& sp, double* reach_out = nullptr) {
    const Expect* e = nullptr;
    for (const Expect& x : kExpect)
        if (std::strcmp(x.name, name) == 0) e = &x;
    CHECK(e != nullptr, "%s has no expected values", name);
    if (!e) return;
    const size_t n = sp.size();
    const rtm_sphere* p = n ? sp.data() : nullptr;
    uint64_t facts[2] = {0, 0}, zt[2] = {0, 0}, pairs[2] = {0, 0};
    std::vector<double> rows(4 * std::max<size_t>(n, 1), -1.0);
    const int rc[4] = {scene_facts_host(p, n, facts), zero_term_facts_host(p, n, zt), axis_rows_host(p, n, rows.data()),
                       wall_pairs_host(p, n, pairs)};
    for (int k = 0; k < 4; ++k) CHECK(rc[k] == e->rc[k], "%s: hook %d returns %d, not %d", name, k, rc[k], e->rc[k]);
    for (int k = 0; k < 2; ++k) {
        CHECK(facts[k] == e->facts[k], "%s: facts[%d] = 0x%llx", name, k, (unsigned long long)facts[k]);
        CHECK(zt[k] == e->zero_term[k], "%s: zero-term facts[%d] = 0x%llx", name, k, (unsigned long long)zt[k]);
        CHECK(pairs[k] == e->pairs[k], "%s: wall-pair facts[%d] = 0x%llx", name, k, (unsigned long long)pairs[k]);
    }
    if (rc[2] == RTM_OK) {
        const uint64_t h = fnv(rows.data(), n * 4 * sizeof(double));
        CHECK(h == e->rows_hash, "%s: the axis rows hash to 0x%llx", name, (unsigned long long)h);
    }

    std::vector<double> geom, mat, surf;
    flatten_scene(p, n, geom, mat, &surf);
    CHECK(geom.size() == n * 4 && mat.size() == (n + 1) * 8 && surf.size() == std::max<size_t>(n, 1) * 4, "%s: table sizes", name);
    geom.resize((n + axis_row_count(n)) * 4);  // as scene_build_host lays them out
    const SceneFacts f = scene_facts(geom.data(), mat.data(), n, geom.data() + n * 4);
    CHECK(f.axis_pat == facts[0], "%s: axis_pat 0x%llx", name, (unsigned long long)f.axis_pat);
    CHECK((f.fold_flags & 3u) == facts[1], "%s: fold_flags 0x%x", name, f.fold_flags);
    CHECK(((f.fold_flags & kFoldZeroTermSkippable) != 0u) == (zt[0] == 1), "%s: fold_flags 0x%x", name, f.fold_flags);
    CHECK(f.emit_mask == zt[1], "%s: emit_mask 0x%llx", name, (unsigned long long)f.emit_mask);
    double reach = 0.0;
    if (rc[2] == RTM_OK) {
        CHECK(((f.fold_flags & kSceneWallPairs) != 0u) == (pairs[0] == 1), "%s: fold_flags 0x%x", name, f.fold_flags);
        CHECK(((f.fold_flags >> kSceneSharedKShift) & kSceneSharedKMask) == e->shared_k, "%s: fold_flags 0x%x", name, f.fold_flags);
        CHECK(n == 0 || std::memcmp(geom.data() + n * 4, rows.data(), n * 4 * sizeof(double)) == 0, "%s: scene_facts' axis rows differ", name);
        for (size_t i = 0; i < n; ++i) reach = std::max(reach, rows[i * 4 + 3]);
        const unsigned bits = (f.fold_flags >> kSceneAxisReachShift) & kSceneAxisReachMask;
        CHECK(reach == (bits ? std::ldexp(1.0, (int)bits - 128) : 0.0), "%s: reach bits %u, rows say %g", name, bits, reach);
    } else {
        CHECK((f.fold_flags & ~7u) == 0u, "%s: a scene without axis rows has fold_flags 0x%x", name, f.fold_flags);
    }
    if (reach_out) *reach_out = reach;
}

// The invariants tests/test_host_io.py checks on a grid: the ranges are monotone and cover `items`, each cell's list ascends,
// the big list ascends, every small sphere is listed in the cell that holds its centre.
static void check_grid(const char* name, const double* geom, size_t n, const double lo[3], double h, const uint64_t dim[3],
                       const std::vector<uint32_t>& ranges, const std::vector<uint32_t>& items, size_t refs,
                       const std::vector<int32_t>& big) {
    const size_t cells = dim[0] * dim[1] * dim[2];
    CHECK(ranges.size() == cells * 2 && cells > 0, "%s: %zu ranges for %zu cells", name, ranges.size() / 2, cells);
    if (ranges.size() != cells * 2 || !cells) return;
    CHECK(ranges[0] == 0 && ranges[cells * 2 - 1] == refs, "%s: the ranges do not cover the items", name);
    std::vector<char> is_big(n, 0);
    for (size_t j = 0; j < big.size(); ++j) {
        CHECK(big[j] >= 0 && (size_t)big[j] < n && (j == 0 || big[j] > big[j - 1]), "%s: big[%zu] = %d", name, j, big[j]);
        if (big[j] >= 0 && (size_t)big[j] < n) is_big[big[j]] = 1;
    }
    for (size_t c = 0; c < cells; ++c) {
        const uint32_t a = ranges[c * 2], b = ranges[c * 2 + 1];
        CHECK(a <= b && b <= refs && (c == 0 || a == ranges[c * 2 - 1]), "%s: cell %zu has range [%u, %u)", name, c, a, b);
        if (!(a <= b && b <= refs)) return;
        for (uint32_t k = a; k < b; ++k)
            CHECK(items[k] < n && !is_big[items[k] < n ? items[k] : 0] && (k == a || items[k] > items[k - 1]),
                  "%s: cell %zu lists %u at %u", name, c, items[k], k);
    }
    for (size_t i = 0; i < n; ++i) {
        if (is_big[i]) continue;
        size_t cell[3];
        bool inside = true;
        for (int k = 0; k < 3; ++k) {
            const double q = std::floor((geom[i * 4 + k] - lo[k]) / h);
            inside = inside && q >= 0.0 && q < (double)dim[k];
            cell[k] = inside ? (size_t)q : 0;
        }
        CHECK(inside, "%s: sphere %zu's centre lies outside the grid", name, i);
        if (!inside) continue;
        const size_t c = (cell[2] * dim[1] + cell[1]) * dim[0] + cell[0];
        const uint32_t* first = items.data() + ranges[c * 2];
        const uint32_t* last = items.data() + ranges[c * 2 + 1];
        CHECK(std::binary_search(first, last, (uint32_t)i), "%s: sphere %zu is not listed in its centre's cell", name, i);
    }
}

static void check_grid_case(const GridExpect& e) {
    char name[64];
    std::snprintf(name, sizeof name, "grid of %zu stress spheres, seed %llu", e.n, (unsigned long long)e.seed);
    rtm_settings st;
    std::vector<rtm_sphere> sp(e.n);
    CHECK(scene_make_stress(e.seed, e.n, &st, sp.data()) == RTM_OK, "%s", name);
    uint64_t info[12] = {0};
    std::vector<double> pads(e.n);
    int rc = grid_build_host(sp.data(), e.n, info, pads.data(), nullptr, 0, nullptr, 0, nullptr, 0);
    CHECK(rc == e.rc, "%s: returns %d, not %d", name, rc, e.rc);
    if (rc != RTM_OK) {
        CHECK(std::strlen(last_error()) > 0, "%s: no message", name);
        return;
    }
    for (int k = 0; k < 6; ++k) CHECK(info[k] == e.info[k], "%s: info[%d] = %llu", name, k, (unsigned long long)info[k]);
    const size_t cells = info[0], refs = info[1], n_big = info[2];
    std::vector<uint32_t> ranges(cells * 2), items(std::max<size_t>(refs, 1));
    std::vector<int32_t> big(std::max<size_t>(n_big, 1));
    // one entry short: refused, and nothing is written past the end
    if (refs > 0) {
        rc = grid_build_host(sp.data(), e.n, info, pads.data(), ranges.data(), ranges.size(), items.data(), refs - 1, big.data(), n_big);
        CHECK(rc == RTM_ERR_CAPACITY, "%s: a short items buffer returns %d", name, rc);
    }
    rc = grid_build_host(sp.data(), e.n, info, pads.data(), ranges.data(), ranges.size(), items.data(), refs, big.data(), n_big);
    CHECK(rc == RTM_OK, "%s: returns %d with buffers", name, rc);
    big.resize(n_big);
    uint64_t h = fnv(pads.data(), pads.size() * sizeof(double));
    h = fnv(ranges.data(), ranges.size() * sizeof(uint32_t), h);
    h = fnv(items.data(), refs * sizeof(uint32_t), h);
    h = fnv(big.data(), big.size() * sizeof(int32_t), h);
    h = fnv(info + 6, 6 * sizeof(uint64_t), h);
    CHECK(h == e.hash, "%s: the tables hash to 0x%llx", name, (unsigned long long)h);
    std::vector<double> geom, mat;
    flatten_scene(sp.data(), e.n, geom, mat);
    double d[4];
    std::memcpy(d, info + 6, sizeof d);  // lo x, y, z, h
    check_grid(name, geom.data(), e.n, d, d[3], info + 3, ranges, items, refs, big);
}

// A plane's geometry row has a negative "r*r" (rtm_kernels.hip: scene_create_objects).  Expected by hand, there being no
// host hook that takes planes: the plane at (0, 0, 5) gets no axis although only z is non-zero, the sphere at (0, 2, 0) gets
// y; both are diffuse and dark, within 6 of the origin, and the one axis sphere (r = 1) allows a reach of
// sqrt(2^46 x 1e-5f) = 26 527, so 2^14.
static void check_plane_rows(const std::string& scenes) {
    double geom[4 * 4] = {0.0, 0.0, 5.0, -1.0, 0.0, 2.0, 0.0, 1.0};  // two geometry rows, room for two axis rows
    double mat[3 * 8] = {0.5, 1.0, 0.25, 0, 0, 0, 0.5, 0.5 * 16777216.0, 1.0, 0.5, 0.5, 0, 0, 0, 0.75, 0.75 * 16777216.0, 1, 1, 1};
    const SceneFacts f = scene_facts(geom, mat, 2, geom + 8);
    CHECK(f.axis_pat == (2ull << 2), "plane row: axis_pat 0x%llx", (unsigned long long)f.axis_pat);
    const unsigned want = kFoldNoLevelEmission | kSceneCompact | kFoldZeroTermSkippable | ((128u + 14u) << kSceneAxisReachShift);
    CHECK(f.fold_flags == want, "plane row: fold_flags 0x%x, not 0x%x", f.fold_flags, want);
    CHECK(f.emit_mask == 0, "plane row: emit_mask 0x%llx", (unsigned long long)f.emit_mask);
    const double rows[8] = {0, 0, 0, 0, 2.0, -4.0, 3.0, 16384.0};
    CHECK(std::memcmp(geom + 8, rows, sizeof rows) == 0, "plane row: axis rows (%g, %g, %g, %g)", geom[12], geom[13], geom[14], geom[15]);

    // png::PlaneObject's rows of the shipped scene with planes: finite, and the two squared half-extents are those of the rows
    rtm_settings st;
    std::vector<rtm_object> objs(64);
    size_t n = 0;
    const int rc = scene_load_json_objects((scenes + "/planeRoom.json").c_str(), 0, &st, objs.data(), objs.size(), &n);
    CHECK(rc == RTM_OK && n > 0 && n <= objs.size(), "planeRoom.json: returns %d (%s)", rc, last_error());
    size_t planes = 0;
    for (size_t i = 0; rc == RTM_OK && i < n; ++i) {
        if (objs[i].type != RTM_OBJECT_PLANE) continue;
        ++planes;
        double row[16];
        plane_row(objs[i], row);
        for (int k = 0; k < 16; ++k) CHECK(std::isfinite(row[k]), "planeRoom.json: object %zu, row[%d] = %g", i, k, row[k]);
        CHECK(row[12] == row[6] * row[6] + row[7] * row[7] + row[8] * row[8] && row[13] == row[9] * row[9] + row[10] * row[10] + row[11] * row[11],
              "planeRoom.json: object %zu's half-extents", i);
    }
    CHECK(planes > 0, "planeRoom.json holds no plane");

    // the grid builder with a plane among 64 spheres: the plane is in the list every ray tests, the lists hold the spheres
    rtm_sphere sp[64];
    CHECK(scene_make_stress(1, 64, &st, sp) == RTM_OK, "stress scene");
    std::vector<double> g, m;
    flatten_scene(sp, 64, g, m);
    const double plane[4] = {0.0, -60.0, 0.0, -1.0};
    g.insert(g.begin() + 4 * 10, plane, plane + 4);  // object 10 of 65
    GridBuild B;
    std::vector<double> pads(65);
    const bool made = make_grid(g.data(), 65, B, pads.data());
    CHECK(made, "64 spheres and a plane get no grid");
    if (made) {
        CHECK(B.big.size() == 1 && B.big[0] == 10, "the plane is not the one big object");
        const size_t cells = B.cell_start.size() - 1;
        std::vector<uint32_t> ranges(cells * 2);
        for (size_t c = 0; c < cells; ++c) {
            ranges[c * 2] = B.cell_start[c];
            ranges[c * 2 + 1] = B.cell_start[c + 1];
        }
        const uint64_t dim[3] = {(uint64_t)B.hdr.dim[0], (uint64_t)B.hdr.dim[1], (uint64_t)B.hdr.dim[2]};
        check_grid("64 spheres and a plane", g.data(), 65, B.hdr.lo, B.hdr.h, dim, ranges,
                   std::vector<uint32_t>(B.items.begin(), B.items.end()), B.refs, std::vector<int32_t>(B.big.begin(), B.big.end()));
        const GridLayout lay = grid_layout(cells, B.items.size(), B.big.size());
        CHECK(lay.off_cs % 256 == 0 && lay.off_items % 256 == 0 && lay.off_big % 256 == 0 && lay.bytes > lay.off_big, "grid_layout");
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s <directory of the shipped scenes>\n", argv[0]);
        return 2;
    }
    const std::string scenes = argv[1];
    std::vector<std::string> files;
    for (const auto& entry : std::filesystem::directory_iterator(scenes))
        if (entry.path().extension() == ".json") files.push_back(entry.path().filename().string());
    std::sort(files.begin(), files.end());
    CHECK(files.size() >= 5, "%zu scenes in %s", files.size(), scenes.c_str());
    std::vector<rtm_sphere> cornell;
    size_t sphere_scenes = 0;
    for (const std::string& name : files) {
        rtm_settings st;
        std::vector<rtm_sphere> sp(64);
        size_t n = 0;
        const int rc = scene_load_json((scenes + "/" + name).c_str(), 0, &st, sp.data(), sp.size(), &n);
        bool refused = false;
        for (const auto& r : kRefused)
            if (name == r.name) {
                refused = true;
                CHECK(rc == r.rc, "%s: scene_load_json returns %d, not %d", name.c_str(), rc, r.rc);
            }
        if (refused) continue;
        CHECK(rc == RTM_OK && n <= sp.size(), "%s: scene_load_json returns %d (%s)", name.c_str(), rc, last_error());
        if (rc != RTM_OK) continue;
        sp.resize(n);
        check_case(name.c_str(), sp);
        ++sphere_scenes;
        if (name == "cornellBoxSetting.json") cornell = sp;
    }
    CHECK(sphere_scenes >= 4, "%zu sphere scenes checked", sphere_scenes);

    for (size_t n : {0, 1, 32, 33, 63, 64}) {
        char name[32];
        std::snprintf(name, sizeof name, "synthetic %zu", n);
        check_case(name, synthetic(n));
    }
    {
        std::vector<rtm_sphere> sp = synthetic(5);
        sp[0].center[0] = std::numeric_limits<double>::quiet_NaN();
        check_case("nan centre", sp);
        sp = synthetic(5);
        sp[2].center[1] = std::numeric_limits<double>::infinity();
        check_case("infinite centre", sp);
        sp = synthetic(5);
        sp[0].center[1] = sp[0].center[2] = sp[2].center[0] = -0.0;
        check_case("negative zeros", sp);
    }
    CHECK(cornell.size() == 7 && cornell[1].center[0] == 10010.0, "the Cornell box is not the scene the cases below vary");
    if (cornell.size() == 7) {
        double reach = 0.0;
        check_case("cornellBoxSetting.json", cornell, &reach);
        CHECK(reach > 0.0, "the Cornell box is inside no envelope");
        std::vector<rtm_sphere> sp = cornell;  // wall 1 one ulp farther out: no partner for wall 2, another K
        sp[1].center[0] = std::nextafter(sp[1].center[0], std::numeric_limits<double>::infinity());
        check_case("cornell one ulp", sp, &reach);
        CHECK(reach > 0.0, "one ulp takes the Cornell box out of the envelope");
        sp = cornell;  // wall 1 as a sphere of radius 100 at 1e6: it could hit itself
        sp[1].center[0] = 1e6;
        sp[1].radius = 100.0f;
        check_case("cornell far wall", sp, &reach);
        CHECK(reach == 0.0, "a sphere of radius 100 at 1e6 is inside an envelope of %g", reach);
    }
    check_plane_rows(scenes);
    for (const GridExpect& e : kGridExpect) check_grid_case(e);

    if (g_failures) {
        std::printf("scene facts selftest: %d checks FAILED\n", g_failures);
        return 1;
    }
    std::printf("scene facts selftest ok\n");
    return 0;
}
