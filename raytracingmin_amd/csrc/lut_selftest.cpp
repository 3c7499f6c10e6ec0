// lut_selftest.cpp — a stand-alone run of the grade's host-only code: the .cube reader and the white balance matrix
// (rtm_lut.cpp, with rtm_scene.cpp for the last-error text) and the LUT's index arithmetic (rtm_grade_index.h, the function
// the kernel compiles), built with AddressSanitizer and UBSan by `make lut_selftest_asan` (tests/test_lut_asan.py).  No
// device, no library: the units are linked into this program.
//
//   lut_selftest_asan <a directory to write temporary files into>
//
// The cases: well-formed files (N = 2, 3, 17; comments, blank lines, CR LF, a title, both domain spellings), read back bit
// for bit, with the size query and a too-small table; every malformed family of include/rtm.h with its line number; a valid
// file cut at every byte of its first 200 (each cut has too few rows and is refused, and reads nothing past its end); the
// file loader on a written file and on a missing one; the white balance matrix at the published chromaticities' temperatures
// and its range refusals; gr_lut_index on 0, -0, denormals, N - 1, N - 1 +- 1 ulp, +-3.4e38, +-inf, NaN and a sweep, for
// every N in 2..256: 0 <= i <= N - 2 and 0 <= f <= 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rtm_grade_index.h"
#include "rtm_internal.h"

using namespace rtm;

static int g_failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            ++g_failures;                                        \
            std::printf("FAIL line %d: %s — ", __LINE__, #cond); \
            std::printf(__VA_ARGS__);                            \
            std::printf("\n");                                   \
        }                                                        \
    } while (0)

// entry (r, g, b), channel c of the test table: distinct, exactly representable values
static float entry(int n, int r, int g, int b, int c) { return (float)(c + 3 * (r + n * (g + n * b))) / 4096.0f - 0.25f; }

static std::string cube_text(int n, const char* eol, bool decorate) {
    std::string s;
    char buf[160];
    if (decorate) {
        s += std::string("# a comment") + eol + eol + "TITLE \"a look # with a hash\"" + eol;
        s += std::string("  \t") + eol;
    }
    std::snprintf(buf, sizeof buf, "LUT_3D_SIZE %d%s", n, eol);
    s += buf;
    if (decorate) s += std::string("DOMAIN_MIN -0.25 0 0.5") + eol + "DOMAIN_MAX 4 1.0 1.5e0" + eol + "# the table" + eol;
    for (int b = 0; b < n; ++b)
        for (int g = 0; g < n; ++g)
            for (int r = 0; r < n; ++r) {
                std::snprintf(buf, sizeof buf, "%.9g %.9g\t%.9g%s", (double)entry(n, r, g, b, 0), (double)entry(n, r, g, b, 1),
                              (double)entry(n, r, g, b, 2), eol);
                s += buf;
            }
    return s;
}

struct Parsed {
    int rc;
    int32_t size;
    float lo[3], hi[3];
    std::vector<float> table;
    std::string detail;
};

// the size query, then the load into a table of exactly that size
static Parsed parse(const std::string& text) {
    Parsed p;
    p.size = -1;
    p.rc = lut_parse_cube(text.data(), text.size(), &p.size, p.lo, p.hi, nullptr, 0);
    p.detail = last_error();
    if (p.rc != RTM_OK) return p;
    p.table.resize((size_t)3 * p.size * p.size * p.size);
    p.rc = lut_parse_cube(text.data(), text.size(), &p.size, p.lo, p.hi, p.table.data(), p.table.size());
    p.detail = last_error();
    return p;
}

static void well_formed() {
    const int sizes[] = {2, 3, 17};
    for (const int n : sizes)
        for (int form = 0; form < 3; ++form) {
            const std::string text = cube_text(n, form == 2 ? "\r\n" : "\n", form != 0);
            const Parsed p = parse(text);
            CHECK(p.rc == RTM_OK && p.size == n, "n %d form %d: rc %d size %d (%s)", n, form, p.rc, p.size, p.detail.c_str());
            if (p.rc != RTM_OK) continue;
            const float lo[3] = {form ? -0.25f : 0.0f, 0.0f, form ? 0.5f : 0.0f}, hi[3] = {form ? 4.0f : 1.0f, 1.0f, form ? 1.5f : 1.0f};
            CHECK(std::memcmp(p.lo, lo, sizeof lo) == 0 && std::memcmp(p.hi, hi, sizeof hi) == 0, "n %d form %d: domain", n, form);
            size_t bad = 0;
            for (int b = 0; b < n; ++b)
                for (int g = 0; g < n; ++g)
                    for (int r = 0; r < n; ++r)
                        for (int c = 0; c < 3; ++c) {
                            const float want = entry(n, r, g, b, c), got = p.table[(size_t)3 * (r + n * (g + n * b)) + c];
                            bad += std::memcmp(&want, &got, sizeof want) != 0;
                        }
            CHECK(bad == 0, "n %d form %d: %zu entries differ", n, form, bad);
            // a table one float short: the size and the domain are set, nothing is written past the capacity
            std::vector<float> small((size_t)3 * n * n * n - 1);
            int32_t size = -1;
            float dlo[3], dhi[3];
            const int rc = lut_parse_cube(text.data(), text.size(), &size, dlo, dhi, small.data(), small.size());
            CHECK(rc == RTM_ERR_CAPACITY && size == n, "n %d form %d: short table rc %d size %d", n, form, rc, size);
        }
    // LUT_3D_INPUT_RANGE sets all three channels; no end of line after the last row
    const Parsed p = parse("LUT_3D_INPUT_RANGE -1 2\nLUT_3D_SIZE 2\n0 0 0\n1 0 0\n0 1 0\n1 1 0\n0 0 1\n1 0 1\n0 1 1\n1 1 1");
    CHECK(p.rc == RTM_OK && p.size == 2 && p.lo[0] == -1.0f && p.lo[2] == -1.0f && p.hi[1] == 2.0f, "input range: rc %d (%s)", p.rc,
          p.detail.c_str());
}

static void malformed() {
    const std::string rows8 = "0 0 0\n1 0 0\n0 1 0\n1 1 0\n0 0 1\n1 0 1\n0 1 1\n1 1 1\n";
    const struct {
        const char* name;
        std::string text;
        int rc;
        const char* line;  // the detail begins with it
    } cases[] = {
        {"unknown keyword", "LUT_3D_SIZE 2\nLUT_3D_FOO 1\n" + rows8, RTM_ERR_PARSE, "line 2:"},
        {"size 1", "LUT_3D_SIZE 1\n0 0 0\n", RTM_ERR_PARSE, "line 1:"},
        {"size 257", "# c\nLUT_3D_SIZE 257\n", RTM_ERR_PARSE, "line 2:"},
        {"size 2.5", "LUT_3D_SIZE 2.5\n" + rows8, RTM_ERR_PARSE, "line 1:"},
        {"size twice", "LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n" + rows8, RTM_ERR_PARSE, "line 2:"},
        {"size with two numbers", "LUT_3D_SIZE 2 2\n" + rows8, RTM_ERR_PARSE, "line 1:"},
        {"too few rows", "LUT_3D_SIZE 2\n0 0 0\n1 0 0\n", RTM_ERR_PARSE, "line 3:"},
        {"too many rows", "LUT_3D_SIZE 2\n" + rows8 + "0 0 0\n", RTM_ERR_PARSE, "line 10:"},
        {"not a number", "LUT_3D_SIZE 2\n0 0 0\n1 zero 0\n", RTM_ERR_PARSE, "line 3:"},
        {"hex", "LUT_3D_SIZE 2\n0x1 0 0\n", RTM_ERR_PARSE, "line 2:"},
        {"nan", "LUT_3D_SIZE 2\n0 nan 0\n", RTM_ERR_PARSE, "line 2:"},
        {"inf", "LUT_3D_SIZE 2\n0 0 inf\n", RTM_ERR_PARSE, "line 2:"},
        {"overflow", "LUT_3D_SIZE 2\n0 0 1e39\n", RTM_ERR_PARSE, "line 2:"},
        {"two numbers", "LUT_3D_SIZE 2\n0 0\n", RTM_ERR_PARSE, "line 2:"},
        {"four numbers", "LUT_3D_SIZE 2\n0 0 0 0\n", RTM_ERR_PARSE, "line 2:"},
        {"max <= min", "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 0 1\n" + rows8, RTM_ERR_PARSE, "line 3:"},
        {"range max <= min", "LUT_3D_INPUT_RANGE 1 1\nLUT_3D_SIZE 2\n" + rows8, RTM_ERR_PARSE, "line 1:"},
        {"domain not finite", "LUT_3D_SIZE 2\nDOMAIN_MAX 1 inf 1\n" + rows8, RTM_ERR_PARSE, "line 2:"},
        {"domain two numbers", "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0\n" + rows8, RTM_ERR_PARSE, "line 2:"},
        {"data before size", "0 0 0\nLUT_3D_SIZE 2\n" + rows8, RTM_ERR_PARSE, "line 1:"},
        {"keyword inside the table", "LUT_3D_SIZE 2\n0 0 0\nDOMAIN_MIN 0 0 0\n", RTM_ERR_PARSE, "line 3:"},
        {"no size", "# nothing\nTITLE \"x\"\n", RTM_ERR_PARSE, "line 2:"},
        {"empty", "", RTM_ERR_PARSE, "line 0:"},
        {"1D", "LUT_1D_SIZE 16\n", RTM_ERR_UNSUPPORTED, "line 1:"},
        {"1D range", "TITLE \"t\"\nLUT_1D_INPUT_RANGE 0 1\n", RTM_ERR_UNSUPPORTED, "line 2:"},
    };
    for (const auto& c : cases) {
        const Parsed p = parse(c.text);
        CHECK(p.rc == c.rc, "%s: rc %d, want %d (%s)", c.name, p.rc, c.rc, p.detail.c_str());
        CHECK(p.detail.compare(0, std::strlen(c.line), c.line) == 0, "%s: detail \"%s\" does not begin with \"%s\"", c.name,
              p.detail.c_str(), c.line);
    }
    // an embedded NUL is no number; null arguments
    const std::string nul = std::string("LUT_3D_SIZE 2\n0 0") + '\0' + " 0\n";
    CHECK(parse(nul).rc == RTM_ERR_PARSE, "embedded NUL");
    int32_t size = 0;
    float lo[3], hi[3], one = 0.0f;
    CHECK(lut_parse_cube(nullptr, 4, &size, lo, hi, nullptr, 0) == RTM_ERR_INVALID_ARGUMENT, "null text");
    CHECK(lut_parse_cube("x", 1, nullptr, lo, hi, nullptr, 0) == RTM_ERR_INVALID_ARGUMENT, "null size");
    CHECK(lut_parse_cube("x", 1, &size, nullptr, hi, nullptr, 0) == RTM_ERR_INVALID_ARGUMENT, "null domain_min");
    CHECK(lut_parse_cube("x", 1, &size, lo, nullptr, nullptr, 0) == RTM_ERR_INVALID_ARGUMENT, "null domain_max");
    CHECK(lut_parse_cube("x", 1, &size, lo, hi, nullptr, 3) == RTM_ERR_INVALID_ARGUMENT, "null table with a capacity");
    CHECK(lut_parse_cube("LUT_3D_SIZE 2\n", 14, &size, lo, hi, &one, 0) == RTM_ERR_PARSE, "too few rows come before the capacity");
}

// a valid file cut at every byte of its first 200: a cut is accepted or refused, and reads nothing it should not (the text is
// copied into a buffer of exactly its length, so that the sanitizer sees a read past the cut)
static void truncations() {
    const std::string text = cube_text(3, "\r\n", true);
    CHECK(text.size() > 200, "the file is %zu bytes", text.size());
    for (size_t cut = 0; cut <= 200 && cut <= text.size(); ++cut) {
        std::vector<char> copy(text.begin(), text.begin() + cut);
        int32_t size = -1;
        float lo[3], hi[3];
        std::vector<float> table(81);
        const int rc = lut_parse_cube(copy.data(), copy.size(), &size, lo, hi, table.data(), table.size());
        CHECK(rc == RTM_ERR_PARSE, "cut at %zu: rc %d (a file of 27 rows cut inside its first 200 bytes has too few)", cut, rc);
    }
}

static void files(const std::string& dir) {
    const std::string path = dir + "/lut_selftest.cube", text = cube_text(3, "\n", true);
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != nullptr, "cannot write %s", path.c_str());
    if (!f) return;
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    int32_t size = -1;
    float lo[3], hi[3];
    std::vector<float> table(81);
    CHECK(lut_load_cube(path.c_str(), &size, lo, hi, nullptr, 0) == RTM_OK && size == 3, "size query of the file");
    CHECK(lut_load_cube(path.c_str(), &size, lo, hi, table.data(), table.size()) == RTM_OK, "load of the file");
    CHECK(table[80] == entry(3, 2, 2, 2, 2) && lo[0] == -0.25f && hi[2] == 1.5f, "the file's last entry and domain");
    std::remove(path.c_str());
    CHECK(lut_load_cube(path.c_str(), &size, lo, hi, nullptr, 0) == RTM_ERR_IO, "a missing file");
    CHECK(lut_load_cube(nullptr, &size, lo, hi, nullptr, 0) == RTM_ERR_INVALID_ARGUMENT, "a null path");
}

static void white_balance() {
    float m[9];
    // D65's own temperature on Kang's locus is close to, not exactly, D65: the matrix is near the identity
    CHECK(grade_white_balance(6504.0f, 0.0f, m) == RTM_OK, "6504 K");
    for (int k = 0; k < 9; ++k) CHECK(std::fabs(m[k] - (k % 4 == 0 ? 1.0f : 0.0f)) < 0.05f, "6504 K: m[%d] = %g", k, (double)m[k]);
    // a warm source is brought to white by lifting blue against red
    CHECK(grade_white_balance(2856.0f, 0.0f, m) == RTM_OK && m[8] > 1.5f && m[0] < 1.0f, "2856 K: m[0] %g m[8] %g", (double)m[0], (double)m[8]);
    const float ok_k[] = {1667.0f, 2222.0f, 4000.0f, 4001.0f, 25000.0f}, ok_t[] = {-0.05f, 0.0f, 0.03f, 0.05f};
    for (const float k : ok_k)
        for (const float t : ok_t) {
            CHECK(grade_white_balance(k, t, m) == RTM_OK, "%g K tint %g", (double)k, (double)t);
            for (int i = 0; i < 9; ++i) CHECK(std::isfinite(m[i]), "%g K tint %g: m[%d]", (double)k, (double)t, i);
        }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float bad_k[] = {1666.0f, 25001.0f, 0.0f, -5000.0f, nan, inf, -inf};
    for (const float k : bad_k) CHECK(grade_white_balance(k, 0.0f, m) == RTM_ERR_INVALID_ARGUMENT, "kelvin %g", (double)k);
    const float bad_t[] = {-0.051f, 0.051f, nan, inf, -inf};
    for (const float t : bad_t) CHECK(grade_white_balance(5000.0f, t, m) == RTM_ERR_INVALID_ARGUMENT, "tint %g", (double)t);
    CHECK(grade_white_balance(5000.0f, 0.0f, nullptr) == RTM_ERR_INVALID_ARGUMENT, "null matrix_out");
}

static void lut_index() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float den = std::numeric_limits<float>::denorm_min(), tiny = std::numeric_limits<float>::min();
    size_t checked = 0;
    for (int n = 2; n <= 256; ++n) {
        const float last = (float)(n - 1);
        std::vector<float> vals = {0.0f, -0.0f, den, -den, tiny, -tiny, tiny / 2, last, std::nextafter(last, 0.0f), std::nextafter(last, inf),
                                   last - 1.0f, std::nextafter(last - 1.0f, 0.0f), std::nextafter(last - 1.0f, inf), 3.4e38f, -3.4e38f,
                                   inf, -inf, nan, -nan, 0.5f, 1.0f, std::nextafter(1.0f, 0.0f), 2147483648.0f, -2147483904.0f, 4294967296.0f};
        for (int k = 0; k <= 4 * (n - 1) + 8; ++k) vals.push_back((float)k * 0.25f - 1.0f);
        for (const float s : vals) {
            int i = -1;
            float f = -1.0f;
            gr_lut_index(s, n, i, f);
            CHECK(i >= 0 && i <= n - 2 && f >= 0.0f && f <= 1.0f, "n %d s %.9g: i %d f %.9g", n, (double)s, i, (double)f);
            // where s is inside the lattice, (i, f) is s again
            if (s >= 0.0f && s <= last) CHECK((float)i + f == s, "n %d s %.9g: i %d + f %.9g", n, (double)s, i, (double)f);
            ++checked;
        }
        int i;
        float f;
        gr_lut_index(last, n, i, f);
        CHECK(i == n - 2 && f == 1.0f, "n %d: the last lattice point gives i %d f %g", n, i, (double)f);
        gr_lut_index(inf, n, i, f);
        CHECK(i == n - 2 && f == 1.0f, "n %d: +inf gives i %d f %g", n, i, (double)f);
        gr_lut_index(nan, n, i, f);
        CHECK(i == 0 && f == 0.0f && !std::signbit(f), "n %d: NaN gives i %d f %g", n, i, (double)f);
        gr_lut_index(-0.0f, n, i, f);
        CHECK(i == 0 && f == 0.0f && !std::signbit(f), "n %d: -0 gives i %d f %g", n, i, (double)f);
    }
    std::printf("lut index: %zu values checked\n", checked);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: lut_selftest_asan <a directory for temporary files>\n");
        return 2;
    }
    well_formed();
    malformed();
    truncations();
    files(argv[1]);
    white_balance();
    lut_index();
    if (g_failures) {
        std::printf("lut selftest: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("lut selftest ok\n");
    return 0;
}
