// rtm_lut.cpp — the host-only helpers of the grade (include/rtm.h): rtm_grade_white_balance, the Bradford adaptation from a
// colour temperature's white to D65 in linear Rec.709 primaries, and rtm_lut_parse_cube / rtm_lut_load_cube, an own reader
// of the Adobe / Resolve .cube text format for 3D LUTs.  No device call, no HIP header: lut_selftest.cpp builds this unit
// alone (with rtm_scene.cpp for the last-error text) under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rtm_internal.h"

namespace rtm {

namespace {
struct M3 {
    double v[3][3];
};
struct V3 {
    double v[3];
};

M3 mul(const M3& a, const M3& b) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.v[i][j] = (a.v[i][0] * b.v[0][j] + a.v[i][1] * b.v[1][j]) + a.v[i][2] * b.v[2][j];
    return r;
}
V3 mul(const M3& a, const V3& x) {
    V3 r;
    for (int i = 0; i < 3; ++i) r.v[i] = (a.v[i][0] * x.v[0] + a.v[i][1] * x.v[1]) + a.v[i][2] * x.v[2];
    return r;
}
// the inverse by cofactors (the matrices here are far from singular)
M3 inverse(const M3& m) {
    const double(*a)[3] = m.v;
    M3 c;
    c.v[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    c.v[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
    c.v[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
    c.v[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    c.v[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
    c.v[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
    c.v[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    c.v[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    c.v[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = (a[0][0] * c.v[0][0] + a[0][1] * c.v[1][0]) + a[0][2] * c.v[2][0];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.v[i][j] /= det;
    return c;
}
// XYZ of the chromaticity (x, y) at Y = 1
V3 white_xyz(double x, double y) { return V3{{x / y, 1.0, ((1.0 - x) - y) / y}}; }

constexpr double kD65x = 0.3127, kD65y = 0.3290;
// Lam's Bradford cone response matrix
const M3 kBradford = {{{0.8951, 0.2664, -0.1614}, {-0.7502, 1.7135, 0.0367}, {0.0389, -0.0685, 1.0296}}};

// linear Rec.709 / sRGB RGB -> XYZ, derived from the primaries and the D65 white: the columns are the primaries' XYZ scaled
// so that RGB (1, 1, 1) is the white
M3 rec709_to_xyz() {
    static const double prim[3][2] = {{0.64, 0.33}, {0.30, 0.60}, {0.15, 0.06}};
    M3 p;
    for (int j = 0; j < 3; ++j) {
        const V3 c = white_xyz(prim[j][0], prim[j][1]);
        for (int i = 0; i < 3; ++i) p.v[i][j] = c.v[i];
    }
    const V3 s = mul(inverse(p), white_xyz(kD65x, kD65y));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) p.v[i][j] *= s.v[j];
    return p;
}
}  // namespace

// Kang et al. (2002): the Planckian locus's chromaticity as cubics in 1 / T and x (rtm.h gives the coefficients)
int grade_white_balance(float kelvin, float tint, float* matrix_out) {
    if (!matrix_out) return invalid("null matrix_out");
    if (!(kelvin >= 1667.0f && kelvin <= 25000.0f)) return invalid("kelvin is NaN or outside [1667, 25000]");
    if (!(tint >= -0.05f && tint <= 0.05f)) return invalid("tint is NaN or outside [-0.05, 0.05]");
    const double T = (double)kelvin, T2 = T * T, T3 = T2 * T;
    double x, y;
    if (T <= 4000.0)
        x = -0.2661239e9 / T3 - 0.2343589e6 / T2 + 0.8776956e3 / T + 0.179910;
    else
        x = -3.0258469e9 / T3 + 2.1070379e6 / T2 + 0.2226347e3 / T + 0.240390;
    const double x2 = x * x, x3 = x2 * x;
    if (T <= 2222.0)
        y = -1.1063814 * x3 - 1.34811020 * x2 + 2.18555832 * x - 0.20219683;
    else if (T <= 4000.0)
        y = -0.9549476 * x3 - 1.37418593 * x2 + 2.09137015 * x - 0.16748867;
    else
        y = 3.0817580 * x3 - 5.87338670 * x2 + 3.75112997 * x - 0.37001483;
    // tint: along v of CIE 1960 (u, v), and back
    const double d = -2.0 * x + 12.0 * y + 3.0;
    const double u = 4.0 * x / d, v = 6.0 * y / d + (double)tint;
    const double e = 2.0 * u - 8.0 * v + 4.0;
    x = 3.0 * u / e;
    y = 2.0 * v / e;
    if (!(std::isfinite(x) && std::isfinite(y) && y > 0.0)) return invalid("the tinted white has no chromaticity");
    // Bradford: scale the cone responses of the source white to those of D65
    const V3 cs = mul(kBradford, white_xyz(x, y)), cd = mul(kBradford, white_xyz(kD65x, kD65y));
    M3 scale = {{{cd.v[0] / cs.v[0], 0.0, 0.0}, {0.0, cd.v[1] / cs.v[1], 0.0}, {0.0, 0.0, cd.v[2] / cs.v[2]}}};
    const M3 adapt = mul(inverse(kBradford), mul(scale, kBradford));
    const M3 to_xyz = rec709_to_xyz();
    const M3 m = mul(inverse(to_xyz), mul(adapt, to_xyz));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            if (!std::isfinite(m.v[i][j])) return invalid("the white balance matrix is not finite");
            matrix_out[3 * i + j] = (float)m.v[i][j];
        }
    return RTM_OK;
}

namespace {
int parse_fail(int line, const std::string& what) { return fail(RTM_ERR_PARSE, "line " + std::to_string(line) + ": " + what); }
bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// the whitespace-separated tokens of a line
std::vector<std::string> tokens(const std::string& line) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && blank(line[i])) ++i;
        const size_t b = i;
        while (i < line.size() && !blank(line[i])) ++i;
        if (i > b) out.push_back(line.substr(b, i - b));
    }
    return out;
}
// a decimal number, all of the token, finite as a float
bool number(const std::string& t, float& out) {
    if (t.empty() || t.size() > 64) return false;
    for (const char c : t)
        if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return false;
    char* end = nullptr;
    const double v = std::strtod(t.c_str(), &end);
    if (end != t.c_str() + t.size() || !std::isfinite(v)) return false;
    out = (float)v;
    return std::isfinite(out);
}
bool numbers(const std::vector<std::string>& t, size_t first, size_t count, float* out) {
    if (t.size() != first + count) return false;
    for (size_t k = 0; k < count; ++k)
        if (!number(t[first + k], out[k])) return false;
    return true;
}
}  // namespace

int lut_parse_cube(const char* text, size_t len, int32_t* size, float* domain_min, float* domain_max, float* table,
                   size_t capacity) {
    if ((!text && len) || !size || !domain_min || !domain_max) return invalid("null text, size, domain_min or domain_max");
    if (!table && capacity) return invalid("null table with a capacity");
    int n = 0, line_no = 0, domain_line = 0;
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {1.0f, 1.0f, 1.0f};
    size_t rows = 0, want = 0;
    bool store = false, checked = false;
    // the header is complete (the first row, or the end of the text): what it must have said, and whether the table fits
    const auto header_done = [&]() -> int {
        checked = true;
        if (n == 0) return parse_fail(line_no, "no LUT_3D_SIZE before the table");
        for (int c = 0; c < 3; ++c)
            if (!(hi[c] > lo[c])) return parse_fail(domain_line ? domain_line : line_no, "the domain's max <= min");
        *size = n;
        std::memcpy(domain_min, lo, sizeof lo);
        std::memcpy(domain_max, hi, sizeof hi);
        want = (size_t)n * n * n;
        store = table != nullptr && capacity >= 3 * want;
        return RTM_OK;
    };
    size_t pos = 0;
    while (pos < len) {
        size_t eol = pos;
        while (eol < len && text[eol] != '\n') ++eol;
        const std::string line(text + pos, eol - pos);
        pos = eol + 1;
        ++line_no;
        const std::vector<std::string> t = tokens(line);
        if (t.empty() || t[0][0] == '#') continue;
        const char c0 = t[0][0];
        if ((c0 >= 'A' && c0 <= 'Z') || (c0 >= 'a' && c0 <= 'z') || c0 == '_') {  // a keyword
            if (t[0] == "LUT_1D_SIZE" || t[0] == "LUT_1D_INPUT_RANGE")
                return fail(RTM_ERR_UNSUPPORTED, "line " + std::to_string(line_no) + ": a 1D LUT (" + t[0] + ") is not supported");
            if (rows > 0) return parse_fail(line_no, "a keyword inside the table: " + t[0]);
            if (t[0] == "TITLE") continue;
            if (t[0] == "LUT_3D_SIZE") {
                float v = 0.0f;
                if (n != 0) return parse_fail(line_no, "LUT_3D_SIZE given twice");
                if (!numbers(t, 1, 1, &v) || v != std::floor(v) || v < 2.0f || v > 256.0f)
                    return parse_fail(line_no, "LUT_3D_SIZE takes one whole number in 2..256");
                n = (int)v;
            } else if (t[0] == "DOMAIN_MIN" || t[0] == "DOMAIN_MAX") {
                if (!numbers(t, 1, 3, t[0] == "DOMAIN_MIN" ? lo : hi)) return parse_fail(line_no, t[0] + " takes three finite numbers");
                domain_line = line_no;
            } else if (t[0] == "LUT_3D_INPUT_RANGE") {
                float r[2];
                if (!numbers(t, 1, 2, r)) return parse_fail(line_no, "LUT_3D_INPUT_RANGE takes two finite numbers");
                for (int c = 0; c < 3; ++c) lo[c] = r[0], hi[c] = r[1];
                domain_line = line_no;
            } else {
                return parse_fail(line_no, "unknown keyword " + t[0]);
            }
            continue;
        }
        // a row of the table
        if (n == 0) return parse_fail(line_no, "data before LUT_3D_SIZE");
        if (!checked)
            if (const int rc = header_done(); rc != RTM_OK) return rc;
        float v[3];
        if (!numbers(t, 0, 3, v)) return parse_fail(line_no, "a row takes three finite numbers");
        if (rows == want) return parse_fail(line_no, "too many rows: more than size^3");
        if (store) std::memcpy(table + 3 * rows, v, sizeof v);
        ++rows;
    }
    if (!checked)
        if (const int rc = header_done(); rc != RTM_OK) return rc;
    if (rows != want) return parse_fail(line_no, "too few rows: " + std::to_string(rows) + " of " + std::to_string(want));
    if (table && !store) return fail(RTM_ERR_CAPACITY, "table buffer too small");
    return RTM_OK;
}

int lut_load_cube(const char* path, int32_t* size, float* domain_min, float* domain_max, float* table, size_t capacity) {
    if (!path) return invalid("null path");
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail(RTM_ERR_IO, std::string("cannot open ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    return lut_parse_cube(text.data(), text.size(), size, domain_min, domain_max, table, capacity);
}

}  // namespace rtm
