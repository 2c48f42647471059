// Host side of colour grading (include/pt_hip.h: pt_lut_*, pt_colour_matrix, pt_colour_host): the LUT's owner and the .cube reader,
// the parameter check every entry point with the stage shares (it composes M), and the host chain's colour step.  The per-pixel
// arithmetic is pt_colour.hpp's, the one copy the kernel uses too.  Nothing here touches a device.
#include "pt_capi_internal.hpp"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>

using ptc::fail;
using ptc::guarded;

static_assert(PT_LUT_MAX_SIZE == pt::kLutMaxSize, "the ABI header states the largest LUT");
static_assert(sizeof(pt::LutVertex) == 16, "a LUT vertex is one 16-byte load");

namespace {

std::atomic<uint64_t> next_generation{1};

int check_lut_size(long n, const std::string &where) {
    if (n < pt::kLutMinSize || n > pt::kLutMaxSize)
        return fail(PT_ERR_UNSUPPORTED, where + "a 3D LUT has 2 .. " + std::to_string(pt::kLutMaxSize) + " vertices per axis, not " + std::to_string(n));
    return PT_OK;
}

std::unique_ptr<pt_lut> new_lut(int32_t n) {
    std::unique_ptr<pt_lut> lut(new pt_lut);
    lut->n = n;
    lut->generation = next_generation.fetch_add(1);
    lut->vertices.reserve(static_cast<size_t>(n) * n * n);
    return lut;
}

int lut_create_impl(int32_t n, const float *rgb, pt_lut **out) {
    if (!rgb || !out) return fail(PT_ERR_INVALID_ARGUMENT, "lut: null pointer");
    const int rc = check_lut_size(n, "lut: ");
    if (rc != PT_OK) return rc;
    const size_t count = static_cast<size_t>(n) * n * n;
    for (size_t i = 0; i < 3 * count; ++i)
        if (!std::isfinite(rgb[i])) return fail(PT_ERR_INVALID_ARGUMENT, "lut: vertex " + std::to_string(i / 3) + " is not finite");
    std::unique_ptr<pt_lut> lut = new_lut(n);
    for (size_t i = 0; i < count; ++i) lut->vertices.push_back({rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f});
    *out = lut.release();
    return PT_OK;
}

// `count` numbers and nothing else from p; false: a token does not parse.
bool parse_numbers(const char *p, int count, float *v) {
    for (int k = 0; k < count; ++k) {
        char *end = nullptr;
        v[k] = std::strtof(p, &end);
        if (end == p) return false;
        p = end;
    }
    while (*p == ' ' || *p == '\t') ++p;
    return *p == '\0';
}

// "KEY" at the start of `line`, followed by blank space or the end: the rest, else NULL.
const char *after_keyword(const std::string &line, const char *key) {
    const size_t k = std::strlen(key);
    if (line.compare(0, k, key) != 0) return nullptr;
    if (line.size() > k && line[k] != ' ' && line[k] != '\t') return nullptr;
    return line.c_str() + k;
}

int lut_load_cube_impl(const char *path, pt_lut **out) {
    if (!path || !out) return fail(PT_ERR_INVALID_ARGUMENT, "cube: null pointer");
    std::ifstream in(path, std::ios::binary);
    if (!in) return fail(PT_ERR_IO, std::string("cube: cannot open ") + path);
    std::unique_ptr<pt_lut> lut;
    size_t want = 0;
    std::string line;
    long number = 0;
    while (std::getline(in, line)) {
        ++number;
        const std::string where = std::string("cube: ") + path + " line " + std::to_string(number) + ": ";
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        const size_t first = line.find_first_not_of(" \t");
        if (first == std::string::npos) continue;
        line.erase(0, first);
        if (line[0] == '#' || after_keyword(line, "TITLE")) continue;
        if (after_keyword(line, "LUT_1D_SIZE")) return fail(PT_ERR_UNSUPPORTED, where + "a 1D LUT (LUT_1D_SIZE) is not supported");
        float v[3];
        if (const char *rest = after_keyword(line, "LUT_3D_SIZE")) {
            if (lut) return fail(PT_ERR_INVALID_ARGUMENT, where + "a second LUT_3D_SIZE");
            if (!parse_numbers(rest, 1, v) || !(v[0] == std::floor(v[0])) || !(std::fabs(v[0]) < 1e6f))
                return fail(PT_ERR_INVALID_ARGUMENT, where + "LUT_3D_SIZE takes one whole number");
            const int rc = check_lut_size(static_cast<long>(v[0]), where);
            if (rc != PT_OK) return rc;
            lut = new_lut(static_cast<int32_t>(v[0]));
            want = static_cast<size_t>(lut->n) * lut->n * lut->n;
            continue;
        }
        const char *dmin = after_keyword(line, "DOMAIN_MIN"), *dmax = after_keyword(line, "DOMAIN_MAX");
        if (dmin || dmax) {
            if (!parse_numbers(dmin ? dmin : dmax, 3, v)) return fail(PT_ERR_INVALID_ARGUMENT, where + "a domain takes three numbers");
            const float d = dmin ? 0.0f : 1.0f;
            if (!(v[0] == d && v[1] == d && v[2] == d)) return fail(PT_ERR_UNSUPPORTED, where + "only the domain 0 0 0 .. 1 1 1 is supported");
            continue;
        }
        if (!parse_numbers(line.c_str(), 3, v)) return fail(PT_ERR_INVALID_ARGUMENT, where + "not a keyword of a 3D .cube file and not three numbers");
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return fail(PT_ERR_INVALID_ARGUMENT, where + "a value is not finite");
        if (!lut) return fail(PT_ERR_INVALID_ARGUMENT, where + "data before LUT_3D_SIZE");
        if (lut->vertices.size() == want) return fail(PT_ERR_INVALID_ARGUMENT, where + "more than " + std::to_string(want) + " data lines");
        lut->vertices.push_back({v[0], v[1], v[2], 0.0f});
    }
    const std::string where = std::string("cube: ") + path + " line " + std::to_string(number) + " (the last): ";
    if (!lut) return fail(PT_ERR_INVALID_ARGUMENT, where + "no LUT_3D_SIZE line");
    if (lut->vertices.size() != want)
        return fail(PT_ERR_INVALID_ARGUMENT, where + std::to_string(lut->vertices.size()) + " data lines, " + std::to_string(want) + " expected");
    *out = lut.release();
    return PT_OK;
}

int colour_host_impl(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, int32_t curve,
                     const pt_colour_params *c, float *out_rgb) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "colour: null buffer or empty image");
    if (curve < 0 || curve >= pt::kCurveCount) return fail(PT_ERR_INVALID_ARGUMENT, "colour: unknown curve");
    if (!std::isfinite(exposure) || !(exposure > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "colour: exposure must be finite and > 0");
    ptc::ColourSetup setup;
    const int rc = ptc::colour_params_check(c, setup);
    if (rc != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    for (size_t p = 0; p < n; ++p) {
        float r = mean_rgb[3 * p], g = mean_rgb[3 * p + 1], b = mean_rgb[3 * p + 2];
        if (count[p]) pt::colour_pixel(setup.step, curve, exposure, r, g, b);
        out_rgb[3 * p] = r; out_rgb[3 * p + 1] = g; out_rgb[3 * p + 2] = b;
    }
    return PT_OK;
}

}  // namespace

int ptc::colour_params_check(const pt_colour_params *c, ColourSetup &out) {
    if (!c) return fail(PT_ERR_INVALID_ARGUMENT, "colour: null params");
    auto bad = [](float v) { return !std::isfinite(v) || v < 0.0f; };
    if (bad(c->wb[0]) || bad(c->wb[1]) || bad(c->wb[2]))
        return fail(PT_ERR_INVALID_ARGUMENT, "colour: the white balance gains must be finite and not negative (0 0 0 = 1 1 1)");
    if (bad(c->saturation)) return fail(PT_ERR_INVALID_ARGUMENT, "colour: saturation must be finite and not negative (0 without saturation_set = 1)");
    bool user = false;
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(c->matrix[i])) return fail(PT_ERR_INVALID_ARGUMENT, "colour: the matrix must be finite (all zero = identity)");
        user = user || c->matrix[i] != 0.0f;
    }
    if (c->lut && (c->lut->n < pt::kLutMinSize || c->lut->n > pt::kLutMaxSize ||
                   c->lut->vertices.size() != static_cast<size_t>(c->lut->n) * c->lut->n * c->lut->n))
        return fail(PT_ERR_INVALID_ARGUMENT, "colour: lut is not a LUT made by pt_lut_create or pt_lut_load_cube");
    // M = U S W in double, each entry rounded once
    const bool unit_wb = c->wb[0] == 0.0f && c->wb[1] == 0.0f && c->wb[2] == 0.0f;
    const double s = (c->saturation_set != 0 || c->saturation != 0.0f) ? static_cast<double>(c->saturation) : 1.0;
    const double lum[3] = {0.2126, 0.7152, 0.0722};
    double SW[9], U[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double w = unit_wb ? 1.0 : static_cast<double>(c->wb[j]);
            SW[3 * i + j] = ((i == j ? s : 0.0) + (1.0 - s) * lum[j]) * w;
            U[3 * i + j] = user ? static_cast<double>(c->matrix[3 * i + j]) : (i == j ? 1.0 : 0.0);
        }
    ColourSetup setup;
    bool identity = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double m = (U[3 * i] * SW[j] + U[3 * i + 1] * SW[3 + j]) + U[3 * i + 2] * SW[6 + j];
            const float f = static_cast<float>(m);
            if (!std::isfinite(f)) return fail(PT_ERR_INVALID_ARGUMENT, "colour: the composed matrix is not finite");
            setup.step.m[3 * i + j] = f;
            identity = identity && pt::grade_bits(f) == pt::grade_bits(i == j ? 1.0f : 0.0f);
        }
    setup.step.apply_matrix = identity ? 0 : 1;
    setup.lut = c->lut;
    setup.step.lut_n = c->lut ? c->lut->n : 0;
    setup.step.lut = c->lut ? c->lut->vertices.data() : nullptr;
    setup.on = !identity || c->lut != nullptr;
    out = setup;
    return PT_OK;
}

extern "C" {

int pt_lut_create(int32_t n, const float *rgb, pt_lut **out) {
    return guarded([&] { return lut_create_impl(n, rgb, out); });
}

int pt_lut_load_cube(const char *path, pt_lut **out) {
    return guarded([&] { return lut_load_cube_impl(path, out); });
}

int pt_lut_size(const pt_lut *lut, int32_t *n) {
    return guarded([&] {
        if (!lut || !n) return fail(PT_ERR_INVALID_ARGUMENT, "lut: null pointer");
        *n = lut->n;
        return static_cast<int>(PT_OK);
    });
}

void pt_lut_destroy(pt_lut *lut) { delete lut; }

int pt_colour_matrix(const pt_colour_params *c, float out[9]) {
    return guarded([&] {
        if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "colour: null output");
        ptc::ColourSetup setup;
        const int rc = ptc::colour_params_check(c, setup);
        if (rc != PT_OK) return rc;
        std::memcpy(out, setup.step.m, sizeof setup.step.m);
        return static_cast<int>(PT_OK);
    });
}

int pt_colour_host(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, int32_t curve,
                   const pt_colour_params *c, float *out_rgb) {
    return guarded([&] { return colour_host_impl(width, height, mean_rgb, count, exposure, curve, c, out_rgb); });
}

}  // extern "C"
