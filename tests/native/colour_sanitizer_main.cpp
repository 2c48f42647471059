// The .cube reader and the host colour stage (path-tracing_amd/csrc/pt_colour_capi.cpp) under AddressSanitizer + UBSan, as a
// program of its own (tests/test_colour_host.py builds and runs it): malformed files, a maximal file, and the stage on values
// that push every LUT index to either end.  It links pt_colour_capi.cpp alone; the two helpers that file takes from the C API's
// main translation unit are defined here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pt_capi_internal.hpp"

static std::string g_error;
int ptc::fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_error.c_str()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static std::string write(const std::string &dir, const std::string &name, const std::string &text) {
    const std::string path = dir + name;
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(3);
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    return path;
}

static int load(const std::string &path) {
    pt_lut *lut = reinterpret_cast<pt_lut *>(0x10);
    const int rc = pt_lut_load_cube(path.c_str(), &lut);
    if (rc == PT_OK) pt_lut_destroy(lut);
    else EXPECT(lut == reinterpret_cast<pt_lut *>(0x10));
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::string row = "0.25 0.5 0.75\n";
    auto rows = [&](int n) { std::string s; for (int i = 0; i < n; ++i) s += row; return s; };
    // malformed files
    EXPECT(load(dir + "absent.cube") == PT_ERR_IO);
    EXPECT(load(write(dir, "empty.cube", "")) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "nul.cube", std::string("LUT_3D_SIZE 2\n\0\0\0\n", 18) + rows(8))) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "short.cube", "LUT_3D_SIZE 3\n" + rows(26))) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "long.cube", "LUT_3D_SIZE 2\n" + rows(9))) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "huge_n.cube", "LUT_3D_SIZE 99999999999999999999\n")) != PT_OK);
    EXPECT(load(write(dir, "neg_n.cube", "LUT_3D_SIZE -3\n")) == PT_ERR_UNSUPPORTED);
    EXPECT(load(write(dir, "one_d.cube", "LUT_1D_SIZE 4\n" + rows(4))) == PT_ERR_UNSUPPORTED);
    EXPECT(load(write(dir, "domain.cube", "LUT_3D_SIZE 2\nDOMAIN_MAX 1 1\n" + rows(8))) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "token.cube", "LUT_3D_SIZE 2\n" + rows(7) + "0.5 0.5 x\n")) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "long_line.cube", "LUT_3D_SIZE 2\n" + std::string(100000, '7') + "\n")) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(load(write(dir, "no_end.cube", "LUT_3D_SIZE 2\r\n" + rows(7) + "1 1 1")) == PT_OK);
    // a maximal file, and the stage on it
    const int n = PT_LUT_MAX_SIZE;
    std::string text = "TITLE \"max\"\nLUT_3D_SIZE 65\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n";
    text.reserve(text.size() + 12 * static_cast<size_t>(n) * n * n);
    for (int b = 0; b < n; ++b)
        for (int g = 0; g < n; ++g)
            for (int r = 0; r < n; ++r) {
                char buf[64];
                std::snprintf(buf, sizeof buf, "%.6g %.6g %.6g\n", r / 64.0, g / 64.0, b / 64.0);
                text += buf;
            }
    pt_lut *lut = nullptr;
    EXPECT(pt_lut_load_cube(write(dir, "max.cube", text).c_str(), &lut) == PT_OK && lut);
    int32_t size = 0;
    EXPECT(pt_lut_size(lut, &size) == PT_OK && size == n);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float edge[] = {0.0f, -0.0f, 1.0f, 0.99999994f, 1.0000001f, 0.5f, -1.0f, 2.0f, inf, -inf, nan, 3.0e38f, -3.0e38f, 1e-45f, 63.0f / 64.0f, 1.0f / 64.0f};
    const int k = sizeof edge / sizeof edge[0];
    std::vector<float> mean, out;
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b)
            for (int c = 0; c < k; ++c) { mean.push_back(edge[a]); mean.push_back(edge[b]); mean.push_back(edge[c]); }
    const int32_t px = static_cast<int32_t>(mean.size() / 3);
    std::vector<int32_t> count(px, 1);
    count[5] = 0;
    out.resize(mean.size());
    pt_colour_params prm{};
    prm.lut = lut;
    prm.wb[0] = 1.5f; prm.wb[1] = 1.0f; prm.wb[2] = 0.5f;
    prm.saturation = 0.5f;
    for (int curve = 0; curve < 4; ++curve) {
        EXPECT(pt_colour_host(px, 1, mean.data(), count.data(), 1.0f, curve, &prm, out.data()) == PT_OK);
        EXPECT(pt_colour_host(px, 1, mean.data(), count.data(), 3.0e38f, curve, &prm, out.data()) == PT_OK);
    }
    // the identity LUT at its vertices, in place
    prm = pt_colour_params{};
    prm.lut = lut;
    std::vector<float> v = {0.0f, 1.0f, 0.5f, 0.25f, 0.75f, 1.0f};
    std::vector<int32_t> two(2, 1);
    EXPECT(pt_colour_host(2, 1, v.data(), two.data(), 1.0f, PT_CURVE_REFERENCE, &prm, v.data()) == PT_OK);
    EXPECT(v[0] == 0.0f && v[1] == 1.0f && v[2] == 0.5f && v[3] == 0.25f && v[4] == 0.75f && v[5] == 1.0f);
    // refusals
    float m9[9];
    prm.wb[1] = -1.0f;
    EXPECT(pt_colour_matrix(&prm, m9) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_colour_matrix(nullptr, m9) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_colour_host(2, 1, v.data(), two.data(), 1.0f, 0, nullptr, v.data()) == PT_ERR_INVALID_ARGUMENT);
    pt_lut *made = nullptr;
    std::vector<float> small(3 * 8, 0.5f);
    EXPECT(pt_lut_create(2, small.data(), &made) == PT_OK && made);
    pt_lut_destroy(made);
    made = nullptr;
    EXPECT(pt_lut_create(1, small.data(), &made) == PT_ERR_UNSUPPORTED && !made);
    small[7] = nan;
    EXPECT(pt_lut_create(2, small.data(), &made) == PT_ERR_INVALID_ARGUMENT && !made);
    pt_lut_destroy(lut);
    pt_lut_destroy(nullptr);
    if (failures) return 1;
    std::printf("colour host ok\n");
    return 0;
}
