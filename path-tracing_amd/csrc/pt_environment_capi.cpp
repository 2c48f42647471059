// Host side of environment lighting (include/pt_hip.h: pt_environment_*): the readers of Radiance .hdr and PFM pictures, the
// conversion of an equirectangular picture into the octahedral map and the handle's setters.  The arithmetic is pt_environment.hpp's,
// the one copy the kernels use too.  A setter prepares everything -- picture, map, device copy -- before it touches the handle, so a
// failed call leaves the handle as it was.
#include "pt_capi_internal.hpp"

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>

using ptc::fail;
using ptc::guarded;

namespace {

struct Picture {
    int w = 0, h = 0;
    std::vector<float> rgb;   // rows top-down
};

int read_file(const char *path, std::vector<uint8_t> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(PT_ERR_IO, std::string("environment: cannot open ") + path);
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    return bad ? fail(PT_ERR_IO, std::string("environment: cannot read ") + path) : static_cast<int>(PT_OK);
}

int parse_fail(const std::string &why) { return fail(PT_ERR_PARSE, "environment: " + why); }

bool size_ok(long long w, long long h) { return w >= 1 && h >= 1 && w <= pt::kEnvMaxSourceW && h <= pt::kEnvMaxSourceH; }

// one line of a text header from `at` on, without its '\n'; false at the end of the data
bool next_line(const std::vector<uint8_t> &d, size_t &at, std::string &line) {
    const size_t begin = at;
    while (at < d.size() && d[at] != '\n') ++at;
    if (at >= d.size()) return false;
    line.assign(reinterpret_cast<const char *>(d.data()) + begin, at - begin);
    ++at;
    return true;
}

// Radiance: "#?RADIANCE" or "#?RGBE", header lines up to an empty one with FORMAT=32-bit_rle_rgbe among them, "-Y h +X w", then per
// scanline either w flat pixels or the new-style run-length coding (2, 2, w >> 8, w & 255, then each of the four channels as runs).
int read_hdr(const std::vector<uint8_t> &d, Picture &out) {
    size_t at = 0;
    std::string line;
    if (!next_line(d, at, line) || (line != "#?RADIANCE" && line != "#?RGBE")) return parse_fail("not a Radiance picture");
    bool format = false;
    for (;;) {
        if (!next_line(d, at, line)) return parse_fail("Radiance header: truncated");
        if (line.empty()) break;
        if (line == "FORMAT=32-bit_rle_rgbe") format = true;
        else if (line.compare(0, 7, "FORMAT=") == 0) return parse_fail("Radiance header: " + line + " is not 32-bit_rle_rgbe");
    }
    if (!format) return parse_fail("Radiance header: no FORMAT=32-bit_rle_rgbe line");
    if (!next_line(d, at, line)) return parse_fail("Radiance header: truncated");
    long long h = 0, w = 0;
    char tail = 0;
    if (std::sscanf(line.c_str(), "-Y %lld +X %lld%c", &h, &w, &tail) != 2) return parse_fail("Radiance picture: only the orientation -Y h +X w is read, not \"" + line + "\"");
    if (!size_ok(w, h)) return parse_fail("Radiance picture: size " + std::to_string(w) + " x " + std::to_string(h) + " is empty or above 16384 x 8192");
    std::vector<uint8_t> px(static_cast<size_t>(w) * 4);
    out.w = static_cast<int>(w);
    out.h = static_cast<int>(h);
    out.rgb.resize(static_cast<size_t>(w) * h * 3);
    for (long long y = 0; y < h; ++y) {
        const bool rle = w >= 8 && w < 32768 && at + 4 <= d.size() && d[at] == 2 && d[at + 1] == 2 && d[at + 2] < 128 &&
                         ((static_cast<long long>(d[at + 2]) << 8) | d[at + 3]) == w;
        if (rle) {
            at += 4;
            for (int c = 0; c < 4; ++c) {
                long long x = 0;
                while (x < w) {
                    if (at >= d.size()) return parse_fail("Radiance picture: truncated inside a run-length scanline");
                    const int code = d[at++];
                    const int len = code > 128 ? code - 128 : code;
                    if (len == 0) return parse_fail("Radiance picture: a run of length 0");
                    if (x + len > w) return parse_fail("Radiance picture: a run overruns its scanline");
                    if (code > 128) {
                        if (at >= d.size()) return parse_fail("Radiance picture: truncated inside a run-length scanline");
                        const uint8_t v = d[at++];
                        for (int i = 0; i < len; ++i) px[4 * static_cast<size_t>(x + i) + c] = v;
                    } else {
                        if (at + static_cast<size_t>(len) > d.size()) return parse_fail("Radiance picture: truncated inside a run-length scanline");
                        for (int i = 0; i < len; ++i) px[4 * static_cast<size_t>(x + i) + c] = d[at++];
                    }
                    x += len;
                }
            }
        } else {
            if (at + px.size() > d.size()) return parse_fail("Radiance picture: truncated");
            std::memcpy(px.data(), d.data() + at, px.size());
            at += px.size();
        }
        // the inverse pt_hip.h defines for PT_LINEAR_RGBE: (byte + 0.5) * 2^(E - 136); the pixel 0, 0, 0, 0 is black
        float *row = &out.rgb[static_cast<size_t>(y) * w * 3];
        for (long long x = 0; x < w; ++x) {
            const uint8_t *p = &px[4 * static_cast<size_t>(x)];
            const bool zero = p[0] == 0 && p[1] == 0 && p[2] == 0 && p[3] == 0;
            for (int c = 0; c < 3; ++c) row[3 * x + c] = zero ? 0.0f : static_cast<float>(std::ldexp(p[c] + 0.5, static_cast<int>(p[3]) - 136));
        }
    }
    if (at != d.size()) return parse_fail("Radiance picture: bytes after the last scanline");
    return PT_OK;
}

// PFM: "PF", width, height and scale as whitespace-separated tokens, ONE whitespace byte, then rows bottom-up of r, g, b floats,
// little-endian if the scale is negative, big-endian if it is positive (its magnitude is not applied).
int read_pfm(const std::vector<uint8_t> &d, Picture &out) {
    if (d.size() >= 2 && d[0] == 'P' && d[1] == 'f') return parse_fail("PFM: a one-channel picture (Pf); three channels (PF) are read");
    size_t at = 2;
    std::string tok[3];
    for (auto &t : tok) {
        while (at < d.size() && std::isspace(d[at])) ++at;
        while (at < d.size() && !std::isspace(d[at])) t.push_back(static_cast<char>(d[at++]));
        if (t.empty() || t.size() > 32) return parse_fail("PFM header: truncated");
    }
    if (at >= d.size()) return parse_fail("PFM header: truncated");
    ++at;
    char *end = nullptr;
    const long long w = std::strtoll(tok[0].c_str(), &end, 10);
    if (*end) return parse_fail("PFM header: width \"" + tok[0] + "\"");
    const long long h = std::strtoll(tok[1].c_str(), &end, 10);
    if (*end) return parse_fail("PFM header: height \"" + tok[1] + "\"");
    const double scale = std::strtod(tok[2].c_str(), &end);
    if (*end || !std::isfinite(scale) || scale == 0.0) return parse_fail("PFM header: scale \"" + tok[2] + "\"");
    if (!size_ok(w, h)) return parse_fail("PFM: size " + std::to_string(w) + " x " + std::to_string(h) + " is empty or above 16384 x 8192");
    const size_t n = static_cast<size_t>(w) * h * 3;
    if (d.size() - at < 4 * n) return parse_fail("PFM: truncated");
    if (d.size() - at > 4 * n) return parse_fail("PFM: bytes after the last row");
    out.w = static_cast<int>(w);
    out.h = static_cast<int>(h);
    out.rgb.resize(n);
    const bool little = scale < 0.0;
    for (long long y = 0; y < h; ++y) {
        const uint8_t *src = d.data() + at + 12 * static_cast<size_t>(h - 1 - y) * w;
        float *row = &out.rgb[static_cast<size_t>(y) * w * 3];
        for (long long i = 0; i < 3 * w; ++i) {
            const uint8_t *b = src + 4 * i;
            const uint32_t u = little ? (b[0] | (b[1] << 8) | (b[2] << 16) | (static_cast<uint32_t>(b[3]) << 24))
                                      : (b[3] | (b[2] << 8) | (b[1] << 16) | (static_cast<uint32_t>(b[0]) << 24));
            row[i] = pt::grade_from_bits(u);
        }
    }
    return PT_OK;
}

// by content, not by name
int read_picture(const char *path, Picture &out) {
    std::vector<uint8_t> d;
    const int rc = read_file(path, d);
    if (rc != PT_OK) return rc;
    if (d.size() >= 2 && d[0] == 'P' && (d[1] == 'F' || d[1] == 'f')) return read_pfm(d, out);
    if (d.size() >= 2 && d[0] == '#' && d[1] == '?') return read_hdr(d, out);
    return parse_fail(std::string(path) + " is neither a Radiance picture (#?RADIANCE, #?RGBE) nor a PFM (PF)");
}

int check_samples(const float *rgb, size_t n, const char *what) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(rgb[i]) || rgb[i] < 0.0f) return fail(PT_ERR_PARSE, std::string("environment: ") + what + " holds a non-finite or negative sample");
    return PT_OK;
}

int check_map_size(int32_t n) {
    if (n < pt::kEnvMinSize || n > pt::kEnvMaxSize) return fail(PT_ERR_INVALID_ARGUMENT, "environment: the map's size must lie in 8 .. 4096");
    return PT_OK;
}

int check_params(const pt_environment_params *p, int32_t h, float &gain, float &rotate, int &n) {
    gain = p ? p->gain : 1.0f;
    rotate = p ? p->rotate_y_degrees : 0.0f;
    const int32_t size = p ? p->size : 0;
    if (!std::isfinite(gain) || gain < 0.0f) return fail(PT_ERR_INVALID_ARGUMENT, "environment: gain must be finite and >= 0");
    if (!std::isfinite(rotate)) return fail(PT_ERR_INVALID_ARGUMENT, "environment: rotate_y_degrees must be finite");
    if (size != 0) {
        const int rc = check_map_size(size);
        if (rc != PT_OK) return rc;
    }
    n = size != 0 ? size : pt::env_default_size(h);
    return PT_OK;
}

int check_picture(int32_t w, int32_t h, const float *rgb) {
    if (!rgb) return fail(PT_ERR_INVALID_ARGUMENT, "environment: null picture");
    if (!size_ok(w, h)) return fail(PT_ERR_INVALID_ARGUMENT, "environment: the picture's size is empty or above 16384 x 8192");
    return check_samples(rgb, static_cast<size_t>(w) * h * 3, "the picture");
}

// Puts a finished map on the handle: the device copy is allocated and filled first, the handle changes last.
int install(pt_scene *scene, std::shared_ptr<pt_env_map> map) {
    ptc::DeviceBuffer fresh;
    if (scene->device >= 0) {
        PT_HIP_TRY(hipSetDevice(scene->device));
        if (map) {
            const int rc = fresh.upload(pt::env_with_apron(map->n, map->rgb.data()), "environment map", 64);
            if (rc != PT_OK) return rc;
        }
        PT_HIP_TRY(hipDeviceSynchronize());   // (a launch in flight may still read the old map)
    }
    scene->d_env = std::move(fresh);
    scene->env = std::move(map);
    return PT_OK;
}

const char *const kHasSkybox = "environment: the scene handle has a skybox; a handle has a skybox or an environment";

// The three ways to a finished map (nullptr: removal).  Nothing here touches a handle.
int map_from_equirect(int32_t w, int32_t h, const float *rgb, const pt_environment_params *p, std::shared_ptr<pt_env_map> &out) {
    int rc = check_picture(w, h, rgb);
    float gain, rotate;
    int n;
    if (rc != PT_OK || (rc = check_params(p, h, gain, rotate, n)) != PT_OK) return rc;
    auto map = std::make_shared<pt_env_map>();
    map->n = n;
    map->rgb.resize(static_cast<size_t>(n) * n * 3);
    pt::env_from_equirect(w, h, rgb, gain, rotate, n, map->rgb.data());
    if ((rc = check_samples(map->rgb.data(), map->rgb.size(), "the map (picture x gain)")) != PT_OK) return rc;
    out = std::move(map);
    return PT_OK;
}

int map_from_file(const char *path, const pt_environment_params *p, std::shared_ptr<pt_env_map> &out) {
    Picture pic;
    const int rc = read_picture(path, pic);
    if (rc != PT_OK) return rc;
    return map_from_equirect(pic.w, pic.h, pic.rgb.data(), p, out);
}

int map_from_map(int32_t n, const float *rgb, std::shared_ptr<pt_env_map> &out) {
    if (!rgb) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_map_size(n);
    if (rc != PT_OK || (rc = check_samples(rgb, static_cast<size_t>(n) * n * 3, "the map")) != PT_OK) return rc;
    auto map = std::make_shared<pt_env_map>();
    map->n = n;
    map->rgb.assign(rgb, rgb + static_cast<size_t>(n) * n * 3);
    out = std::move(map);
    return PT_OK;
}

// A setter on one handle or on every device's copy of a frame's scene: the skybox check on all of them first, then the map is made
// ONCE (make), then each handle takes it (the map is shared; each device gets its own copy of the texels).
template <class Make>
int set_on(pt_scene *const *scenes, size_t n_scenes, bool removal, Make &&make) {
    for (size_t i = 0; i < n_scenes; ++i) {
        if (!scenes[i]) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
        if (scenes[i]->sky && !removal) return fail(PT_ERR_INVALID_ARGUMENT, kHasSkybox);
    }
    // (environment sampling: the handle keeps an environment while the switch is on, and a new one brings its table with it)
    bool sampled = false;
    for (size_t i = 0; i < n_scenes; ++i) sampled = sampled || scenes[i]->surface.envdirect;
    if (sampled && removal) return fail(PT_ERR_INVALID_ARGUMENT, "environment: the scene handle has environment sampling switched on; clear it first");
    std::shared_ptr<pt_env_map> map;
    if (!removal) {
        const int rc = make(map);
        if (rc != PT_OK) return rc;
    }
    ptc::EnvSamplingRebuild rebuild;
    if (sampled) {
        const int rc = ptc::envdirect_prepare(scenes, n_scenes, *map, rebuild);
        if (rc != PT_OK) return rc;
    }
    for (size_t i = 0; i < n_scenes; ++i) {
        if (removal && scenes[i]->sky) continue;   // (there is none to remove)
        const int rc = install(scenes[i], map);
        if (rc != PT_OK) return rc;
        if (sampled) ptc::envdirect_commit(scenes[i], i, rebuild);
    }
    return PT_OK;
}

int set_file_impl(pt_scene *const *scenes, size_t n, const char *path, const pt_environment_params *p) {
    const bool removal = !path || !*path;
    return set_on(scenes, n, removal, [&](std::shared_ptr<pt_env_map> &m) { return map_from_file(path, p, m); });
}
int set_equirect_impl(pt_scene *const *scenes, size_t n, int32_t w, int32_t h, const float *rgb, const pt_environment_params *p) {
    return set_on(scenes, n, false, [&](std::shared_ptr<pt_env_map> &m) { return map_from_equirect(w, h, rgb, p, m); });
}
int set_map_impl(pt_scene *const *scenes, size_t n_scenes, int32_t n, const float *rgb) {
    return set_on(scenes, n_scenes, false, [&](std::shared_ptr<pt_env_map> &m) { return map_from_map(n, rgb, m); });
}

int get_impl(const pt_scene *scene, int32_t *n, float *rgb) {
    if (!scene || !n) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *n = scene->env ? scene->env->n : 0;
    if (rgb && scene->env) std::memcpy(rgb, scene->env->rgb.data(), scene->env->rgb.size() * sizeof(float));
    return PT_OK;
}

int from_equirect_impl(int32_t w, int32_t h, const float *rgb, const pt_environment_params *p, int32_t n, float *map_rgb) {
    if (!map_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_picture(w, h, rgb);
    float gain, rotate;
    int n_default;
    if (rc != PT_OK || (rc = check_params(p, h, gain, rotate, n_default)) != PT_OK || (rc = check_map_size(n)) != PT_OK) return rc;
    pt::env_from_equirect(w, h, rgb, gain, rotate, n, map_rgb);
    return PT_OK;
}

int lookup_impl(int32_t n, const float *map_rgb, int32_t n_dirs, const float *directions, float *rgb) {
    if (!map_rgb || n_dirs < 0 || (n_dirs > 0 && (!directions || !rgb))) return fail(PT_ERR_INVALID_ARGUMENT, "null argument or negative count");
    const int rc = check_map_size(n);
    if (rc != PT_OK) return rc;
    const std::vector<pt::EnvTexel> t = pt::env_with_apron(n, map_rgb);
    for (int32_t i = 0; i < n_dirs; ++i)
        pt::env_lookup(t.data(), n, directions[3 * i], directions[3 * i + 1], directions[3 * i + 2], rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_set_environment_file(pt_scene *scene, const char *path, const pt_environment_params *params) {
    return guarded([&] { return set_file_impl(&scene, 1, path, params); });
}

int pt_scene_set_environment_equirect(pt_scene *scene, int32_t w, int32_t h, const float *rgb, const pt_environment_params *params) {
    return guarded([&] { return set_equirect_impl(&scene, 1, w, h, rgb, params); });
}

int pt_scene_set_environment_map(pt_scene *scene, int32_t n, const float *rgb) {
    return guarded([&] { return set_map_impl(&scene, 1, n, rgb); });
}

int pt_scene_get_environment(const pt_scene *scene, int32_t *n, float *rgb) {
    return guarded([&] { return get_impl(scene, n, rgb); });
}

// The same on a frame: every device's copy of its scene takes the map, which is read and converted once.
int pt_frame_set_environment_file(pt_frame *frame, const char *path, const pt_environment_params *params) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_file_impl(sc, n_sc, path, params); });
}

int pt_frame_set_environment_equirect(pt_frame *frame, int32_t w, int32_t h, const float *rgb, const pt_environment_params *params) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_equirect_impl(sc, n_sc, w, h, rgb, params); });
}

int pt_frame_set_environment_map(pt_frame *frame, int32_t n, const float *rgb) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_map_impl(sc, n_sc, n, rgb); });
}

int pt_frame_get_environment(pt_frame *frame, int32_t *n, float *rgb) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, n, rgb); });
}

int pt_environment_from_equirect(int32_t w, int32_t h, const float *rgb, const pt_environment_params *params, int32_t n, float *map_rgb) {
    return guarded([&] { return from_equirect_impl(w, h, rgb, params, n, map_rgb); });
}

int pt_environment_lookup(int32_t n, const float *map_rgb, int32_t n_dirs, const float *directions, float *rgb) {
    return guarded([&] { return lookup_impl(n, map_rgb, n_dirs, directions, rgb); });
}

}  // extern "C"
