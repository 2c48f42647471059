// The 24-bit BMP reader of the skybox (pt_scene_set_skybox_bmp) and of pt_texture_load_bmp: bitmap_image(filename) -> load_bitmap(),
// bitmap_image.hpp:1508-1603 of the reference -- the same checks, reported instead of printed.  Host only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace pt {

// texels = B, G, R bytes, rows top-down, no padding.  false: `why` says what is wrong; cannot_open = the file could not be opened.
inline bool read_bmp24(const char *path, std::vector<uint8_t> &texels, int &w, int &h, std::string &why, bool &cannot_open) {
    cannot_open = false;
    why.clear();
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        cannot_open = true;
        why = std::string("cannot open ") + path;
        return false;
    }
    uint8_t hdr[54];
    const bool got = std::fread(hdr, 1, 54, f) == 54;
    auto u16 = [&](int at) { return static_cast<uint32_t>(hdr[at]) | (static_cast<uint32_t>(hdr[at + 1]) << 8); };
    auto u32 = [&](int at) { return u16(at) | (u16(at + 2) << 16); };
    if (!got) why = "file shorter than its headers";
    else if (u16(0) != 19778) why = "invalid type value " + std::to_string(u16(0)) + " expected 19778";
    else if (u16(28) != 24) why = "invalid bit depth " + std::to_string(u16(28)) + " expected 24";
    else if (u32(14) != 40) why = "invalid BIH size " + std::to_string(u32(14)) + " expected 40";
    if (why.empty()) {
        const uint32_t uw = u32(18), uh = u32(22);
        const uint32_t pad = (4u - (3u * uw) % 4u) % 4u;
        std::fseek(f, 0, SEEK_END);
        const size_t physical = static_cast<size_t>(std::ftell(f));
        const size_t logical = static_cast<size_t>(uh) * uw * 3 + static_cast<size_t>(uh) * pad + 54;
        if (physical != logical || uw == 0 || uh == 0) {
            why = "mismatch between logical (" + std::to_string(logical) + ") and physical (" + std::to_string(physical) + ") sizes";
        } else {
            texels.resize(static_cast<size_t>(uw) * uh * 3);
            std::fseek(f, 54, SEEK_SET);
            uint8_t padbuf[4];
            for (uint32_t i = 0; i < uh && why.empty(); ++i) {   // rows are stored bottom-up
                if (std::fread(&texels[static_cast<size_t>(uh - i - 1) * uw * 3], 1, static_cast<size_t>(uw) * 3, f) != static_cast<size_t>(uw) * 3 ||
                    (pad && std::fread(padbuf, 1, pad, f) != pad))
                    why = "short read";
            }
            w = static_cast<int>(uw);
            h = static_cast<int>(uh);
        }
    }
    std::fclose(f);
    return why.empty();
}

}  // namespace pt
