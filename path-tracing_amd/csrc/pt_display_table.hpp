// The threshold table of the display path (include/pt_hip.h: pt_display_table), host only: built from whatever function says
// "the host's tone map puts m at level k or above" -- the library passes its own pow; a test passes one that is not monotone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ptc {

// ---- the table ------------------------------------------------------------------------------------------------------------
// L(m) = (int)(tonemap_value(m, gamma)) is what pt_quantize makes a byte of.  Threshold k (1 .. levels) is the smallest float
// with L >= k, found by bisection over the bit patterns of the non-negative finite floats -- which are ordered as the floats
// are.  "L >= k" is asked of the float product (v >= k): the same thing for an integer k while the conversion is defined, and
// still true where the product has outgrown an int.
struct DisplayTable {
    float gamma = 0;
    std::vector<float> thresholds;          // non-decreasing
    std::vector<float> doubt_lo, doubt_hi;   // per level: [lo, hi), lo == hi where the neighbourhood of the threshold is consistent
    std::vector<float> band_lo, band_hi;    // the non-empty ones, merged where they touch, ascending
};

constexpr int kDisplayMaxLevels = 4096;
constexpr uint32_t kMaxFiniteBits = 0x7f7fffffu;
constexpr int kDoubtNeighbours = 64;

inline float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

// `reaches(m, k)`: does the host's tone map put m at level k or above?  A template so that the builder can be tried on a
// function that is not monotone.
template <class Reaches>
void build_display_table(Reaches &&reaches, DisplayTable &t) {
    uint32_t from = 0;   // thresholds do not decrease: level k is searched from threshold k - 1 on
    for (int k = 1; k <= kDisplayMaxLevels; ++k) {
        if (!reaches(from_bits(kMaxFiniteBits), k)) break;   // no finite float reaches this level: the table ends here
        uint32_t lo = from, hi = kMaxFiniteBits;             // invariant: reaches(hi); the answer lies in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (reaches(from_bits(mid), k)) hi = mid;
            else lo = mid + 1;
        }
        from = lo;
        // pow need not be monotone to the last bit: the floats around the threshold must agree with "below: < k, at or above: >= k"
        uint32_t bad_lo = 0, bad_hi = 0;
        bool bad = false;
        const uint32_t first = lo > static_cast<uint32_t>(kDoubtNeighbours) ? lo - kDoubtNeighbours : 0;
        const uint32_t last = std::min(kMaxFiniteBits, lo + kDoubtNeighbours);
        for (uint32_t u = first; u <= last; ++u) {
            if (reaches(from_bits(u), k) == (u >= lo)) continue;
            if (!bad) bad_lo = u;
            bad_hi = u;
            bad = true;
        }
        t.thresholds.push_back(from_bits(lo));
        // [first disagreeing float, the float after the last one); at the top of the range the band ends at +inf
        t.doubt_lo.push_back(from_bits(bad ? bad_lo : lo));
        t.doubt_hi.push_back(from_bits(bad ? bad_hi + 1 : lo));
    }
    for (size_t k = 0; k < t.thresholds.size(); ++k) {
        if (!(t.doubt_lo[k] < t.doubt_hi[k])) continue;
        if (!t.band_lo.empty() && t.doubt_lo[k] <= t.band_hi.back()) {
            t.band_hi.back() = std::max(t.band_hi.back(), t.doubt_hi[k]);
        } else {
            t.band_lo.push_back(t.doubt_lo[k]);
            t.band_hi.push_back(t.doubt_hi[k]);
        }
    }
}

}  // namespace ptc
