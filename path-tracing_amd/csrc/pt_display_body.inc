// The statements of the display kernel (pt_display.hip states what they do), included between the braces of the ungraded kernel
// there and of the graded one in pt_display_graded.hip -- as text, so that the ungraded kernel is compiled from exactly the
// tokens it always had.  Names from outside: a (DisplayArgs), DIVIDE; with PT_DISPLAY_GRADED defined also CURVE (a PT_CURVE_* of
// pt_grade.hpp) and exposure (a device scalar).  Then every channel becomes g = curve(m * *exposure) between the optional divide
// and the out-of-table test: what is looked up, compared and deferred on is g, while a deferred entry still carries the ungraded
// mean -- the host finishes such a pixel with the same pt_grade.hpp, so a NaN's payload never has to agree between host and device.
// With PT_DISPLAY_COLOUR defined as well (pt_display_colour.hip) also LUT (a bool) and colour (a ColourStep of pt_colour.hpp): g is
// then what matrix -> exposure -> curve -> LUT makes of the pixel, and a deferred entry carries the mean before the matrix.
// With PT_DISPLAY_GRAIN defined as well (pt_display_grain.hip) also SIZED (a bool) and grain (a GrainStep of pt_grain.hpp): g then
// takes the pixel's grain before the out-of-table test, and the level of a channel the table covers is dithered between T[k - 1] and
// T[k].  A lane's four pixels are consecutive in the flat plane: one division gives the first one's (x, y), the others follow along
// the row and wrap at its end.
    __shared__ __attribute__((aligned(16))) float T[kDisplayTableSize];
    for (int i = threadIdx.x; i < kDisplayTableSize / 4; i += kDisplayBlock)
        reinterpret_cast<float4 *>(T)[i] = reinterpret_cast<const float4 *>(a.table)[i];
    __syncthreads();
#ifdef PT_DISPLAY_GRADED
    const float e = *exposure;
#endif
    const int n_groups = (a.n + 3) / 4;
    for (int g = blockIdx.x * kDisplayBlock + threadIdx.x; g < n_groups; g += gridDim.x * kDisplayBlock) {
        const int p0 = 4 * g;
        float m[12];
        int32_t c[4];
        if (p0 + 4 <= a.n) {
            const float4 *src = reinterpret_cast<const float4 *>(a.rgb + 3 * static_cast<size_t>(p0));
            const float4 v0 = src[0], v1 = src[1], v2 = src[2];
            const int4 cc = *reinterpret_cast<const int4 *>(a.count + p0);
            m[0] = v0.x; m[1] = v0.y; m[2] = v0.z; m[3] = v0.w; m[4] = v1.x; m[5] = v1.y; m[6] = v1.z; m[7] = v1.w;
            m[8] = v2.x; m[9] = v2.y; m[10] = v2.z; m[11] = v2.w;
            c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w;
        } else {   // the tail of the plane: one to three pixels
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = p0 + j;
                const bool inside = p < a.n;
                c[j] = inside ? a.count[p] : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) m[3 * j + k] = inside ? a.rgb[3 * static_cast<size_t>(p) + k] : 0.0f;
            }
        }
        if (DIVIDE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float n = static_cast<float>(c[j]);
#pragma unroll
                for (int k = 0; k < 3; ++k) m[3 * j + k] = m[3 * j + k] / n;   // (count == 0: never looked at)
            }
        }
#ifdef PT_DISPLAY_GRADED
        float mean[12];   // what a deferred entry carries: the ungraded mean
#ifdef PT_DISPLAY_COLOUR
#pragma unroll
        for (int i = 0; i < 12; ++i) mean[i] = m[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // matrix -> exposure -> curve -> LUT (pt_colour.hpp); the LUT's loads are in bounds for any value
            if (colour.apply_matrix) colour_matrix_apply(colour.m, m[3 * j], m[3 * j + 1], m[3 * j + 2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) m[3 * j + k] = grade_value<CURVE>(m[3 * j + k], e);
            if (LUT) colour_lut_apply(colour.lut, colour.lut_n, m[3 * j], m[3 * j + 1], m[3 * j + 2]);
        }
#else
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            mean[i] = m[i];
            m[i] = grade_value<CURVE>(m[i], e);
        }
#endif
#endif
#ifdef PT_DISPLAY_GRAIN
        uint32_t px_x[4], px_y[4];
        {
            const uint32_t width = static_cast<uint32_t>(grain.width);
            uint32_t y = static_cast<uint32_t>(p0) / width, x = static_cast<uint32_t>(p0) - y * width;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                px_x[j] = x; px_y[j] = y;
                if (++x == width) { x = 0; ++y; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) grain_pixel<SIZED>(grain, px_x[j], px_y[j], m[3 * j], m[3 * j + 1], m[3 * j + 2]);
#endif
        bool out_of_table[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) out_of_table[i] = !(m[i] >= 0.0f) || m[i] >= a.last;
        for (int b = 0; b < a.n_bands; ++b) {
            const float lo = a.band_lo[b], hi = a.band_hi[b];
#pragma unroll
            for (int i = 0; i < 12; ++i) out_of_table[i] |= m[i] >= lo && m[i] < hi;
        }
        bool defer[4];
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool samples = c[j] != 0;
            defer[j] = samples && (out_of_table[3 * j] || out_of_table[3 * j + 1] || out_of_table[3 * j + 2]);
#ifdef PT_DISPLAY_GRAIN
            uint32_t level[3], word[3] = {0u, 0u, 0u};
            const bool dithered = grain.dither != 0.0f && samples && !defer[j];   // (a deferred pixel is the host's, dither and all)
            if (dithered) grain_dither_words(grain, px_x[j], px_y[j], word[0], word[1], word[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = m[3 * j + k];
                level[k] = display_level(T, v);
                // covered: level[k] thresholds lie at or below v and the next one, T[level[k]], is in use (v < a.last)
                if (dithered) level[k] = grain_dither_level(level[k], level[k] ? T[level[k] - 1] : 0.0f, T[level[k]], v, grain.dither, word[k]);
            }
            const uint32_t r = level[0] & 255u, gr = level[1] & 255u, bl = level[2] & 255u;
#else
            const uint32_t r = display_level(T, m[3 * j]) & 255u, gr = display_level(T, m[3 * j + 1]) & 255u,
                           bl = display_level(T, m[3 * j + 2]) & 255u;
#endif
            px[j] = samples && !defer[j] ? (bl | (gr << 8) | (r << 16)) : 0u;
        }
        // B G R B | G R B G | R B G R
        uint3 w;
        w.x = px[0] | (px[1] << 24);
        w.y = (px[1] >> 8) | (px[2] << 16);
        w.z = (px[2] >> 16) | (px[3] << 8);
        *reinterpret_cast<uint3 *>(a.bgr + 3 * static_cast<size_t>(g)) = w;

        if (__ballot(defer[0] || defer[1] || defer[2] || defer[3])) {   // rare: the whole wave skips it otherwise
            const uint32_t lane = __lane_id();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long mask = __ballot(defer[j]);
                if (!mask) continue;
                const int leader = __ffsll(mask) - 1;
                uint32_t base = 0;
                if (static_cast<int>(lane) == leader) base = atomicAdd(a.n_deferred, static_cast<uint32_t>(__popcll(mask)));
                base = __shfl(base, leader);
                if (defer[j]) {   // every pixel is appended at most once, so the list never outgrows its n entries
                    const uint32_t at = base + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
#ifdef PT_DISPLAY_GRADED
                    reinterpret_cast<float4 *>(a.deferred)[at] = make_float4(__int_as_float(p0 + j), mean[3 * j], mean[3 * j + 1], mean[3 * j + 2]);
#else
                    reinterpret_cast<float4 *>(a.deferred)[at] = make_float4(__int_as_float(p0 + j), m[3 * j], m[3 * j + 1], m[3 * j + 2]);
#endif
                }
            }
        }
    }
