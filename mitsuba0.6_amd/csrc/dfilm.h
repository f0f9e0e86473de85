// dfilm.h -- a sample into the film: ImageBlock::put (include/mitsuba/render/imageblock.h:
// 124-204) as the sample's own-pixel record in the splat buffer plus neighbour splats, or as
// the gather mode's record (film_kernel.hip sums and gathers them).  Included by dpath.h.
#pragma once

// ---------------------------------------------------------------------------
// film splat: ImageBlock::put (render/imageblock.h:124-204) into the 32x32
// block that owns pixel (px, py); own-pixel weight goes to the lane's
// registers, other touched pixels to the spill film (double atomics)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float filter_disc(const MtsgFilter &F, float x) {
    int i = (int)fabsf(x * F.scale);
    if (MTSG_FILTER_RES < i) i = MTSG_FILTER_RES;
    return F.values[i];
}

// WARN = false: an ImageBlock built with warnInvalid off (the multichannel integrator's,
// multichannel.cpp:143-145) takes negative and non-finite values as they are.
// spill: the neighbour-splat film, L.film_spill unless given (the field pass has one per field)
template <bool WARN = true>
__device__ __forceinline__ bool film_splat(const MtsgLaunch &L, int px, int py, float sx, float sy,
                                           const float *val, float &ownW, double *spill = nullptr) {
    if constexpr (WARN) {
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (!isfinite(val[i]) || val[i] < 0) return false;
    }
    const MtsgFilter &F = L.filter;
    const int b = F.border;
    const int bx = (px / MTSG_BLOCK_SIZE) * MTSG_BLOCK_SIZE, by = (py / MTSG_BLOCK_SIZE) * MTSG_BLOCK_SIZE;
    const int bw = MTSG_BLOCK_SIZE + 2 * b;
    const float posx = sx - 0.5f - (float)(bx - b), posy = sy - 0.5f - (float)(by - b);
    int minx = (int)ceilf(posx - F.radius), miny = (int)ceilf(posy - F.radius);
    int maxx = (int)floorf(posx + F.radius), maxy = (int)floorf(posy + F.radius);
    if (minx < 0) minx = 0;
    if (miny < 0) miny = 0;
    if (maxx > bw - 1) maxx = bw - 1;
    if (maxy > bw - 1) maxy = bw - 1;
    for (int y = miny; y <= maxy; ++y) {
        const float wy = filter_disc(F, (float)y - posy);
        for (int x = minx; x <= maxx; ++x) {
            const float weight = filter_disc(F, (float)x - posx) * wy;
            const int gx = x + bx, gy = y + by;
            if (gx >= L.fw || gy >= L.fh) continue;
            if (gx == px + b && gy == py + b) {
                ownW = weight;
            } else {
                // weight * value[k] in float as the reference forms it, summed in double
                // (film_finalize rounds once).  The total does not depend on the order the
                // atomics land while every partial sum is exact: with q the smallest exponent
                // of a lowest set mantissa bit over a film value's contributions, that is
                // sum|c| < 2^(q + 53).  Box filters and a gaussian of stddev 0.1 meet it in every
                // film value; a gaussian with a 121- or 169-pixel footprint (stddev 1.13, 1.5)
                // leaves it in about a sixth of its film pixels (C1 40 x 36: 380 of 2300, 475
                // of 2496), where two orders' totals can differ in the last bits of the double
                // and the film by one float ulp (tests/film_ref.py, tests/test_gpu_filter_widths.py)
                double *dst = (spill ? spill : L.film_spill) + ((size_t)gy * L.fw + gx) * 5;
#pragma unroll
                for (int k = 0; k < 5; ++k) atomicAdd(dst + k, (double)(weight * val[k]));
            }
        }
    }
    return true;
}

// block->put(samplePos, spec, alpha) (integrator.cpp:184) as the sample's record in
// the splat buffer (slot = (j - j0) * num_pixels + pix).  Box filter: {L.rgb, w} with
// the own-pixel weight w (alpha in {0,1} in its sign bit; film_reduce re-forms
// weight * value[k]) and the rare neighbour splats as atomics.  Gather mode: the
// sample's value and film position, {L.rgb, sx (alpha in its sign bit: sx >= +0)}
// and {sy (-1: an invalid sample, which ImageBlock::put drops whole), 0, 0, 0} in one
// 32 B record: HBM writes whole 32 B sectors (profiles/r06_write_gran), so the
// record costs what a lone 16 B store costs, where a separate 4 B sy array cost
// another sector; film_gather forms every footprint weight with film_splat's arithmetic.
#ifndef MTSG_SPLAT_PAIR
#define MTSG_SPLAT_PAIR 1
#endif
// the record slot of sample jj (= j - j0) of compact pixel pix.  Box filter: the records
// of samples 2k and 2k+1 of a pixel share one 32 B sector (the lanes that write them
// run at different times; the sector is written to HBM once if both halves meet in L2).
// Gather mode: one 32 B record per slot.
__device__ __forceinline__ size_t film_slot(const MtsgLaunch &L, uint32_t jj, uint32_t pix) {
    if (MTSG_SPLAT_PAIR && !L.gather) return ((size_t)(jj >> 1) * L.num_pixels + pix) * 2 + (jj & 1);
    return (size_t)jj * L.num_pixels + pix;
}

template <bool WARN = true>
__device__ __forceinline__ void film_record(const MtsgLaunch &L, size_t slot, int px, int py, float sx, float sy,
                                            const float *val, bool alpha, double *spill = nullptr) {
    float4 rec4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (L.gather) {
        bool valid = true;
        if constexpr (WARN) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (!isfinite(val[i]) || val[i] < 0) valid = false;   // (alpha and 1 are valid)
        }
        if (valid) rec4 = make_float4(val[0], val[1], val[2], alpha ? sx : -sx);
        float4 *r = reinterpret_cast<float4 *>(L.contrib) + 2 * slot;
        r[0] = rec4;
        r[1] = make_float4(valid ? sy : -1.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float ownW = 0.0f;
    if (film_splat<WARN>(L, px, py, sx, sy, val, ownW, spill)) rec4 = make_float4(val[0], val[1], val[2], alpha ? ownW : -ownW);
    reinterpret_cast<float4 *>(L.contrib)[slot] = rec4;
}
