// ldrfilm_kernel.hip -- ldrfilm develop on the device.
//
// LDRFilm::develop (src/films/ldrfilm.cpp:300-321) turns the film's
// SpectrumAlphaWeight storage into 8-bit pixels in one of two ways:
//   gamma    : Bitmap::convert(pixelFormat, EUInt8, gamma, powf(2, exposure))
//   reinhard : Bitmap::convert(pixelFormat, EFloat), Bitmap::tonemapReinhard in
//              place (src/libcore/bitmap.cpp:1711-1854), then
//              Bitmap::convert(pixelFormat, EUInt8, gamma, 1)
// The conversions are FormatConverterImpl's (src/libcore/fmtconv.cpp:955-1005:
// invWeight = weight != 0 ? 1/weight : weight, luminance of the spectrum times
// invWeight or the spectrum times invWeight, alpha * invWeight) and
// convertScalar's (fmtconv.cpp:1137-1160): value * multiplier, applyGamma
// (fmtconv.cpp:1104-1111) unless 1/gamma is 1, min(255, max(0, value * 255 +
// 0.5f)) cast to uint8_t; alpha with neither multiplier nor gamma.  std::pow on
// floats is glibc's powf (glibc_f32.h), math::fastlog / fastexp are double
// log / exp (dmath.h).  The film interior is addressed as film_kernel.hip does.
//
// Three kernels for the reinhard method:
//   ldr_lum_kernel      per pixel, the luminance as bitmap.cpp:1744 (RGB[A]: of
//                       the developed r, g, b) or :1763 (monochrome: the developed
//                       value) forms it and the term fastlog(1e-3f + luminance),
//                       both to scratch; a luminance of exactly 1024 records its
//                       pixel number (the maximum's reset, bitmap.cpp:1745-1746)
//   ldr_reduce_kernel   one workgroup.  Wave 0 forms the float sum of the terms in
//                       pixel order -- a serial chain, float addition is not
//                       associative -- with the loads taken off the chain: the wave
//                       fetches 256 consecutive terms per 16-byte load, with three more
//                       such loads in flight, and every lane adds them in order out of
//                       the lanes' registers (v_readlane), so all 64 lanes hold the
//                       sequential sum: about 8 cycles per term.  Waves 1-3 meanwhile
//                       take the maximum luminance over the pixels from the last
//                       exactly-1024 one on, which is what the sequential loop's reset
//                       leaves.  Thread 0 then forms
//                       logAvgLuminance, scale and invWp2 (bitmap.cpp:1772-1784).
//   develop_ldr_kernel  per pixel: develop, tonemap (bitmap.cpp:1788-1853) unless the
//                       image is black (bitmap.cpp:1775), gamma, uint8.
// The gamma method is develop_ldr_kernel alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mtsgpu.h"
#include "dmath.h"
#include "launchers.h"

namespace {

constexpr int LDR_BLOCK = 256;
constexpr size_t LDR_HEADER = 256;   // scratch: {last1024, LdrTone}, then terms[n4], luminance[n4]
constexpr size_t LDR_TONE_OFFSET = 16;

struct LdrTone { float logAvg, maxLum, scale, invWp2; };

template <int PIX> struct Chan {
    static constexpr int C = (PIX == MTSGPU_PIX_LUMINANCE) ? 1 : (PIX == MTSGPU_PIX_LUMINANCE_ALPHA) ? 2
                           : (PIX == MTSGPU_PIX_RGB) ? 3 : 4;
    static constexpr bool mono = PIX == MTSGPU_PIX_LUMINANCE || PIX == MTSGPU_PIX_LUMINANCE_ALPHA;
};

// Bitmap::convert(pixelFormat, EFloat) of pixel i (fmtconv.cpp:955-1005): v[0] (monochrome)
// or v[0..2] (RGB), and the alpha value
template <int PIX>
__device__ __forceinline__ void develop_px(const float *__restrict__ film, uint32_t full_w, uint32_t border,
                                           uint32_t w, size_t i, float v[3], float &a) {
    const uint32_t y = (uint32_t)(i / w), x = (uint32_t)(i - (size_t)y * w);
    const float *px = film + ((size_t)(y + border) * full_w + (x + border)) * 5;
    const float s0 = px[0], s1 = px[1], s2 = px[2], alpha = px[3], weight = px[4];
    const float inv = (weight != 0.0f) ? 1.0f / weight : weight;
    if constexpr (Chan<PIX>::mono) {
        v[0] = (s0 * 0.212671f + s1 * 0.715160f + s2 * 0.072169f) * inv;
    } else {
        v[0] = s0 * inv;
        v[1] = s1 * inv;
        v[2] = s2 * inv;
    }
    a = alpha * inv;
}

template <int PIX>
__global__ __launch_bounds__(LDR_BLOCK) void ldr_lum_kernel(const float *__restrict__ film, uint32_t full_w,
                                                            uint32_t border, uint32_t w, uint32_t h,
                                                            float *__restrict__ terms, float *__restrict__ lums,
                                                            unsigned long long *__restrict__ last1024) {
    const size_t n = (size_t)w * h;
    for (size_t i = (size_t)blockIdx.x * LDR_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * LDR_BLOCK) {
        float v[3], a;
        develop_px<PIX>(film, full_w, border, w, i, v, a);
        float lum;
        if constexpr (Chan<PIX>::mono) lum = v[0];
        else lum = v[0] * 0.212671f + v[1] * 0.715160f + v[2] * 0.072169f;
        lums[i] = lum;
        terms[i] = d_fastlog(1e-3f + lum);
        if (lum == 1024.0f) atomicMax(last1024, (unsigned long long)i + 1);
    }
}

// A lane's terms 256 * chunk + 4 * lane .. + 3, in two steps, so that the load can be pinned in
// front of the 256 adds that hide it (the scheduler otherwise sinks it to its use).  No branch:
// the address is clamped to the last four floats of the array (its length is a multiple of
// four; the floats past n are never written), and ldr_mask_terms puts +0 where the index is
// past n.  The running sum starts at +0, and a float sum is -0 only when both addends are, so
// it is never -0 and adding +0 leaves its bits alone (NaN and infinity included).
__device__ __forceinline__ float4 ldr_load_terms(const float *__restrict__ terms, size_t n, size_t chunk, int lane) {
    const size_t i = chunk * 256 + 4 * (size_t)lane, last = (n + 3) / 4 * 4 - 4;
    const float4 r = *reinterpret_cast<const float4 *>(terms + (i < last ? i : last));
    __builtin_amdgcn_sched_barrier(0);
    return r;
}

__device__ __forceinline__ float4 ldr_mask_terms(float4 r, size_t n, size_t chunk, int lane) {
    const size_t i = chunk * 256 + 4 * (size_t)lane;
    r.x = i < n ? r.x : 0.0f;
    r.y = i + 1 < n ? r.y : 0.0f;
    r.z = i + 2 < n ? r.z : 0.0f;
    r.w = i + 3 < n ? r.w : 0.0f;
    return r;
}

__device__ __forceinline__ float ldr_lane(float v, int k) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// acc + the wave's 256 terms in order: lane 0's four, lane 1's four, ...  Sixteen terms are
// read out of the lanes ahead of their adds, so that the chain waits for the add before it
// alone and not for a v_readlane as well.
__device__ __forceinline__ float ldr_consume(float acc, float4 b) {
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
        float t[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[4 * j] = ldr_lane(b.x, k + j);
            t[4 * j + 1] = ldr_lane(b.y, k + j);
            t[4 * j + 2] = ldr_lane(b.z, k + j);
            t[4 * j + 3] = ldr_lane(b.w, k + j);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) acc += t[j];
    }
    return acc;
}

__global__ __launch_bounds__(LDR_BLOCK) void ldr_reduce_kernel(const float *__restrict__ terms,
                                                               const float *__restrict__ lums, size_t n, float key,
                                                               float burn,
                                                               const unsigned long long *__restrict__ last1024,
                                                               LdrTone *__restrict__ tone) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc = 0.0f;
    if (wave == 0) {
        const size_t chunks = (n + 255) / 256;
        float4 b0 = ldr_load_terms(terms, n, 0, lane), b1 = ldr_load_terms(terms, n, 1, lane);
        float4 b2 = ldr_load_terms(terms, n, 2, lane), b3 = ldr_load_terms(terms, n, 3, lane);
        for (size_t c = 0; c < chunks; c += 4) {
            acc = ldr_consume(acc, ldr_mask_terms(b0, n, c, lane));
            b0 = ldr_load_terms(terms, n, c + 4, lane);
            acc = ldr_consume(acc, ldr_mask_terms(b1, n, c + 1, lane));
            b1 = ldr_load_terms(terms, n, c + 5, lane);
            acc = ldr_consume(acc, ldr_mask_terms(b2, n, c + 2, lane));
            b2 = ldr_load_terms(terms, n, c + 6, lane);
            acc = ldr_consume(acc, ldr_mask_terms(b3, n, c + 3, lane));
            b3 = ldr_load_terms(terms, n, c + 7, lane);
        }
    } else {
        // std::max(maxLuminance, luminance) from 0 on: NaN and negative luminances never enter, so
        // the values are ordered as their bit patterns and the order of the pixels does not matter
        const unsigned long long last = *last1024;
        float m = 0.0f;
        for (size_t i = (last ? (size_t)last - 1 : 0) + (threadIdx.x - 64); i < n; i += LDR_BLOCK - 64)
            m = smax(m, lums[i]);
        atomicMax(&s_max, __float_as_uint(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        LdrTone T;
        T.maxLum = __uint_as_float(s_max);
        T.logAvg = d_fastexp(acc / (float)n);
        const float b = smin(1.0f, smax(1e-8f, 1.0f - burn));
        T.scale = key / T.logAvg;
        const float Lwhite = T.maxLum * T.scale;
        T.invWp2 = 1.0f / (Lwhite * Lwhite * d_powf(b, 4.0f));
        *tone = T;
    }
}

__device__ __forceinline__ float ldr_apply_gamma(float value, float invGamma) {   // fmtconv.cpp:1104-1111
    if (invGamma == -1.0f)
        return (value <= 0.0031308f) ? (12.92f * value) : (1.055f * d_powf(value, (float)(1.0 / 2.4)) - 0.055f);
    return d_powf(value, invGamma);
}

// convertScalar<uint8_t> (fmtconv.cpp:1137-1160); a NaN becomes 0 by std::max's argument order
__device__ __forceinline__ uint32_t ldr_u8(float value, float mult, float invGamma) {
    value = value * mult;
    if (invGamma != 1.0f) value = ldr_apply_gamma(value, invGamma);
    return (uint32_t)(int32_t)smin(255.0f, smax(0.0f, value * 255.0f + 0.5f));
}

__device__ __forceinline__ uint32_t ldr_u8_alpha(float value) {
    return (uint32_t)(int32_t)smin(255.0f, smax(0.0f, value * 255.0f + 0.5f));
}

template <int PIX, bool REINHARD>
__global__ __launch_bounds__(LDR_BLOCK) void develop_ldr_kernel(const float *__restrict__ film, uint32_t full_w,
                                                                uint32_t border, uint32_t w, uint32_t h, float gamma,
                                                                float exposure, const LdrTone *__restrict__ tone,
                                                                uint8_t *__restrict__ out) {
    constexpr int C = Chan<PIX>::C;
    const size_t n = (size_t)w * h;
    const float invGamma = 1.0f / gamma;                               // fmtconv.cpp:148
    const float mult = REINHARD ? 1.0f : d_powf(2.0f, exposure);       // ldrfilm.cpp:318
    float scale = 0.0f, invWp2 = 0.0f;
    bool black = true;
    if constexpr (REINHARD) {
        scale = tone->scale;
        invWp2 = tone->invWp2;
        black = tone->maxLum == 0.0f;                                  // bitmap.cpp:1775
    }
    for (size_t i = (size_t)blockIdx.x * LDR_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * LDR_BLOCK) {
        float v[3], a;
        develop_px<PIX>(film, full_w, border, w, i, v, a);
        if (REINHARD && !black) {
            if constexpr (Chan<PIX>::mono) {                           // bitmap.cpp:1845-1852
                const float Lp = v[0] * scale;
                v[0] = Lp * (1.0f + Lp * invWp2) / (1.0f + Lp);
            } else {                                                   // bitmap.cpp:1788-1814
                float X = v[0] * 0.412453f + v[1] * 0.357580f + v[2] * 0.180423f;
                float Y = v[0] * 0.212671f + v[1] * 0.715160f + v[2] * 0.072169f;
                float Z = v[0] * 0.019334f + v[1] * 0.119193f + v[2] * 0.950227f;
                const float normalization = 1.0f / (X + Y + Z), x = X * normalization, y = Y * normalization,
                            Lp = Y * scale;
                Y = Lp * (1.0f + Lp * invWp2) / (1.0f + Lp);
                const float ratio = Y / y;
                X = ratio * x;
                Z = ratio * (1.0f - x - y);
                v[0] = 3.240479f * X + -1.537150f * Y + -0.498535f * Z;
                v[1] = -0.969256f * X + 1.875991f * Y + 0.041556f * Z;
                v[2] = 0.055648f * X + -0.204043f * Y + 1.057311f * Z;
            }
        }
        uint8_t *o = out + i * C;
        if constexpr (PIX == MTSGPU_PIX_LUMINANCE) {
            o[0] = (uint8_t)ldr_u8(v[0], mult, invGamma);
        } else if constexpr (PIX == MTSGPU_PIX_LUMINANCE_ALPHA) {      // one 16-bit store
            *reinterpret_cast<uint16_t *>(o) = (uint16_t)(ldr_u8(v[0], mult, invGamma) | ldr_u8_alpha(a) << 8);
        } else {
            const uint32_t r = ldr_u8(v[0], mult, invGamma), g = ldr_u8(v[1], mult, invGamma),
                           b = ldr_u8(v[2], mult, invGamma);
            if constexpr (PIX == MTSGPU_PIX_RGBA) {                    // one 32-bit store
                *reinterpret_cast<uint32_t *>(o) = r | g << 8 | b << 16 | ldr_u8_alpha(a) << 24;
            } else {
                o[0] = (uint8_t)r;
                o[1] = (uint8_t)g;
                o[2] = (uint8_t)b;
            }
        }
    }
}

template <int PIX>
hipError_t launch_ldr(const mtsgpu_develop_ldr_params &P, const float *film, uint8_t *out, void *scratch, int grid,
                      hipStream_t s) {
    const uint32_t b = P.border, w = P.film_width - 2 * b, h = P.film_height - 2 * b;
    if (P.tonemap_method == MTSGPU_TONEMAP_GAMMA) {
        develop_ldr_kernel<PIX, false><<<grid, LDR_BLOCK, 0, s>>>(film, P.film_width, b, w, h, P.gamma, P.exposure,
                                                                   nullptr, out);
        return hipGetLastError();
    }
    const size_t n = (size_t)w * h, n4 = (n + 3) / 4 * 4;
    unsigned long long *last = (unsigned long long *)scratch;
    LdrTone *tone = (LdrTone *)((char *)scratch + LDR_TONE_OFFSET);
    float *terms = (float *)((char *)scratch + LDR_HEADER), *lums = terms + n4;
    hipError_t e = hipMemsetAsync(scratch, 0, LDR_HEADER, s);
    if (e != hipSuccess) return e;
    ldr_lum_kernel<PIX><<<grid, LDR_BLOCK, 0, s>>>(film, P.film_width, b, w, h, terms, lums, last);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ldr_reduce_kernel<<<1, LDR_BLOCK, 0, s>>>(terms, lums, n, P.key, P.burn, last, tone);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    develop_ldr_kernel<PIX, true><<<grid, LDR_BLOCK, 0, s>>>(film, P.film_width, b, w, h, P.gamma, P.exposure, tone,
                                                              out);
    return hipGetLastError();
}

}  // namespace

// bytes of device scratch mtsg_launch_develop_ldr needs (0: none)
size_t mtsg_develop_ldr_scratch(const mtsgpu_develop_ldr_params &P) {
    if (P.tonemap_method != MTSGPU_TONEMAP_REINHARD) return 0;
    const size_t n = (size_t)(P.film_width - 2 * P.border) * (P.film_height - 2 * P.border);
    return LDR_HEADER + 2 * ((n + 3) / 4 * 4) * sizeof(float);
}

// where in the scratch {logAvgLuminance, maxLuminance} stand after a reinhard develop
size_t mtsg_develop_ldr_info_offset() { return LDR_TONE_OFFSET; }

hipError_t mtsg_launch_develop_ldr(const mtsgpu_develop_ldr_params &P, const float *film, uint8_t *out, void *scratch,
                                   int num_cus, hipStream_t s) {
    const uint32_t b = P.border, w = P.film_width - 2 * b, h = P.film_height - 2 * b;
    const size_t n = (size_t)w * h;
    const size_t want = (n + LDR_BLOCK - 1) / LDR_BLOCK, cap = (size_t)std::max(num_cus, 1) * 16;
    const int grid = (int)std::max<size_t>(1, std::min(want, cap));
    switch (P.pixel_format) {
        case MTSGPU_PIX_LUMINANCE: return launch_ldr<MTSGPU_PIX_LUMINANCE>(P, film, out, scratch, grid, s);
        case MTSGPU_PIX_LUMINANCE_ALPHA: return launch_ldr<MTSGPU_PIX_LUMINANCE_ALPHA>(P, film, out, scratch, grid, s);
        case MTSGPU_PIX_RGB: return launch_ldr<MTSGPU_PIX_RGB>(P, film, out, scratch, grid, s);
        case MTSGPU_PIX_RGBA: return launch_ldr<MTSGPU_PIX_RGBA>(P, film, out, scratch, grid, s);
    }
    return hipErrorInvalidValue;
}
