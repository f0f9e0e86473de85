// dsampler.h -- the samplers on the device, and the address-space typedefs the device
// headers share: the Sobol sampler (src/samplers/sobol.cpp:147-258, include/mitsuba/core/
// sobolseq.h:43-130) through 4-bit XOR tables in LDS or HBM, the independent sampler
// (src/samplers/independent.cpp:82-104) as a counter-based stream or as the SFMT replay
// (sfmt.h), and the per-sample state with Sampler::next1D / next2D over them.
// Included by dpath.h.
#pragma once

typedef __attribute__((address_space(3))) const uint32_t lds_u32;     // LDS
typedef __attribute__((address_space(1))) const uint32_t glb_u32;     // global
typedef __attribute__((address_space(3))) const MtsgNode lds_node;
typedef __attribute__((address_space(1))) const MtsgNode glb_node;
typedef __attribute__((address_space(3))) const MtsgTri lds_tri;
typedef __attribute__((address_space(1))) const MtsgTri glb_tri;
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef int vi4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const vf4 lds_f4;
typedef __attribute__((address_space(1))) const vf4 glb_f4;
typedef __attribute__((address_space(3))) const vi4 lds_i4;
typedef __attribute__((address_space(1))) const vi4 glb_i4;
typedef unsigned int vu4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const vu4 glb_u4;
typedef __attribute__((address_space(1))) const MtsgHNode glb_hnode;

// ---------------------------------------------------------------------------
// Sobol sampler (samplers/sobol.cpp:147-258, sobolseq.h:43-130)
// ---------------------------------------------------------------------------
// sobol::sampleSingle (sobolseq.h:43-57): XOR of the direction-number columns
// selected by the bits of `index`, evaluated 4 bits at a time through
// precomputed XOR tables (exactly the same XOR, so the same result)
template <int NIB, typename T>
__device__ __forceinline__ uint32_t sobol_bits(T *tab, uint64_t index) {
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < NIB; ++c) r ^= tab[c * 16 + (uint32_t)((index >> (4 * c)) & 15u)];
    return r;
}

struct SobolCtx {
    lds_u32 *lds;             // [lds_dims][nibbles][16]
    glb_u32 *glob;            // [1024][MTSG_NIBBLES][16]
    uint32_t lds_dims, nibbles, scramble;
    bool indep;               // the `independent` sampler: `index` is a stream key
    bool replay;              // SFMT replay: draws come from the lane's SFMT stream
    bool tight;               // a constant of the kernel (lds_view: SCENE_LDS): the LDS tables are read
                              // through sobol_row, next2d's two dimensions together.  Taken by the
                              // small-scene kernels, which are VALU-bound and where it was measured
                              // (DESIGN.md 4, round 9); the large-scene kernels wait on memory and
                              // keep the draws as they were
    uint32_t *sfmt;           // the streams (lane u: sfmt + u * MTSG_SFMT_WORDS)
};

// the SFMT replay stream of this lane (MtsgLaunch::sfmt; unit = global lane index)
typedef __attribute__((address_space(1))) uint32_t glb_w32;
__device__ __forceinline__ glb_w32 *lane_sfmt(const SobolCtx &C) {
    return (glb_w32 *)C.sfmt + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * MTSG_SFMT_WORDS;
}

// The independent sampler (independent.cpp:82-104): a counter-based stream per
// (pixel, sample) -- splitmix64-finalised key, one finalised draw per dimension
// -- in place of the reference's per-thread SFMT19937, whose values depend on
// the thread schedule; Random::nextFloat's [1,2) - 1 conversion
// (random.cpp:630-639).  The oracle's indep_* functions are the same.
__device__ __forceinline__ uint64_t indep_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t indep_key(uint32_t px, uint32_t py, uint32_t frame) {
    return indep_mix64((((uint64_t)px << 48) | ((uint64_t)py << 32) | frame) ^ 0x6A09E667F3BCC909ull);
}
__device__ __forceinline__ float indep_float(uint64_t key, uint32_t dim) {
    const uint32_t u = (uint32_t)indep_mix64(key + (uint64_t)(dim + 1) * 0x9E3779B97F4A7C15ull);
    return __uint_as_float((u >> 9) | 0x3f800000u) - 1.0f;
}

// The LDS tables' addressing.  A table starts at a multiple of 64 bytes (the kernels
// declare `lds` 64-byte aligned; a dimension's table is nibbles * 64 bytes), so nibble c's
// byte offset within a row, (index >> (4c - 2)) & 0x3c, does not carry into the base: one
// shift and one v_and_or_b32 per nibble, the row (c * 16 words) in the read's offset field.
// Written as an integer sum: still the right address wherever the base is not so aligned.
template <int C>
__device__ __forceinline__ lds_u32 *sobol_row(lds_u32 *tab, uint64_t index) {
    const uint32_t w = C < 8 ? (uint32_t)index : (uint32_t)(index >> 32);
    const uint32_t o = (C & 7) == 0 ? (w << 2) & 0x3cu : (w >> (4 * (C & 7) - 2)) & 0x3cu;
    return (lds_u32 *)(uintptr_t)((uint32_t)(uintptr_t)tab + o);
}
// XOR of NIB table words (and `r`), folded three inputs at a time
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);   // the truth table of a ^ b ^ c
#else
    return a ^ b ^ c;
#endif
}
template <int NIB>
__device__ __forceinline__ uint32_t sobol_fold(uint32_t r, const uint32_t *w) {
#pragma unroll
    for (int c = 0; c + 1 < NIB; c += 2) r = xor3(r, w[c], w[c + 1]);
    if (NIB & 1) r ^= w[NIB - 1];
    return r;
}
#define MTSG_NIB_SEQ(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12)
static_assert(MTSG_NIBBLES == 13, "MTSG_NIB_SEQ lists the nibbles of the widest index");
// one dimension's bits ^ r, from its LDS table
template <int NIB>
__device__ __forceinline__ uint32_t sobol_bits_lds(lds_u32 *tab, uint64_t index, uint32_t r) {
    uint32_t w[NIB];
#define MTSG_NIB(c) if constexpr (c < NIB) w[c < NIB ? c : 0] = sobol_row<c>(tab, index)[c * 16];
    MTSG_NIB_SEQ(MTSG_NIB)
#undef MTSG_NIB
    return sobol_fold<NIB>(r, w);
}
// two successive dimensions of one index, both in LDS: their tables are NIB * 16
// words apart, so the row addresses are formed once and (NIB = 8: 128 words,
// within ds_read2_b32's second offset) each nibble's two words are one read
template <int NIB>
__device__ __forceinline__ void sobol_bits2_lds(lds_u32 *tab, uint64_t index, uint32_t r, uint32_t &b0, uint32_t &b1) {
    uint32_t w0[NIB], w1[NIB];
#define MTSG_NIB(c)                                              \
    if constexpr (c < NIB) {                                     \
        lds_u32 *p = sobol_row<c>(tab, index);                   \
        w0[c < NIB ? c : 0] = p[c * 16];                         \
        w1[c < NIB ? c : 0] = p[c * 16 + NIB * 16];              \
    }
    MTSG_NIB_SEQ(MTSG_NIB)
#undef MTSG_NIB
    b0 = sobol_fold<NIB>(r, w0);
    b1 = sobol_fold<NIB>(r, w1);
}
#undef MTSG_NIB_SEQ

__device__ __forceinline__ float sobol_finish(uint32_t result) {
    float v = (float)result * (1.0f / 4294967296.0f);
    return smin(v, D_ONE_MINUS_EPS);
}

__device__ __forceinline__ float sobol_sample(const SobolCtx &C, uint64_t index, uint32_t dim) {
    if (C.indep) return indep_float(index, dim);
    uint32_t result;
    if (dim < C.lds_dims) {
        lds_u32 *t = C.lds + dim * C.nibbles * 16;
        if (C.tight)
            result = (C.nibbles == 8) ? sobol_bits_lds<8>(t, index, C.scramble)
                                      : sobol_bits_lds<MTSG_NIBBLES>(t, index, C.scramble);
        else
            result = C.scramble ^ ((C.nibbles == 8) ? sobol_bits<8>(t, index) : sobol_bits<MTSG_NIBBLES>(t, index));
    } else {
        glb_u32 *t = C.glob + (size_t)dim * MTSG_NIBBLES * 16;
        result = C.scramble ^ ((C.nibbles == 8) ? sobol_bits<8>(t, index) : sobol_bits<MTSG_NIBBLES>(t, index));
    }
    return sobol_finish(result);
}

// dimensions dim and dim + 1 of one index (next2d).  Both in the LDS tables: one
// set of nibble offsets for the two (sobol_bits2_lds); any other case -- a pair
// that straddles lds_dims, global tables, the independent sampler -- is two
// sobol_sample draws.  The same words XORed in another order: the same bits.
__device__ __forceinline__ void sobol_sample2(const SobolCtx &C, uint64_t index, uint32_t dim, float &u, float &v) {
    if (C.tight && !C.indep && dim + 1 < C.lds_dims) {
        lds_u32 *t = C.lds + dim * C.nibbles * 16;
        uint32_t b0, b1;
        if (C.nibbles == 8) sobol_bits2_lds<8>(t, index, C.scramble, b0, b1);
        else sobol_bits2_lds<MTSG_NIBBLES>(t, index, C.scramble, b0, b1);
        u = sobol_finish(b0);
        v = sobol_finish(b1);
        return;
    }
    u = sobol_sample(C, index, dim);
    v = sobol_sample(C, index, dim + 1);
}

// sobol::look_up restated as the GF(2) solve it encodes (host precomputes inv/ycol)
__device__ __forceinline__ uint64_t sobol_lookup(const MtsgLookup &L, uint32_t frame, uint32_t px, uint32_t py,
                                                 uint64_t scramble) {
    const uint32_t m = L.m;
    uint32_t s = (uint32_t)((scramble & 0xFFFFFFFFull) >> (32 - m));
    uint32_t mask = (1u << m) - 1u;
    uint32_t sx = (px ^ s) & mask, sy = (py ^ s) & mask;
    uint32_t jlo = __builtin_bitreverse32(sx) >> (32 - m);
    uint64_t index = ((uint64_t)frame << (2 * m)) | jlo;
    uint32_t K = 0;
    uint64_t bits = index;
    while (bits) {
        uint32_t b = (uint32_t)__builtin_ctzll(bits);
        K ^= L.ycol[b];
        bits &= bits - 1;
    }
    uint32_t rhs = (sy ^ K) & mask, jhi = 0;
    for (uint32_t t = 0; t < m; ++t) jhi |= (uint32_t)(__builtin_popcount(L.inv[t] & rhs) & 1) << t;
    return index | ((uint64_t)jhi << m);
}

struct SamplerState {
    uint64_t sobolIndex;
    uint32_t sampleIndex;
    uint32_t dim;
    bool err;
};

__device__ __forceinline__ float next1d(const SobolCtx &C, SamplerState &s) {   // sobol.cpp:219-229
    if (C.replay) { s.dim++; return sfmt_next_float(lane_sfmt(C)); }   // independent.cpp:97-99
    if (s.dim >= MTSG_SOBOL_DIMS && !C.indep) { s.err = true; return 0.0f; }
    return sobol_sample(C, s.sobolIndex, s.dim++);
}
__device__ __forceinline__ void next2d(const SobolCtx &C, float resolution, SamplerState &s, int px, int py,
                                       float &u, float &v) {                       // sobol.cpp:231-250
    if (C.replay) {   // independent.cpp:101-105: value1, then value2
        u = sfmt_next_float(lane_sfmt(C));
        v = sfmt_next_float(lane_sfmt(C));
        s.dim += 2;
        return;
    }
    if (s.dim + 1 >= 5 && s.dim < 5) s.dim = 5;   // skip the (empty) array dimensions [5,5)
    if (s.dim + 1 >= MTSG_SOBOL_DIMS && !C.indep) { s.err = true; u = v = 0.0f; return; }
    if (!C.indep && s.dim == 0 && s.sobolIndex != (uint64_t)s.sampleIndex) {
        sobol_sample2(C, s.sobolIndex, s.dim, u, v);
        u = u * resolution - (float)px;
        v = v * resolution - (float)py;
    } else {
        sobol_sample2(C, s.sobolIndex, s.dim, u, v);
    }
    s.dim += 2;
}

// A sample's start: sample j of pixel (px, py) -> its index into the Sobol sequence
// (SobolSampler::generate + setSampleIndex, sobol.cpp:147-217: sobol::look_up, or j itself for
// a 1 x 1 resolution) or the independent sampler's stream key, the state at dimension 0 and
// the first next2d, the film offset (u, v).
// nibbles: L.nibbles, which the megakernel reads from its LDS view (SobolCtx::nibbles)
template <typename T>
__device__ __forceinline__ void sample_start(const SobolCtx &SC, const MtsgLaunch &L, T *ycolTab, uint32_t nibbles,
                                             int px, int py, uint32_t j, SamplerState &smp, float &u, float &v) {
    smp.dim = 0;
    smp.sampleIndex = j;
    smp.err = false;
    smp.sobolIndex = SC.indep ? indep_key((uint32_t)px, (uint32_t)py, j)
                   : (L.lut.m > 1) ? sobol_lookup_lds(L.lut, ycolTab, nibbles, j, (uint32_t)px, (uint32_t)py, L.scramble64)
                                   : (uint64_t)j;
    next2d(SC, L.resolution, smp, px, py, u, v);
}
