// sobol_host.cpp -- the Sobol sampler's host tables (samplers/sobol.cpp:147-258,
// sobolseq.h:43-130): the 1024 x 52 direction matrices regenerated from the Joe-Kuo
// parameters, the look_up GF(2) inverse for a film resolution, and sampleTEA (core/qmc.h).
#include <cstring>

#include "scene_build.h"
#include "sobol_params.inc"

// Built once by a function-local static's initialiser, which C++11 runs
// exactly once even when several group members upload concurrently.
static std::vector<uint32_t> build_sobol_matrices() {
    std::vector<uint32_t> M((size_t)MTSG_SOBOL_DIMS * MTSG_SOBOL_SIZE, 0u);
    for (int k = 0; k < MTSG_SOBOL_SIZE; ++k) M[k] = (uint32_t)(((uint64_t)1 << (MTSG_SOBOL_SIZE - 1 - k)) >> 20);
    const size_t n = sizeof(kJoeKuoParams) / sizeof(kJoeKuoParams[0]);
    size_t i = 0;
    uint64_t m[MTSG_SOBOL_SIZE];
    while (i < n) {
        const uint32_t d = kJoeKuoParams[i], s = kJoeKuoParams[i + 1], a = kJoeKuoParams[i + 2];
        for (uint32_t t = 0; t < s; ++t) m[t] = kJoeKuoParams[i + 3 + t];
        i += 3 + s;
        // Sobol' recurrence: m_k = 2a_1 m_{k-1} ^ ... ^ 2^{s-1} a_{s-1} m_{k-s+1} ^ 2^s m_{k-s} ^ m_{k-s}
        for (uint32_t k = s; k < MTSG_SOBOL_SIZE; ++k) {
            uint64_t val = m[k - s] ^ (m[k - s] << s);
            for (uint32_t t = 1; t < s; ++t)
                if ((a >> (s - 1 - t)) & 1) val ^= m[k - t] << t;
            m[k] = val;
        }
        for (int k = 0; k < MTSG_SOBOL_SIZE; ++k)
            M[(size_t)(d - 1) * MTSG_SOBOL_SIZE + k] = (uint32_t)((m[k] << (MTSG_SOBOL_SIZE - 1 - k)) >> 20);
    }
    return M;
}

const std::vector<uint32_t> &mtsg_sobol_matrices() {
    static const std::vector<uint32_t> M = build_sobol_matrices();
    return M;
}

void mtsg_sobol_lookup_table(uint32_t m, MtsgLookup &L) {
    std::memset(&L, 0, sizeof L);
    L.m = m;
    if (m <= 1 || m > 31) return;   // (the kernels enumerate a 2 x 2 film's samples without look_up)
    mtsg_sobol_lookup_solve(m, L);
}

// the GF(2) inverse for any 1 <= m <= 31 (mtsgpu_lookup_host checks m = 1 as well)
void mtsg_sobol_lookup_solve(uint32_t m, MtsgLookup &L) {
    std::memset(&L, 0, sizeof L);
    L.m = m;
    if (m < 1 || m > 31) return;
    const std::vector<uint32_t> &M = mtsg_sobol_matrices();
    for (int b = 0; b < 64; ++b) L.ycol[b] = b < MTSG_SOBOL_SIZE ? (M[MTSG_SOBOL_SIZE + b] >> (32 - m)) : 0u;
    uint32_t A[32], I[32];
    for (uint32_t r = 0; r < m; ++r) {
        A[r] = 0; I[r] = 1u << r;
        for (uint32_t t = 0; t < m; ++t) A[r] |= ((L.ycol[m + t] >> r) & 1u) << t;
    }
    for (uint32_t c = 0; c < m; ++c) {
        uint32_t piv = c;
        while (piv < m && !((A[piv] >> c) & 1u)) ++piv;
        if (piv == m) continue;   // cannot happen for a (0,2)-sequence
        std::swap(A[c], A[piv]); std::swap(I[c], I[piv]);
        for (uint32_t r = 0; r < m; ++r)
            if (r != c && ((A[r] >> c) & 1u)) { A[r] ^= A[c]; I[r] ^= I[c]; }
    }
    for (uint32_t t = 0; t < m; ++t) L.inv[t] = I[t];
}

uint64_t mtsg_sample_tea(uint32_t v0, uint32_t v1, int rounds) {   // core/qmc.h:146-156
    uint32_t sum = 0;
    for (int i = 0; i < rounds; ++i) {
        sum += 0x9e3779b9;
        v0 += ((v1 << 4) + 0xA341316C) ^ (v1 + sum) ^ ((v1 >> 5) + 0xC8013EA4);
        v1 += ((v0 << 4) + 0xAD90777D) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7E95761E);
    }
    return ((uint64_t)v1 << 32) + v0;
}
