// host_math.h -- the reference's vector, 4x4 transform and half-float arithmetic as the host
// configure units use it (scene_build_impl.h).  Everything is inline and float: the units
// are built with -ffp-contract=off, and every function keeps the reference's operation order.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mtsg_host {

inline float fmax_std(float a, float b) { return (a < b) ? b : a; }   // std::max
inline float fmin_std(float a, float b) { return (b < a) ? b : a; }   // std::min

struct V { float x, y, z; };
inline V v(float x, float y, float z) { V r = {x, y, z}; return r; }
inline V operator+(V a, V b) { return v(a.x + b.x, a.y + b.y, a.z + b.z); }
inline V operator-(V a, V b) { return v(a.x - b.x, a.y - b.y, a.z - b.z); }
inline V operator*(V a, float f) { return v(a.x * f, a.y * f, a.z * f); }
inline V vdiv(V a, float f) { float r = 1.0f / f; return a * r; }
inline float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V cross(V a, V b) { return v((a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)); }
inline float length(V a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
inline V normalize(V a) { return vdiv(a, length(a)); }
inline float at(V a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
inline float avg3(float a) { float r = 0.0f; r += a; r += a; r += a; return r * (1.0f / 3); }   // Spectrum::average
inline float luminance(const float s[3]) { return s[0] * 0.212671f + s[1] * 0.715160f + s[2] * 0.072169f; }   // spectrum.h:725

const float kPi = 3.14159265358979323846f;

// ---- 4x4 transforms (core/matrix.h:744-756, matrix.inl:138-193, transform.cpp) ----
struct M4 { float m[4][4]; };
inline M4 mul(const M4 &a, const M4 &b) {
    M4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float sum = 0;
            for (int k = 0; k < 4; ++k) sum += a.m[i][k] * b.m[k][j];
            r.m[i][j] = sum;
        }
    return r;
}
inline bool invert(const M4 &src, M4 &t) {
    int indxc[4], indxr[4], ipiv[4] = {0, 0, 0, 0};
    t = src;
    for (int i = 0; i < 4; i++) {
        int irow = -1, icol = -1;
        float big = 0;
        for (int j = 0; j < 4; j++)
            if (ipiv[j] != 1)
                for (int k = 0; k < 4; k++) {
                    if (ipiv[k] == 0) {
                        if (std::fabs(t.m[j][k]) >= big) { big = std::fabs(t.m[j][k]); irow = j; icol = k; }
                    } else if (ipiv[k] > 1) {
                        return false;
                    }
                }
        ++ipiv[icol];
        if (irow != icol)
            for (int k = 0; k < 4; ++k) std::swap(t.m[irow][k], t.m[icol][k]);
        indxr[i] = irow; indxc[i] = icol;
        if (t.m[icol][icol] == 0) return false;
        float pivinv = 1.f / t.m[icol][icol];
        t.m[icol][icol] = 1.f;
        for (int j = 0; j < 4; j++) t.m[icol][j] *= pivinv;
        for (int j = 0; j < 4; j++)
            if (j != icol) {
                float save = t.m[j][icol];
                t.m[j][icol] = 0;
                for (int k = 0; k < 4; k++) t.m[j][k] -= t.m[icol][k] * save;
            }
    }
    for (int j = 3; j >= 0; j--)
        if (indxr[j] != indxc[j])
            for (int k = 0; k < 4; k++) std::swap(t.m[k][indxr[j]], t.m[k][indxc[j]]);
    return true;
}
struct Xf { M4 t, inv; };
inline M4 diag(float a, float b, float c, float d) {
    M4 r; std::memset(&r, 0, sizeof r);
    r.m[0][0] = a; r.m[1][1] = b; r.m[2][2] = c; r.m[3][3] = d;
    return r;
}
inline Xf compose(const Xf &a, const Xf &b) { return Xf{mul(a.t, b.t), mul(b.inv, a.inv)}; }
inline Xf scale(float x, float y, float z) { return Xf{diag(x, y, z, 1), diag(1.0f / x, 1.0f / y, 1.0f / z, 1)}; }
inline Xf translate(float x, float y, float z) {
    Xf r{diag(1, 1, 1, 1), diag(1, 1, 1, 1)};
    r.t.m[0][3] = x; r.t.m[1][3] = y; r.t.m[2][3] = z;
    r.inv.m[0][3] = -x; r.inv.m[1][3] = -y; r.inv.m[2][3] = -z;
    return r;
}
inline float deg2rad(float x) { return x * (kPi / 180.0f); }
inline float rad2deg(float x) { return x * (180.0f / kPi); }
inline V xf_point(const M4 &m, V p) {
    float x = m.m[0][0] * p.x + m.m[0][1] * p.y + m.m[0][2] * p.z + m.m[0][3];
    float y = m.m[1][0] * p.x + m.m[1][1] * p.y + m.m[1][2] * p.z + m.m[1][3];
    float z = m.m[2][0] * p.x + m.m[2][1] * p.y + m.m[2][2] * p.z + m.m[2][3];
    float w = m.m[3][0] * p.x + m.m[3][1] * p.y + m.m[3][2] * p.z + m.m[3][3];
    if (w == 1.0f) return v(x, y, z);
    return vdiv(v(x, y, z), w);
}
inline V xf_vec(const M4 &m, V a) {          // Transform::operator()(const Vector &) (transform.h:175-183)
    return v(m.m[0][0] * a.x + m.m[0][1] * a.y + m.m[0][2] * a.z, m.m[1][0] * a.x + m.m[1][1] * a.y + m.m[1][2] * a.z,
             m.m[2][0] * a.x + m.m[2][1] * a.y + m.m[2][2] * a.z);
}
inline V xf_normal(const M4 &inv, V a) {     // Transform::operator()(const Normal &) (transform.h:203-211)
    return v(inv.m[0][0] * a.x + inv.m[1][0] * a.y + inv.m[2][0] * a.z,
             inv.m[0][1] * a.x + inv.m[1][1] * a.y + inv.m[2][1] * a.z,
             inv.m[0][2] * a.x + inv.m[1][2] * a.y + inv.m[2][2] * a.z);
}
inline void put3(float *d, V a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }
inline void put16(float *d, const M4 &m) { std::memcpy(d, &m.m[0][0], 16 * sizeof(float)); }

// a row-major 'toWorld' of a desc as the reference's Transform (matrix + carried inverse,
// transform.h:54-60): the desc's inverse where it has one (any non-zero entry), else
// Matrix4x4::invert's; false for a singular matrix
inline bool desc_transform(const float *t16, const float *inv16, Xf &out) {
    std::memcpy(&out.t.m[0][0], t16, 16 * sizeof(float));
    bool haveInv = false;
    for (int i = 0; i < 16; ++i) haveInv |= inv16[i] != 0.0f;
    if (!haveInv) return invert(out.t, out.inv);
    std::memcpy(&out.inv.m[0][0], inv16, 16 * sizeof(float));
    return true;
}

// Transform::hasScale (transform.h:76-90) of a row-major matrix
inline bool has_scale(const float *m16) {
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            float sum = 0;
            for (int k = 0; k < 3; ++k) sum += m16[4 * i + k] * m16[4 * j + k];
            if (i == j ? std::fabs(sum - 1) > 1e-3f : std::fabs(sum) > 1e-3f) return true;
        }
    return false;
}

// unitAngle (core/util.h:309-314)
inline float unit_angle(V a, V b) {
    if (dot(a, b) < 0) return kPi - 2 * std::asin(0.5f * length(b + a));
    return 2 * std::asin(0.5f * length(b - a));
}

// coordinateSystem (util.cpp:592-601)
inline void coordinate_system(V a, V &b, V &c) {
    if (std::fabs(a.x) > std::fabs(a.y)) {
        float invLen = 1.0f / std::sqrt(a.x * a.x + a.z * a.z);
        c = v(a.z * invLen, 0.0f, -a.x * invLen);
    } else {
        float invLen = 1.0f / std::sqrt(a.y * a.y + a.z * a.z);
        c = v(0.0f, a.z * invLen, -a.y * invLen);
    }
    b = cross(c, a);
}

// half::half(float) (core/half.h:434-488, libcore/half.cpp:78-200): round to
// nearest even, overflow to infinity, NaN payload kept
inline uint16_t float_to_half(float f) {
    uint32_t i;
    std::memcpy(&i, &f, 4);
    const uint32_t s = (i >> 16) & 0x8000u;
    int e = (int)((i >> 23) & 0xff) - (127 - 15);
    uint32_t m = i & 0x7fffffu;
    if (e <= 0) {
        if (e < -10) return (uint16_t)s;
        m |= 0x800000u;
        const int t = 14 - e;
        const uint32_t a = (1u << (t - 1)) - 1u, b = (m >> t) & 1u;
        m = (m + a + b) >> t;
        return (uint16_t)(s | m);
    }
    if (e == 0xff - (127 - 15)) {
        if (m == 0) return (uint16_t)(s | 0x7c00u);
        m >>= 13;
        return (uint16_t)(s | 0x7c00u | m | (m == 0));
    }
    m = m + 0xfffu + ((m >> 13) & 1u);
    if (m & 0x800000u) { m = 0; e += 1; }
    if (e > 30) return (uint16_t)(s | 0x7c00u);
    return (uint16_t)(s | ((uint32_t)e << 10) | (m >> 13));
}
inline float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu, bits;
    if (e == 0) {
        if (m == 0) bits = s;
        else {
            e = 127 - 15 + 1;
            while (!(m & 0x400u)) { m <<= 1; --e; }
            bits = s | (e << 23) | ((m & 0x3ffu) << 13);
        }
    } else if (e == 31) {
        bits = s | 0x7f800000u | (m << 13);
    } else {
        bits = s | ((e + 127 - 15) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

}  // namespace mtsg_host
