// replay_host.cpp -- the host part of the `independent` sampler replay
// (MTSGPU_SAMPLER_SFMT_*): SFMT19937 stream seeding as the reference's Random does it
// (random.cpp) and the order in which the reference renders a crop's pixels
// (imageproc.cpp, renderproc.cpp).  Plain host code; capi.cpp uploads what it forms.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "render_plan.h"
#include "sfmt.h"

// ---------------------------------------------------------------------------
// The `independent` sampler replay (MTSGPU_SAMPLER_SFMT_*): stream seeding and
// the reference's render order
// ---------------------------------------------------------------------------
static void sfmt_period_certification(uint32_t *w) {   // random.cpp:322-347
    const uint32_t parity[4] = {0x00000001u, 0x00000000u, 0x00000000u, 0x13c9e684u};
    uint32_t inner = 0;
    for (int i = 0; i < 4; ++i) inner ^= w[i] & parity[i];
    for (int i = 16; i > 0; i >>= 1) inner ^= inner >> i;
    if (inner & 1) return;
    for (int i = 0; i < 4; ++i)
        for (uint32_t work = 1, j = 0; j < 32; ++j, work <<= 1)
            if (work & parity[i]) { w[i] ^= work; return; }
}

void mtsg_sfmt_seed(uint32_t *w, uint64_t seed) {   // init_gen_rand (random.cpp:397-406)
    uint64_t v = seed;
    w[0] = (uint32_t)v;
    w[1] = (uint32_t)(v >> 32);
    for (int i = 1; i < MTSG_SFMT_N64; ++i) {
        v = 6364136223846793005ull * (v ^ (v >> 62)) + (uint64_t)i;
        w[2 * i] = (uint32_t)v;
        w[2 * i + 1] = (uint32_t)(v >> 32);
    }
    w[MTSG_SFMT_N32] = MTSG_SFMT_N32;
    sfmt_period_certification(w);
}

// Random(Random *parent): init_by_array over 312 of the parent's outputs as
// 624 little-endian words (random.cpp:408-471, 528-548)
void mtsg_sfmt_clone(uint32_t *w, uint32_t *parent) {
    uint32_t key[MTSG_SFMT_N32];
    for (int i = 0; i < MTSG_SFMT_N64; ++i) {
        const uint64_t v = sfmt_next_ulong(parent);
        key[2 * i] = (uint32_t)v;
        key[2 * i + 1] = (uint32_t)(v >> 32);
    }
    const int n = MTSG_SFMT_N32, lag = 11, mid = (n - lag) / 2, len = MTSG_SFMT_N32;
    auto f1 = [](uint32_t x) { return (x ^ (x >> 27)) * 1664525u; };
    auto f2 = [](uint32_t x) { return (x ^ (x >> 27)) * 1566083941u; };
    std::memset(w, 0x8b, MTSG_SFMT_N32 * 4);
    int count = std::max(len + 1, n);
    uint32_t r = f1(w[0] ^ w[mid] ^ w[n - 1]);
    w[mid] += r;
    r += (uint32_t)len;
    w[mid + lag] += r;
    w[0] = r;
    --count;
    int i = 1, j = 0;
    for (; j < count && j < len; ++j, i = (i + 1) % n) {
        r = f1(w[i] ^ w[(i + mid) % n] ^ w[(i + n - 1) % n]);
        w[(i + mid) % n] += r;
        r += key[j] + (uint32_t)i;
        w[(i + mid + lag) % n] += r;
        w[i] = r;
    }
    for (; j < count; ++j, i = (i + 1) % n) {
        r = f1(w[i] ^ w[(i + mid) % n] ^ w[(i + n - 1) % n]);
        w[(i + mid) % n] += r;
        r += (uint32_t)i;
        w[(i + mid + lag) % n] += r;
        w[i] = r;
    }
    for (j = 0; j < n; ++j, i = (i + 1) % n) {
        r = f2(w[i] + w[(i + mid) % n] + w[(i + n - 1) % n]);
        w[(i + mid) % n] ^= r;
        r -= (uint32_t)i;
        w[(i + mid + lag) % n] ^= r;
        w[i] = r;
    }
    w[MTSG_SFMT_N32] = MTSG_SFMT_N32;
    sfmt_period_certification(w);
}

namespace {
// HilbertCurve2D<uint8_t>::generate (core/sfcurve.h): ENorth 0, EEast 1, ESouth 2, EWest 3
void hilbert(int order, int front, int right, int back, int left, uint8_t pos[2], uint8_t w, uint8_t h, uint32_t bx,
             uint32_t by, std::vector<uint32_t> &out) {
    if (order == 0) {
        if (pos[0] < w && pos[1] < h) out.push_back((bx + pos[0]) | ((by + pos[1]) << 16));
        return;
    }
    auto move = [&](int d) {
        if (d == 0) pos[1]--; else if (d == 1) pos[0]++; else if (d == 2) pos[1]++; else pos[0]--;
    };
    hilbert(order - 1, left, back, right, front, pos, w, h, bx, by, out); move(right);
    hilbert(order - 1, front, right, back, left, pos, w, h, bx, by, out); move(back);
    hilbert(order - 1, front, right, back, left, pos, w, h, bx, by, out); move(left);
    hilbert(order - 1, right, front, left, back, pos, w, h, bx, by, out);
}
}  // namespace

// the crop's pixels (x | y << 16, crop-relative) in the reference's order:
// BlockedImageProcess's spiral (imageproc.cpp:28-80), HilbertCurve2D per block
// (renderproc.cpp:79-81); blockStart: first pixel of each block, then the count
void mtsg_render_order(uint32_t width, uint32_t height, uint32_t bs, std::vector<uint32_t> &order,
                       std::vector<uint32_t> &blockStart) {
    const int nbx = (int)std::ceil((float)width / (float)bs), nby = (int)std::ceil((float)height / (float)bs);
    const int total = nbx * nby;
    int cx = nbx / 2, cy = nby / 2, dir = 0 /* ERight */, stepsLeft = 1, numSteps = 1;
    const float invLog2 = 1.0f / (float)std::log((double)2.0f);   // math::fastlog (math.h:193-195)
    order.clear();
    blockStart.clear();
    for (int b = 0; b < total; ++b) {
        const int bw = std::min<int>((int)width - cx * (int)bs, (int)bs), bh = std::min<int>((int)height - cy * (int)bs, (int)bs);
        blockStart.push_back((uint32_t)order.size());
        const int order2 = (int)std::ceil(invLog2 * (float)std::log((double)(float)std::max(bw, bh)));
        uint8_t pos[2] = {0, 0};
        hilbert(order2, 0, 1, 2, 3, pos, (uint8_t)bw, (uint8_t)bh, (uint32_t)(cx * (int)bs), (uint32_t)(cy * (int)bs),
                order);
        if (b + 1 == total) break;
        do {
            if (dir == 0) ++cx; else if (dir == 1) ++cy; else if (dir == 2) --cx; else --cy;
            if (--stepsLeft == 0) {
                dir = (dir + 1) % 4;
                if (dir == 2 || dir == 0) ++numSteps;   // ELeft, ERight
                stepsLeft = numSteps;
            }
        } while (cx < 0 || cy < 0 || cx >= nbx || cy >= nby);
    }
    blockStart.push_back((uint32_t)order.size());
}

// IndependentSampler's Random() = seed(5489); RenderJob clones it per worker in
// order (renderjob.cpp:58-66).  Units: one worker over all blocks, or one per block
void mtsg_replay_tables(uint32_t width, uint32_t height, bool per_block, std::vector<uint32_t> &order,
                        std::vector<uint32_t> &unitStart, std::vector<uint32_t> &streams) {
    std::vector<uint32_t> blockStart;
    mtsg_render_order(width, height, MTSG_BLOCK_SIZE, order, blockStart);
    if (per_block) unitStart = blockStart;
    else unitStart = {0u, (uint32_t)order.size()};
    const uint32_t units = (uint32_t)unitStart.size() - 1;
    std::vector<uint32_t> master(MTSG_SFMT_WORDS, 0u);
    streams.assign((size_t)units * MTSG_SFMT_WORDS, 0u);
    mtsg_sfmt_seed(master.data(), 5489ull);
    for (uint32_t u = 0; u < units; ++u) mtsg_sfmt_clone(streams.data() + (size_t)u * MTSG_SFMT_WORDS, master.data());
}
