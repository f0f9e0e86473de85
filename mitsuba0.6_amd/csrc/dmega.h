// dmega.h -- the persistent megakernel of Mitsuba 0.6's `path` integrator
// (MIPathTracer::Li, src/integrators/path/path.cpp:119-294, inside
// SamplingIntegrator::renderBlock, src/librender/integrator.cpp:140-188),
// instantiated per scene feature set in path_f.hip:
//
//  * lane g of the persistent grid owns sample runs g, g + lanes, g + 2 lanes, ...
//    (static striding: no global queue, no tail of long per-pixel tasks), a run being
//    2^round_shift consecutive samples of one pixel, one after the other;
//  * a lane whose path ends starts its next item immediately (regeneration);
//  * tiny scenes that are scanned (SCENE_LDS kernels, L.scan, not the SFMT replay)
//    start paths a wave at a time instead: the wave's 64 lanes run one step of their
//    item streams together, the real samples' start records go to a per-wave batch in
//    LDS, and a lane whose path ends pops the next record, whichever lane produced it
//    (mtsg_start_queue, DESIGN.md 4 "Start queue"); these kernels store every splat
//    record as it is formed (no held pair);
//  * in kernels without an environment emitter a production pass retires the samples
//    whose camera ray fails section B's own ray_interval test (the scene bounds and the
//    clip planes): such a path is black at depth 1 with one ray, so the pass writes its
//    records and counts it, and only the other samples enter the batch (MTSG_EARLY_MISS,
//    DESIGN.md 4 "Early miss");
//  * each loop iteration traces the lane's pending shadow ray and its
//    closest-hit ray, then shades (PathShader, dpath.h);
//  * LDS holds the Sobol and look_up tables and the lane-strided traversal stacks
//    (and the whole scene, with its triangles' unit face normals, for small ones).
#pragma once
#include "dpath.h"
#include "launchers.h"

// tiny-scene kernels built without the start queue (-DMTSG_START_QUEUE=0) keep a pair's
// first splat record in registers (PathShader::finish)
#ifndef MTSG_HOLD_PAIR
#define MTSG_HOLD_PAIR 1
#endif

// The tiny set: path_kernel<*, true, MTSG_FEAT_DIFF, 4> -- the kernel of the all-diffuse LDS scenes,
// bench.py's C1 / C2 -- is built for the Sobol sampler with indices below 2^32 only: no
// `independent` draw, no SFMT replay and its start loop, no 13-nibble draw.  Those are
// launch-uniform choices, but register allocation, SGPR spilling and code size belong to the whole
// function, so the hot loop paid for them (DESIGN.md 4 "Tiny set").  render_plan.cpp plan_render
// sends every other launch of such a scene to the generic kernel (mtsg_tiny_set, layout.h).
// L.scan and the loop without the queue stay run-time choices: MTSGPU_NO_SCAN launches keep
// this kernel.  -DMTSG_TINY_SET=0 (A/B builds): the kernel with every choice at run time
#ifndef MTSG_TINY_SET
#define MTSG_TINY_SET 1
#endif

// diagnostic build (-DMTSG_MK_STAMPS): wave cycles per megakernel section,
// summed into counters 11-14 (start, shadow trace, closest trace, shade) by
// lane 0 of each wave.  s_memtime without draining the memory counters: a
// section's loads are consumed inside it (traversal, shading), so the split is
// close; read shares, not times (tools/mk_stamps.py)
#ifdef MTSG_MK_STAMPS
#define MK_STAMP(acc, t0)                                                        \
    do {                                                                         \
        unsigned long long t1_;                                                  \
        __builtin_amdgcn_sched_barrier(0);                                       \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1_)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                       \
        acc += t1_ - t0;                                                         \
        t0 = t1_;                                                                \
    } while (0)
#else
#define MK_STAMP(acc, t0) (void)0
#endif


// a lane's rank among the lanes of `mask` below it
__device__ __forceinline__ uint32_t wave_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// a start record into its slot of the wave's batch (word w of slot s at [w * 64 + s])
__device__ __forceinline__ void queue_store(lds_w32 *w, const StartRec &r) {
    w[0 * 64] = (uint32_t)r.sobolIndex;
    w[1 * 64] = (uint32_t)(r.sobolIndex >> 32);
    w[2 * 64] = __float_as_uint(r.sx);
    w[3 * 64] = __float_as_uint(r.sy);
    w[4 * 64] = __float_as_uint(r.rd.x);
    w[5 * 64] = __float_as_uint(r.rd.y);
    w[6 * 64] = __float_as_uint(r.rd.z);
    w[7 * 64] = __float_as_uint(r.invZ);
    w[8 * 64] = r.pix;
    w[9 * 64] = r.jj;
}

// The persistent megakernel: grid = CUs x resident blocks; every lane runs
// PathShader steps with both traversals inline
template <bool INSTR, bool SCENE_LDS, int FEAT, int WAVES>
__global__ __launch_bounds__(BLOCK, WAVES) void path_kernel(MtsgLaunch L) {   // L: the first argument (launch_fresh)
    constexpr bool STATS = INSTR;
    constexpr bool ANA = (FEAT & MTSG_FEAT_ANA) != 0;
    constexpr bool HNODES = (FEAT & (MTSG_FEAT_GGX | MTSG_FEAT_NORD | MTSG_FEAT_NORC)) != 0;
    extern __shared__ __attribute__((aligned(64))) uint32_t lds[];   // (dsampler.h sobol_row)
    (void)stage_lds<SCENE_LDS>(L, lds);
    PathCounters c = {};   // INSTR statistics only: the always-on counts are wave-uniform (wc)
    WaveCounters wc = {};

    // static striding: lane g takes sample runs g + k * lanes, k = 0, 1, ... (`round` is
    // the carried run state of layout.h mtsg_run_step, or the SFMT replay's position in
    // its unit: 32 bits, not a 64-bit item index, live across the bounce loop)
    // Kernels with the start queue: `round` and prodPix are the lane's PRODUCER state (its
    // item stream, unchanged); st.pix belongs to whatever path the lane renders
    // (not the MTSG_FEAT_LENS kernels: their start record is three origin words and an
    // interval longer, and the aperture draw would run beside every lane's live path state;
    // mtsg_path_start_queue says the same of their launches.  They start as the kernels
    // without the queue do, holding a pair's first splat record)
    constexpr bool TINY = MTSG_TINY_SET && SCENE_LDS && (FEAT & MTSG_FEAT_DIFF) != 0 && WAVES == 4;
    constexpr bool QUEUE = SCENE_LDS && MTSG_START_QUEUE && (FEAT & MTSG_FEAT_LENS) == 0;
    // a production pass retires the samples whose camera ray misses the scene: without an
    // environment emitter their record is known once the ray exists
    constexpr bool EARLY = QUEUE && MTSG_EARLY_MISS && (FEAT & MTSG_FEAT_ENV) == 0;
    const uint32_t g = xcd_block(L.xcds) * BLOCK + threadIdx.x;
    uint32_t round = 0;
    bool done = false;
    float4 held = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // PathShader::finish's held splat record
    PathState st;
    st.active = false;
    st.pix = 0;
    if (TINY || !L.replay) mtsg_run_init(L, g, round, st.pix);   // the lane's one division
    uint32_t prodPix = st.pix;
    uint32_t qHead = 0, qCount = 0, qPasses = 0;   // wave-uniform: the batch's unread entries, production passes
    uint32_t qRetired = 0;                         // wave-uniform: samples the passes finished themselves
    st.smp.sobolIndex = 0; st.smp.sampleIndex = 0; st.smp.dim = 0; st.smp.err = false;
    st.sx = st.sy = 0;
    st.haveRay = st.primary = st.haveShadow = false;
    st.P.its.p = mk(0, 0, 0); st.rd = mk(0, 0, 1); st.sd = mk(0, 0, 1);
    st.rmint = st.rmaxt = st.smaxt = 0;
#ifdef MTSG_MK_STAMPS
    unsigned long long mkT[4] = {0, 0, 0, 0}, mkT0;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(mkT0)::"memory");
#endif

    while (true) {
        // the launch record re-read per bounce instead of held (dstage.h launch_fresh),
        // and the LDS / scene pointers re-derived from it (dstage.h lds_view): C2 +2.0%,
        // C4 +3.8%, C5 +0.7%, C3 0 (profiles/r04_ab_fresh_view.log)
        const MtsgLaunch &L = launch_fresh();
        const MtsgDeviceScene &S = L.scene;
        LdsView<SCENE_LDS> V = lds_view<SCENE_LDS>(L, lds);
        if constexpr (TINY) {   // what mtsg_tiny_set(L) says of every launch of this kernel, as constants
            V.SC.indep = false;
            V.SC.replay = false;
            V.SC.nibbles = 8;
        }
        lds_node *ldsNodes = V.nodes;
        lds_tri *ldsTris = V.tris;
        lds_stk_n *stkN = (lds_stk_n *)(lds + V.stackBase) + threadIdx.x;
        lds_stk_d *stkD = (lds_stk_d *)(lds + V.stackBase + L.stack_depth * BLOCK) + threadIdx.x;
        const PathShader<INSTR, SCENE_LDS, FEAT> sh{L, V.hs, V.SC, V.ycolTab, c};
        // ---- A: start the next sample
        if (QUEUE && mtsg_start_queue(L)) {
            // From the wave's start queue.  The wave's items are those its 64 lanes own
            // (lane i's k-th mtsg_run_step is item (i, k)); a sample's result depends on
            // (pixel, sample) alone and goes to that sample's own record slots, so which
            // lane renders which item changes nothing.  A production pass runs step k of
            // every lane that has items left, all lanes at once, and compacts the real
            // samples' start records (no padding pixel, no missing sample of an odd run)
            // into the batch; the lanes whose path has ended pop the next entries, by their
            // rank among themselves.  An empty batch is refilled while lanes still need an
            // entry and a lane still has items.
            lds_w32 *q = (lds_w32 *)(lds + V.stackBase) + (threadIdx.x >> 6) * (MTSG_QUEUE_REC_WORDS * 64);
            bool want = !st.active;
            while (true) {
                const uint64_t need = __ballot(want);
                if (need == 0) break;
                if (qCount == 0) {
                    if (__all(done)) break;
                    uint32_t jj = 0;
                    int px = 0, py = 0;
                    bool real = false;
                    if (!done) {
                        if (!mtsg_run_step(L, round, prodPix, jj)) done = true;
                        else real = jj < L.chunk_spp && pixel_of(L, prodPix, px, py);
                    }
                    uint64_t made;   // the lanes whose sample enters the batch
                    if constexpr (!EARLY) {
                    made = __ballot(real);
                    if (real) {
                        StartRec r;
                        // A pass runs beside every lane's live path state.  Indices beyond 32
                        // bits draw the film position one dimension at a time (the same words
                        // XORed, the same bits): the paired draw's 26 words in flight made the
                        // bench kernel spill (4 VGPRs; 124 and none with this)
                        SobolCtx SCq = V.SC;
                        SCq.tight = V.SC.nibbles == 8;
                        const PathShader<INSTR, SCENE_LDS, FEAT> shq{L, V.hs, SCq, V.ycolTab, c};
                        shq.produce(r, jj, prodPix, px, py);
                        queue_store(q + wave_rank(made), r);   // slot < 64, words 0..9: within MTSG_QUEUE_WORDS
                    }
                    } else {
                    // The same pass, which also retires.  The record stays inside the branch
                    // of the real lanes and its two ends are an if / else there (kept with r
                    // live across the wave's ballot and the retirement after the stores, the
                    // bench kernel spilled 9 VGPRs; 125 and none like this).  `keep` is false
                    // in the lanes that skip the branch, so a ballot inside it and the one
                    // after it see the same lanes.  A wave cannot retire 2^31 samples in one
                    // launch (their records alone would be 32 GiB), so wc needs no flush here
                    bool keep = real;
                    if (real) {
                        StartRec r;
                        SobolCtx SCq = V.SC;
                        SCq.tight = V.SC.nibbles == 8;
                        const PathShader<INSTR, SCENE_LDS, FEAT> shq{L, V.hs, SCq, V.ycolTab, c};
                        shq.produce(r, jj, prodPix, px, py);
                        // section B's own test of this camera ray (the operands load() forms,
                        // the same function): false here is okC false there, a path that
                        // shade() ends black at depth 1 -- its records are written now and it
                        // never takes a lane
                        float mn, mx;
                        keep = ray_interval(S, shq.cam_origin(), r.rd, S.cam.near_clip * r.invZ,
                                            S.cam.far_clip * r.invZ, false, mn, mx);
                        if (keep) queue_store(q + wave_rank(__ballot(keep)), r);
                        else shq.retire(r, px, py);
                    }
                    // a retired sample: its one ray, no path length beyond its own 1
                    const uint32_t nr = wave_count(real && !keep);
                    wc.rays += nr;
                    wc.samples += nr;
                    qRetired += nr;
                    made = __ballot(keep);
                    }
                    // the batch is written before any lane of the wave pops it
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    qHead = 0;
                    qCount = (uint32_t)__popcll(made);
                    ++qPasses;
                    // every item of the pass was padding or retired: the next pass (a wave that
                    // never queues a record leaves by __all(done) and the test after the loop)
                    if (qCount == 0) continue;
                }
                const uint32_t rank = wave_rank(need);
                if (want && rank < qCount) {   // entry qHead + rank < qHead + qCount <= 64
                    lds_w32 *e = q + qHead + rank;
                    StartRec r;
                    r.sobolIndex = (uint64_t)e[0 * 64] | ((uint64_t)e[1 * 64] << 32);
                    r.sx = __uint_as_float(e[2 * 64]);
                    r.sy = __uint_as_float(e[3 * 64]);
                    r.rd = mk(__uint_as_float(e[4 * 64]), __uint_as_float(e[5 * 64]), __uint_as_float(e[6 * 64]));
                    r.invZ = __uint_as_float(e[7 * 64]);
                    r.pix = e[8 * 64];
                    r.jj = e[9 * 64];
                    r.dim = 2;   // produce() drew the film position (not the replay: dimensions 0, 1)
                    sh.load(st, r);
                    want = false;
                }
                const uint32_t n = min((uint32_t)__popcll(need), qCount);
                qHead += n;
                qCount -= n;
            }
            // no lane got a path: the items are exhausted and the batch is empty
            if (!__any(st.active)) break;
        } else {
        while (!st.active && !done) {
            if (!TINY && L.replay) {   // SFMT replay: this lane's unit, pixel after pixel, in order
                const uint32_t unit = blockIdx.x * BLOCK + threadIdx.x;
                if (unit >= L.units) { done = true; break; }
                const uint32_t k0 = L.unit_start[unit], n = L.unit_start[unit + 1] - k0;
                if ((uint64_t)round >= (uint64_t)n * L.chunk_spp) { done = true; break; }
                const uint32_t k = k0 + round / L.chunk_spp, jj = round % L.chunk_spp;
                ++round;
                sh.start_xy(st, L.order[k], jj);
                break;
            }
            // sample runs: the lane's rounds r * 2^s .. r * 2^s + 2^s - 1 render samples
            // k * 2^s .. of one pixel back to back (run q = g + r * lanes; s = L.round_shift):
            // a box-filter record sector (film_slot: samples 2k, 2k + 1) has both halves
            // stored one path apart, while the line is still in this XCD's L2, and the
            // wave's primary rays revisit the same pixels.  (q / num_pixels, q % num_pixels)
            // is carried from run to run in `round` and st.pix (layout.h mtsg_run_step):
            // no division here
            uint32_t jj;
            if (!mtsg_run_step(L, round, st.pix, jj)) { done = true; break; }
            if (jj < L.chunk_spp) sh.start_jp(st, jj, st.pix);
        }
        if (__all(done)) break;
        }
        MK_STAMP(mkT[0], mkT0);

        // ---- B: trace the shadow ray, then the closest-hit ray ---------------
        bool occluded = false;
        bool hit = false;
        uint32_t slot = 0, prim = 0;
        float hu = 0, hv = 0, ht = 0;
        if (SCENE_LDS && L.scan) {
            // tiny scene: both rays of the bounce in one pass (scan_pair); both
            // leave the same point, P.its.p
            float minS = INFINITY, maxS = -INFINITY, minC = INFINITY, maxC = -INFINITY;
            bool okS = false, okC = false;
            f3 rcpS = mk(0, 0, 0), rcpC = mk(0, 0, 0);   // the clips' 1 / d, which scan_pair divides by
            wc.shadow += wave_count(st.active && st.haveShadow);
            wc.rays += wave_count(st.active && st.haveRay);
            if (st.active && st.haveShadow) {
                if (!is_zero(st.P.neeC)) okS = ray_interval(S, st.P.its.p, st.sd, D_EPSILON, st.smaxt, true, minS, maxS, rcpS);
                if (!okS) { minS = INFINITY; maxS = -INFINITY; }
            }
            if (st.active && st.haveRay) {
                okC = ray_interval(S, st.P.its.p, st.rd, st.rmint, st.rmaxt, false, minC, maxC, rcpC);
                if (!okC) { minC = INFINITY; maxC = -INFINITY; }
            }
            if (__any(okS || okC))
                scan_pair<STATS>(L, st.P.its.p, st.sd, st.rd, rcpS, rcpC, minS, maxS, minC, maxC, occluded, hit,
                                 prim, hu, hv, ht, c.tests);
            hit = hit && okC;
            occluded = occluded && okS;
        } else {
        // (round 4 measured both rays of a bounce through one per-lane loop, traverse_seq:
        // bit-identical, but C3 -5.5%, C4 -10%, C5 -1.7%, profiles/r04_ab_seq_traversal.log; removed)
        wc.shadow += wave_count(st.active && st.haveShadow);
        if (st.active && st.haveShadow) {
            float mint, maxt;
            // a shadow ray whose estimate is zero cannot change Li: skip its traversal
            if (!is_zero(st.P.neeC) && ray_interval(S, st.P.its.p, st.sd, D_EPSILON, st.smaxt, true, mint, maxt)) {
                uint32_t sl; float a0, a1, a2;
                if (SCENE_LDS)
                    occluded = traverse<true, STATS, ANA>(ldsNodes, ldsTris, st.P.its.p, st.sd, mint, maxt, stkN,
                                                                stkD, sl, a0, a1, a2, c.nodes, c.tests, S.analytic);
                else if constexpr (HNODES)
                    occluded = traverse<true, STATS, ANA>((glb_hnode *)S.hnodes, (glb_tri *)S.tris, st.P.its.p,
                                                                st.sd, mint, maxt, stkN, stkD, sl, a0, a1, a2, c.nodes,
                                                                c.tests, S.analytic);
                else
                    occluded = traverse<true, STATS, ANA>((glb_node *)S.nodes, (glb_tri *)S.tris, st.P.its.p,
                                                                st.sd, mint, maxt, stkN, stkD, sl, a0, a1, a2, c.nodes,
                                                                c.tests, S.analytic);
            }
        }
        // the NEE estimate is added now (as shade() would first thing), so it
        // is not live across the closest-hit traversal
        if (st.active && st.haveShadow) {
            if (!occluded) st.P.L = add(st.P.L, st.P.neeC);
            st.haveShadow = false;
        }
        MK_STAMP(mkT[1], mkT0);
        wc.rays += wave_count(st.active && st.haveRay);
        if (st.active && st.haveRay) {
            float mint, maxt;
            if (ray_interval(S, st.P.its.p, st.rd, st.rmint, st.rmaxt, false, mint, maxt)) {
                if (SCENE_LDS)
                    hit = traverse<false, STATS, ANA>(ldsNodes, ldsTris, st.P.its.p, st.rd, mint, maxt, stkN, stkD,
                                                            slot, hu, hv, ht, c.nodes, c.tests, S.analytic);
                else if constexpr (HNODES)
                    hit = traverse<false, STATS, ANA>((glb_hnode *)S.hnodes, (glb_tri *)S.tris, st.P.its.p, st.rd,
                                                            mint, maxt, stkN, stkD, slot, hu, hv, ht, c.nodes, c.tests,
                                                            S.analytic);
                else
                    hit = traverse<false, STATS, ANA>((glb_node *)S.nodes, (glb_tri *)S.tris, st.P.its.p, st.rd,
                                                            mint, maxt, stkN, stkD, slot, hu, hv, ht, c.nodes, c.tests,
                                                            S.analytic);
            }
            if (hit) prim = SCENE_LDS ? ldsTris[slot].prim : S.tris[slot].prim;
        }
        }
        if (st.active && st.haveShadow) {   // scan_pair case
            if (!occluded) st.P.L = add(st.P.L, st.P.neeC);
            st.haveShadow = false;
        }

        MK_STAMP(mkT[2], mkT0);

        // ---- C: shade -------------------------------------------------------
        // wave-uniform counts: a path's length is 1 + the bounces that advanced its
        // depth (shade() advances it at most once), summed over finished samples
        const bool was = st.active;
        const int d0 = st.P.depth;
        bool ended = false;
        if (st.active && sh.shade(st, occluded, hit, slot, prim, hu, hv, ht)) {
            ended = true;
            // (the held pair needs one lane to render a run's two samples back to back: not
            // with the start queue, whose kernels store every record as it is formed)
            sh.template finish<false>(st, MTSG_HOLD_PAIR && SCENE_LDS && !QUEUE ? &held : nullptr);
        }
        wc.len += wave_count(was && st.P.depth != d0);
        wc.samples += wave_count(ended);
        wc.err += wave_count(ended && st.smp.err);
        if (__builtin_expect((wc.len | wc.rays | wc.shadow) >= 0x80000000u, 0)) {   // uniform: flush before a wrap
            wc.len += wc.samples;
            wave_counters_flush(L, wc);
            wc = WaveCounters{};
        }
        MK_STAMP(mkT[3], mkT0);
    }
    wc.len += wc.samples;
    wave_counters_flush(L, wc);
    path_counters_flush<STATS>(L, c);
#ifndef MTSG_MK_STAMPS
    // debug counter 11: the start queue's production passes (tests: a render took the queue)
    if (QUEUE && qPasses && lane_id() == 0) atomicAdd(L.counters + 11, (unsigned long long)qPasses);
    // debug counter 12: the samples retired in production passes
    if (EARLY && qRetired && lane_id() == 0) atomicAdd(L.counters + 12, (unsigned long long)qRetired);
#endif
#ifdef MTSG_MK_STAMPS
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0)
        for (int k = 0; k < 4; ++k) atomicAdd(L.counters + 11 + k, mkT[k]);
#endif
}


// one megakernel variant, instrumented or not: the one place that names path_kernel<...>
// (launch and occupancy query both take the pointer: path_f.hip, path_kernel.hip path_pick)
template <bool SCENE_LDS, int FEAT, int WAVES>
static PathKernelFn path_kernel_w(bool instr) {
    if (instr) return path_kernel<true, SCENE_LDS, FEAT, WAVES>;
    return path_kernel<false, SCENE_LDS, FEAT, WAVES>;
}
