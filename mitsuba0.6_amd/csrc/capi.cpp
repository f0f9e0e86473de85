// capi.cpp -- the C-ABI of libmtsgpu.so (include/mtsgpu.h).
//
// Replaces, for the `path` integrator, SamplingIntegrator::render ->
// BlockedRenderProcess -> BlockRenderer::process -> renderBlock
// (src/librender/integrator.cpp:95-188, renderproc.cpp:68-149): one call
// renders a pixel window with a persistent kernel and returns the ImageBlock
// (full crop + filter border) that Film::put would have accumulated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mtsgpu.h"
#include "layout.h"
#include "scene_build.h"
#include "sfmt.h"
#include "kdtree.h"
#include "launchers.h"
#include "render_plan.h"

namespace {

thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, std::max<size_t>(n, 16));
        if (e == hipSuccess) bytes = std::max<size_t>(n, 16);
        return e;
    }
};

}  // namespace

struct mtsgpu_ctx {
    int device = 0;
    int num_cus = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    bool have_scene = false;
    HostScene host;
    MtsgDeviceScene dscene;
    DevBuf scan_tris;   // k-grouped TriAccel records of scan-sized scenes (their counts: host.launch.scan_n)
    DevBuf face_n;   // unit face normals per primitive (MtsgLaunch::face_n)
    DevBuf nodes, hnodes, tris, prim_vtx, dpdu, positions, normals, shapes, bsdfs, emitters, area_cdf, em_cdf, sobol;
    DevBuf env, env_texels, env_rows, env_cols, env_weights, env_grows, env_gcols;
    DevBuf rtrans, texcoords, analytic, delta;
    DevBuf combos;   // mixturebsdf / blendbsdf / mask records (MtsgLaunch::combos)
    DevBuf qrays, qhits;      // mtsgpu_trace_rays staging
    DevBuf film_own, film_spill, samples, counters, contrib;
    DevBuf dev_in, dev_out;   // staging of mtsgpu_develop (host film -> developed image)
    DevBuf ldr_scratch;       // mtsgpu_develop_ldr, reinhard: log-luminance terms, luminances, the tonemapper's scalars
    DevBuf field_first;       // the field pass: first global primitive of each shape (MtsgFieldArgs::shape_first)
    std::vector<uint32_t> field_first_host;   // kept alive for the async upload
    // wavefront pipeline: path slots, ray queues and results, counters
    DevBuf wf_state, wf_ray, wf_rslot, wf_cls, wf_cnt, wf_hit, wf_hitrec, wf_occl, wf_live, wf_ovf, wf_part, wf_kind;
    DevBuf rp_order, rp_start, rp_sfmt;   // SFMT replay: render order, unit starts, streams
    // the reference's SAH kd-tree (kdtree_build.cpp), built on first use
    bool kd_built = false;
    KdTree kd;
    DevBuf kd_nodes, kd_indices, kd_tris;
    uint32_t *wf_live_host = nullptr;   // pinned: live-slot counts read back while the pipeline runs
    hipEvent_t wf_ev[8] = {};
    std::vector<uint32_t> wf_kind_host;   // shape -> shade kind (wf_kinds)
    unsigned long long last_counters[16] = {};
};

// Every object that takes an MtsgLaunch by value reports the size it was compiled with
// (launchers.h).  A library linked from objects of two layouts (a stale object after layout.h
// changed) would hand its kernels a misread launch record: refuse to run instead.
namespace {

// empty when every object agrees with this one on sizeof(MtsgLaunch), else what differs
const std::string &launch_layout_error() {
    static const std::string msg = [] {
        std::string m;
        const uint32_t mine = (uint32_t)sizeof(MtsgLaunch);
        const struct { const char *name; uint32_t bytes; } objs[] = {
            {"path_kernel", mtsg_launch_bytes_path_kernel()}, {"wf_kernel", mtsg_launch_bytes_wf_kernel()},
            {"field_kernel", mtsg_launch_bytes_field_kernel()},
#define MTSG_BYTES_ROW(N) {"path_f" #N, mtsg_launch_bytes_path_f##N()}, {"wf_shade_f" #N, mtsg_launch_bytes_wf_shade_f##N()},
            MTSG_FEAT_SETS(MTSG_BYTES_ROW)
#undef MTSG_BYTES_ROW
        };
        for (const auto &o : objs)
            if (o.bytes != mine)
                m += std::string(m.empty() ? "libmtsgpu.so mixes launch-record layouts (rebuild from clean): " : ", ") +
                     o.name + ".o has " + std::to_string(o.bytes) + " bytes, capi.o " + std::to_string(mine);
        return m;
    }();
    return msg;
}

int ensure_kdtree(mtsgpu_ctx *ctx);   // the reference's SAH kd-tree, built on first use (below)

// the `albedo` field and mtsgpu_albedo_factors_host over a scene with combinator BSDFs
const char *mtsg_albedo_combo_error() {
    return "the 'albedo' field is not supported in a scene with a mixturebsdf, blendbsdf or mask BSDF";
}

int fail(mtsgpu_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return code;
}

int hip_fail(mtsgpu_ctx *ctx, hipError_t e, const char *what) {
    return fail(ctx, e == hipErrorOutOfMemory ? MTSGPU_ENOMEM : MTSGPU_EHIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

// Sobol direction numbers as 4-bit XOR tables: [dim][c][v] = XOR of columns
// 4c..4c+3 of the dimension selected by the bits of v (sobolseq.h:43-57)
// (thread-safe: a static initialised once, group members upload concurrently)
std::vector<uint32_t> build_sobol_nibble_tables() {
    const std::vector<uint32_t> &M = mtsg_sobol_matrices();
    std::vector<uint32_t> T((size_t)MTSG_SOBOL_DIMS * MTSG_NIBBLES * 16, 0u);
    for (int d = 0; d < MTSG_SOBOL_DIMS; ++d)
        for (int c = 0; c < MTSG_NIBBLES; ++c)
            for (int v = 0; v < 16; ++v) {
                uint32_t r = 0;
                for (int b = 0; b < 4; ++b)
                    if ((v >> b) & 1) r ^= M[(size_t)d * MTSG_SOBOL_SIZE + 4 * c + b];
                T[((size_t)d * MTSG_NIBBLES + c) * 16 + v] = r;
            }
    return T;
}

const std::vector<uint32_t> &sobol_nibble_tables() {
    static const std::vector<uint32_t> T = build_sobol_nibble_tables();
    return T;
}

template <class T>
hipError_t upload(DevBuf &b, const std::vector<T> &v, hipStream_t s) {
    hipError_t e = b.ensure(v.size() * sizeof(T));
    if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

}  // namespace

extern "C" {

int mtsgpu_abi_version(void) { return MTSGPU_ABI_VERSION; }

int mtsgpu_create(int device, mtsgpu_ctx **out) {
    if (!out) return MTSGPU_EINVAL;
    *out = nullptr;
    if (!launch_layout_error().empty()) {   // before anything can be launched
        g_create_error = launch_layout_error();
        return MTSGPU_ESTATE;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_create_error = std::string("no HIP device: ") + hipGetErrorString(e);
        return MTSGPU_ENODEV;
    }
    if (device < 0) {
        e = hipGetDevice(&device);
        if (e != hipSuccess) device = 0;
    }
    if (device >= count) { g_create_error = "device index out of range"; return MTSGPU_ENODEV; }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return MTSGPU_EHIP;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("libmtsgpu.so is built for gfx950, device is ") + prop.gcnArchName;
        return MTSGPU_ENODEV;
    }
    mtsgpu_ctx *ctx = new mtsgpu_ctx();
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess) {
        g_create_error = std::string("HIP init: ") + hipGetErrorString(e);
        delete ctx;
        return MTSGPU_EHIP;
    }
    *out = ctx;
    return MTSGPU_OK;
}

int mtsgpu_upload_scene(mtsgpu_ctx *ctx, const mtsgpu_scene_desc *scene) {
    if (!ctx || !scene) return MTSGPU_EINVAL;
    ctx->have_scene = false;
    ctx->kd_built = false;
    std::string err;
    int rc = mtsg_configure_scene(scene, ctx->host, err);
    if (rc) return fail(ctx, rc, err);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    HostScene &H = ctx->host;
    hipStream_t s = ctx->stream;
    if ((e = upload(ctx->nodes, H.nodes, s)) != hipSuccess || (e = upload(ctx->hnodes, H.hnodes, s)) != hipSuccess ||
        (e = upload(ctx->tris, H.tris, s)) != hipSuccess ||
        (e = upload(ctx->prim_vtx, H.prim_vtx, s)) != hipSuccess || (e = upload(ctx->face_n, H.face_n, s)) != hipSuccess ||
        (e = upload(ctx->dpdu, H.dpdu, s)) != hipSuccess ||
        (e = upload(ctx->positions, H.positions, s)) != hipSuccess || (e = upload(ctx->normals, H.normals, s)) != hipSuccess ||
        (e = upload(ctx->shapes, H.shapes, s)) != hipSuccess || (e = upload(ctx->bsdfs, H.bsdfs, s)) != hipSuccess ||
        (e = upload(ctx->emitters, H.emitters, s)) != hipSuccess || (e = upload(ctx->area_cdf, H.area_cdf, s)) != hipSuccess ||
        (e = upload(ctx->em_cdf, H.em_cdf, s)) != hipSuccess || (e = upload(ctx->sobol, sobol_nibble_tables(), s)) != hipSuccess)
        return hip_fail(ctx, e, "scene upload");
    // tiny scenes: the scan's grouped records (render_plan.cpp mtsg_scan_layout)
    std::vector<MtsgTri> g;   // (lives until the sync below)
    scene_scan_n(H, g, H.launch.scan_n);
    if (!g.empty() && (e = upload(ctx->scan_tris, g, s)) != hipSuccess) return hip_fail(ctx, e, "scene upload");
    H.launch.one_emitter = scene_one_emitter(H);
    const MtsgEnv *denv = nullptr;
    if (H.env.emitter >= 0) {
        if ((e = upload(ctx->env_texels, H.env_texels, s)) != hipSuccess || (e = upload(ctx->env_rows, H.env_cdf_rows, s)) != hipSuccess ||
            (e = upload(ctx->env_cols, H.env_cdf_cols, s)) != hipSuccess || (e = upload(ctx->env_weights, H.env_row_weights, s)) != hipSuccess)
            return hip_fail(ctx, e, "envmap upload");
        H.env.texels = (const uint16_t *)ctx->env_texels.p;
        H.env.cdf_rows = (const float *)ctx->env_rows.p;
        H.env.cdf_cols = (const float *)ctx->env_cols.p;
        H.env.row_weights = (const float *)ctx->env_weights.p;
        H.env.guide_rows = H.env.guide_cols = nullptr;
        if (!H.env_guide_rows.empty()) {
            if ((e = upload(ctx->env_grows, H.env_guide_rows, s)) != hipSuccess ||
                (e = upload(ctx->env_gcols, H.env_guide_cols, s)) != hipSuccess)
                return hip_fail(ctx, e, "envmap upload");
            H.env.guide_rows = (const uint16_t *)ctx->env_grows.p;
            H.env.guide_cols = (const uint16_t *)ctx->env_gcols.p;
        }
        if ((e = ctx->env.ensure(sizeof(MtsgEnv))) != hipSuccess ||
            (e = hipMemcpyAsync(ctx->env.p, &H.env, sizeof(MtsgEnv), hipMemcpyHostToDevice, s)) != hipSuccess)
            return hip_fail(ctx, e, "envmap upload");
        denv = (const MtsgEnv *)ctx->env.p;
    }
    if ((!H.rtrans.empty() && (e = upload(ctx->rtrans, H.rtrans, s)) != hipSuccess) ||
        (!H.texcoords.empty() && (e = upload(ctx->texcoords, H.texcoords, s)) != hipSuccess) ||
        (!H.analytic.empty() && (e = upload(ctx->analytic, H.analytic, s)) != hipSuccess) ||
        (!H.deltas.empty() && (e = upload(ctx->delta, H.deltas, s)) != hipSuccess) ||
        (!H.combos.empty() && (e = upload(ctx->combos, H.combos, s)) != hipSuccess))
        return hip_fail(ctx, e, "texture/table upload");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "scene upload sync");
    MtsgDeviceScene &D = ctx->dscene;
    std::memset(&D, 0, sizeof D);
    D.nodes = (const MtsgNode *)ctx->nodes.p;
    D.hnodes = (const MtsgHNode *)ctx->hnodes.p;
    D.tris = (const MtsgTri *)ctx->tris.p;
    D.prim_vtx = (const uint32_t *)ctx->prim_vtx.p;
    D.dpdu = (const float *)ctx->dpdu.p;
    D.positions = (const float *)ctx->positions.p;
    D.normals = (const float *)ctx->normals.p;
    D.shapes = (const MtsgShape *)ctx->shapes.p;
    D.bsdfs = (const MtsgBsdf *)ctx->bsdfs.p;
    D.emitters = (const MtsgEmitter *)ctx->emitters.p;
    D.area_cdf = (const float *)ctx->area_cdf.p;
    D.em_cdf = (const float *)ctx->em_cdf.p;
    D.sobol = nullptr;
    scene_scalars(H, D);
    D.env = denv;
    D.rtrans = H.rtrans.empty() ? nullptr : (const float *)ctx->rtrans.p;
    D.texcoords = H.texcoords.empty() ? nullptr : (const float *)ctx->texcoords.p;
    D.analytic = H.analytic.empty() ? nullptr : (const MtsgAnalytic *)ctx->analytic.p;
    D.delta = H.deltas.empty() ? nullptr : (const MtsgDelta *)ctx->delta.p;
    ctx->have_scene = true;
    return MTSGPU_OK;
}

int mtsgpu_check_scene(const mtsgpu_scene_desc *scene, char *msg, size_t cap) {
    if (!scene) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    int rc = mtsg_configure_scene(scene, H, err);
    if (msg && cap) {
        std::strncpy(msg, err.c_str(), cap - 1);
        msg[cap - 1] = 0;
    }
    return rc;
}

int mtsgpu_film_border(int32_t rfilter, float rfilter_param) {
    MtsgFilter f;
    std::string err;
    if (mtsg_configure_filter(rfilter, rfilter_param, f, err)) return MTSGPU_EINVAL;
    return f.border;
}

// The wavefront engine for one chunk of samples (wf_kernel.hip): the MISS
// kernel starts every slot's first path, then bounce after bounce the shade
// kernel of each kind, then the trace kernel, until no path slot is live.  The
// live count of every POLL-th bounce is read back asynchronously; the host
// stays at most LAG polls ahead of the GPU, so the queues never drain and the
// overshoot (empty bounces) stays small.
static int wf_render_chunk(mtsgpu_ctx *ctx, const MtsgLaunch &L, bool instr, bool stats, hipStream_t stream,
                           const WfPlan &plan, const volatile int *cancel) {
    hipError_t e;
    const size_t R = MTSG_WF_REGIONS, cap = plan.cap, capCls = plan.capCls;
    MtsgLaunch Ls = L;   // the shade kernels' launch record (plan_wavefront)
    Ls.lds_dims = plan.shadeLdsDims;
    MtsgWave W;
    std::memset(&W, 0, sizeof W);
    W.state = (float4 *)ctx->wf_state.p;
    for (int p = 0; p < 2; ++p) {
        W.ray[p] = (float4 *)ctx->wf_ray.p + (size_t)p * 2 * R * cap * 2;
        W.rslot[p] = (uint32_t *)ctx->wf_rslot.p + (size_t)p * 2 * R * cap;
        W.cls[p] = (uint32_t *)ctx->wf_cls.p + (size_t)p * MTSG_WK_KINDS * R * capCls;
    }
    W.cnt = (uint32_t *)ctx->wf_cnt.p;
    W.hit = (float4 *)ctx->wf_hit.p;
    W.occl = (uint32_t *)ctx->wf_occl.p;
    W.live = (uint32_t *)ctx->wf_live.p;
    W.ovf = (uint2 *)ctx->wf_ovf.p;
    W.shape_kind = (const uint32_t *)ctx->wf_kind.p;
    W.slots = plan.slots;
    W.cap = (uint32_t)cap;
    W.cap_cls = (uint32_t)capCls;
    W.ovf_depth = (uint32_t)plan.ovfDepth;
    if (plan.hitrec) {
        W.hitrec = (float4 *)ctx->wf_hitrec.p;
        W.hitrec_uv = plan.hitrecUv ? 1u : 0u;
    }
    unsigned long long *part = (unsigned long long *)ctx->wf_part.p;
    const int partBlocks = plan.partBlocks;
    if ((e = hipMemsetAsync(ctx->wf_cnt.p, 0, (size_t)2 * MTSG_WF_QUEUES * R * 4, stream)) != hipSuccess ||
        (e = hipMemsetAsync(ctx->wf_live.p, 0, 2 * 4, stream)) != hipSuccess ||
        (e = hipMemsetAsync(part, 0, (size_t)partBlocks * 16 * 8, stream)) != hipSuccess)
        return hip_fail(ctx, e, "wavefront reset");
    constexpr int POLL = 4, LAG = 2, RING = 8;
    int polls = 0, checked = 0;
    const uint64_t maxBounces = (uint64_t)1 << 24;
    for (uint64_t it = 0;; ++it) {
        if (it >= maxBounces) return fail(ctx, MTSGPU_EHIP, "wavefront: no convergence");
        W.parity = (uint32_t)(it & 1);
        W.seed = it == 0 ? 1u : 0u;
        for (int k = 0; k < MTSG_WK_KINDS; ++k) {
            if (!plan.kinds[k] || (it == 0 && k != MTSG_WK_MISS)) continue;
            if ((e = mtsg_launch_wf_shade(Ls, W, part, plan.shadeGrid[k], k, plan.ggx[k], instr, stream)) != hipSuccess)
                return hip_fail(ctx, e, "wf_shade launch");
        }
        W.seed = 0;
        if (it % POLL == 0) {
            const int r = polls % RING;
            if ((e = hipMemcpyAsync(ctx->wf_live_host + r, W.live + W.parity, 4, hipMemcpyDeviceToHost,
                                    stream)) != hipSuccess ||
                (e = hipEventRecord(ctx->wf_ev[r], stream)) != hipSuccess)
                return hip_fail(ctx, e, "wavefront poll");
            ++polls;
        }
        if ((e = mtsg_launch_wf_trace(L, W, part, plan.traceGrid, stats, stream)) != hipSuccess)
            return hip_fail(ctx, e, "wf_trace launch");
        bool finished = false;
        while (!finished && polls > checked) {
            const int r = checked % RING;
            if (polls - checked <= LAG && hipEventQuery(ctx->wf_ev[r]) != hipSuccess) break;   // not yet, and not far ahead
            if ((e = hipEventSynchronize(ctx->wf_ev[r])) != hipSuccess) return hip_fail(ctx, e, "wavefront");
            ++checked;
            finished = ctx->wf_live_host[r] == 0;
        }
        if (finished) break;
        if (cancel && *cancel) break;
    }
    if ((e = mtsg_launch_wf_flush(part, (uint32_t)partBlocks, L.counters, stream)) != hipSuccess)
        return hip_fail(ctx, e, "wf_flush launch");
    return MTSGPU_OK;
}

// ---------------------------------------------------------------------------
// A render: what was asked (mtsgpu_render_params, a field list), what will be launched
// (render_plan.h: no HIP call), and launching it: render_impl and its stages below
// ---------------------------------------------------------------------------
// FJ: the field pass (mtsgpu_render_fields) -- the same window, sampler, filter, sharding and
// film machinery with field_kernel in place of the integrator's kernel; film_host / film_dev
// then hold FJ->n consecutive films and samples_host records of 4 + 3 * FJ->n floats
struct FieldJob { const mtsgpu_field_desc *fields; uint32_t n; };

namespace {

// what the stages of one render share
struct RenderRun {
    mtsgpu_ctx *ctx;
    const RenderPlan &plan;
    hipStream_t stream;
    MtsgLaunch L;        // the plan's launch record with the device pointers patched in
    float *own;          // the film(s) on the device
    MtsgFieldArgs FA;    // the field pass
    WfPlan wf;           // the wavefront engine
};

// allocate and clear the film, record and counter buffers; the launch record's pointers
int render_buffers(RenderRun &R, float *film_dev) {
    mtsgpu_ctx *ctx = R.ctx;
    const RenderPlan &p = R.plan;
    hipStream_t stream = R.stream;
    hipError_t e;
    if ((e = ctx->film_own.ensure(p.filmFloats * 4 * p.films)) != hipSuccess ||
        (e = ctx->film_spill.ensure(p.filmFloats * 8 * p.films)) != hipSuccess ||
        (e = ctx->counters.ensure(16 * 8)) != hipSuccess || (e = ctx->contrib.ensure(p.fieldBytes * p.films)) != hipSuccess)
        return hip_fail(ctx, e, "film allocation");
    R.own = film_dev ? film_dev : (float *)ctx->film_own.p;
    if (p.nsamp) {
        if ((e = ctx->samples.ensure(p.nsamp * 4)) != hipSuccess) return hip_fail(ctx, e, "sample buffer");
        if ((e = hipMemsetAsync(ctx->samples.p, 0, p.nsamp * 4, stream)) != hipSuccess) return hip_fail(ctx, e, "memset");
    }
    if ((e = hipMemsetAsync(R.own, 0, p.filmFloats * 4 * p.films, stream)) != hipSuccess ||
        (e = hipMemsetAsync(ctx->film_spill.p, 0, p.filmFloats * 8 * p.films, stream)) != hipSuccess ||
        (e = hipMemsetAsync(ctx->counters.p, 0, 16 * 8, stream)) != hipSuccess)
        return hip_fail(ctx, e, "memset");
    MtsgLaunch &L = R.L;
    L = p.L;
    L.scene = ctx->dscene;
    L.face_n = (const float *)ctx->face_n.p;
    L.sobol_nib = (const uint32_t *)ctx->sobol.p;
    L.scan_tris = (const MtsgTri *)ctx->scan_tris.p;
    L.combos = ctx->host.combos.empty() ? nullptr : (const MtsgCombo *)ctx->combos.p;
    L.film_own = R.own;
    L.film_spill = (double *)ctx->film_spill.p;
    L.samples = p.nsamp ? (float *)ctx->samples.p : nullptr;
    L.contrib = (float *)ctx->contrib.p;
    L.counters = (unsigned long long *)ctx->counters.p;
    return MTSGPU_OK;
}

// the field pass: field_kernel's second argument
int render_field_args(RenderRun &R, const FieldJob &FJ) {
    mtsgpu_ctx *ctx = R.ctx;
    const RenderPlan &p = R.plan;
    const HostScene &H = ctx->host;
    MtsgFieldArgs &FA = R.FA;
    FA.num_fields = p.films;
    FA.record_floats = (uint32_t)p.recFloats;
    FA.contrib_stride = p.fieldBytes / 4;
    for (uint32_t f = 0; f < p.films; ++f) {
        FA.field[f] = FJ.fields[f].field;
        for (int k = 0; k < 3; ++k) FA.undefined[f][k] = FJ.fields[f].undefined[k];
        FA.spill[f] = R.L.film_spill + f * p.filmFloats;
    }
    std::memcpy(FA.world_to_cam, p.world_to_cam, sizeof FA.world_to_cam);
    // its.primIndex counts within the mesh: the first global primitive of each shape
    std::vector<uint32_t> &first = ctx->field_first_host;
    first.assign(H.shapes.size(), 0u);
    for (size_t q = H.prim_vtx.size() / 4; q-- > 0;) first[H.prim_vtx[4 * q + 3]] = (uint32_t)q;
    const hipError_t e = upload(ctx->field_first, first, R.stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "field upload");
    FA.shape_first = (const uint32_t *)ctx->field_first.p;
    return MTSGPU_OK;
}

// the SFMT replay: render order, unit starts and streams (replay_host.cpp)
int render_replay(RenderRun &R, const mtsgpu_render_params &P) {
    mtsgpu_ctx *ctx = R.ctx;
    MtsgLaunch &L = R.L;
    std::vector<uint32_t> order, unitStart, streams;
    mtsg_replay_tables(P.width, P.height, P.sampler == MTSGPU_SAMPLER_SFMT_BLOCKS, order, unitStart, streams);
    if (unitStart.size() - 1 != L.units) return fail(ctx, MTSGPU_ESTATE, "SFMT replay: the plan's units are not the render order's");
    hipError_t e;
    if ((e = upload(ctx->rp_order, order, R.stream)) != hipSuccess || (e = upload(ctx->rp_start, unitStart, R.stream)) != hipSuccess ||
        (e = upload(ctx->rp_sfmt, streams, R.stream)) != hipSuccess ||
        (e = hipStreamSynchronize(R.stream)) != hipSuccess)   // the host vectors go out of scope
        return hip_fail(ctx, e, "replay upload");
    L.order = (const uint32_t *)ctx->rp_order.p;
    L.unit_start = (const uint32_t *)ctx->rp_start.p;
    L.sfmt = (uint32_t *)ctx->rp_sfmt.p;
    return MTSGPU_OK;
}

// the wavefront engine: the kd-tree where wanted, the kernels' occupancy, the queues (plan_wavefront)
int render_wavefront_buffers(RenderRun &R, const RenderKnobs &K) {
    mtsgpu_ctx *ctx = R.ctx;
    MtsgLaunch &L = R.L;
    hipStream_t stream = R.stream;
    hipError_t e;
    if (R.plan.kdtree) {
        const int rc = ensure_kdtree(ctx);
        if (rc) return rc;
        L.kd_nodes = (const uint32_t *)ctx->kd_nodes.p;
        L.kd_indices = (const uint32_t *)ctx->kd_indices.p;
        L.kd_tris = (const MtsgTri *)ctx->kd_tris.p;
    }
    R.wf = plan_wavefront(R.plan, ctx->host, K);
    const WfPlan &wf = R.wf;
    for (int k = 0; k < MTSG_WK_KINDS; ++k) {
        if (!wf.kinds[k]) continue;
        int sb = 0, tb = 0;
        mtsg_wf_occupancy(L, k, wf.ggx[k], &sb, &tb);
        if (sb <= 0 || tb <= 0) return fail(ctx, MTSGPU_EHIP, "wavefront kernels do not fit the device");
    }
    ctx->wf_kind_host = wf.shapeKind;   // kept alive for the async upload
    const size_t Rg = MTSG_WF_REGIONS, slots = wf.slots;
    if ((e = ctx->wf_state.ensure((size_t)MTSG_WF_STATE_VECS * slots * 16)) != hipSuccess ||
        (e = ctx->wf_ray.ensure((size_t)2 * 2 * Rg * wf.cap * 32)) != hipSuccess ||
        (e = ctx->wf_rslot.ensure((size_t)2 * 2 * Rg * wf.cap * 4)) != hipSuccess ||
        (e = ctx->wf_cls.ensure((size_t)2 * MTSG_WK_KINDS * Rg * wf.capCls * 4)) != hipSuccess ||
        (e = ctx->wf_cnt.ensure((size_t)2 * MTSG_WF_QUEUES * Rg * 4)) != hipSuccess ||
        (e = ctx->wf_hit.ensure(slots * 16)) != hipSuccess ||
        (wf.hitrec && (e = ctx->wf_hitrec.ensure(slots * MTSG_WF_HIT_VECS * 16)) != hipSuccess) ||
        (e = ctx->wf_occl.ensure(slots * 4)) != hipSuccess ||
        (e = ctx->wf_live.ensure(2 * 4)) != hipSuccess ||
        (e = ctx->wf_ovf.ensure((size_t)wf.traceGrid * MTSG_BLOCK * wf.ovfDepth * 8)) != hipSuccess ||
        (e = ctx->wf_part.ensure((size_t)wf.partBlocks * 16 * 8)) != hipSuccess ||
        (e = upload(ctx->wf_kind, ctx->wf_kind_host, stream)) != hipSuccess)
        return hip_fail(ctx, e, "wavefront buffers");
    if (!ctx->wf_live_host) {
        if ((e = hipHostMalloc((void **)&ctx->wf_live_host, 8 * sizeof(uint32_t))) != hipSuccess)
            return hip_fail(ctx, e, "wavefront pinned buffer");
        for (hipEvent_t &ev : ctx->wf_ev)
            if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return hip_fail(ctx, e, "event");
    }
    return MTSGPU_OK;
}

// the chunk loop: per launch of the plan the engine's kernels, then the film kernels;
// launched: the loop's iterations (debug counter 8)
int render_launches(RenderRun &R, const volatile int *cancel, unsigned long long &launched) {
    mtsgpu_ctx *ctx = R.ctx;
    const RenderPlan &p = R.plan;
    MtsgLaunch &L = R.L;
    hipStream_t stream = R.stream;
    hipError_t e;
    int bpc = 0;   // resident blocks per CU of the persistent kernel
    if (p.engine == MTSG_ENGINE_FIELDS) mtsg_field_occupancy(L, &bpc);
    else if (p.engine == MTSG_ENGINE_MEGAKERNEL) mtsg_path_kernel_occupancy(L, &bpc);
    if ((e = hipEventRecord(ctx->ev0, stream)) != hipSuccess) return hip_fail(ctx, e, "event");
    launched = 0;
    for (uint32_t j0 = 0; j0 < L.spp; j0 += p.chunk) {
        if (cancel && *cancel) break;
        ++launched;
        const LaunchPlan lp = plan_launch(p, j0, bpc);
        if (lp.err) return fail(ctx, MTSGPU_EINVAL, lp.err);
        L.j0 = j0;
        L.chunk_spp = lp.chunk_spp;
        L.num_items = lp.num_items;
        if (p.engine == MTSG_ENGINE_WAVEFRONT) {
            const int rc = wf_render_chunk(ctx, L, p.instr, p.stats_mode, stream, R.wf, cancel);
            if (rc != MTSGPU_OK) return rc;
        } else {
            L.round_shift = lp.round_shift;
            mtsg_launch_index(L, (uint64_t)lp.grid * MTSG_BLOCK);
            if (p.engine == MTSG_ENGINE_FIELDS) {
                if ((e = mtsg_launch_field(L, R.FA, lp.grid, stream)) != hipSuccess) return hip_fail(ctx, e, "field kernel launch");
            } else if ((e = mtsg_launch_path(L, lp.grid, p.nsamp != 0, p.stats_mode, stream)) != hipSuccess) {
                return hip_fail(ctx, e, "path kernel launch");
            }
        }
        // (the field pass: every field's record array into its own film, by the same kernels)
        for (uint32_t f = 0; f < p.films; ++f) {
            MtsgLaunch Lf = L;
            Lf.contrib = L.contrib + f * (p.fieldBytes / 4);
            Lf.film_own = R.own + f * p.filmFloats;
            if ((e = Lf.gather ? mtsg_launch_gather(Lf, stream) : mtsg_launch_reduce(Lf, stream)) != hipSuccess)
                return hip_fail(ctx, e, "film reduce launch");
        }
    }
    if ((e = hipEventRecord(ctx->ev1, stream)) != hipSuccess) return hip_fail(ctx, e, "event");
    return MTSGPU_OK;
}

// finalize the film(s), read back, fill the stats, set debug counters 8 and 15
int render_readback(RenderRun &R, float *film_host, float *samples_host, mtsgpu_stats *stats, unsigned long long launched) {
    mtsgpu_ctx *ctx = R.ctx;
    const RenderPlan &p = R.plan;
    hipStream_t stream = R.stream;
    hipError_t e;
    if ((e = mtsg_launch_finalize(R.own, R.L.film_spill, p.filmFloats * p.films, stream)) != hipSuccess)
        return hip_fail(ctx, e, "finalize launch");
    unsigned long long hc[16];
    if ((e = hipMemcpyAsync(hc, R.L.counters, sizeof hc, hipMemcpyDeviceToHost, stream)) != hipSuccess) return hip_fail(ctx, e, "counters");
    if (film_host && (e = hipMemcpyAsync(film_host, R.own, p.filmFloats * 4 * p.films, hipMemcpyDeviceToHost, stream)) != hipSuccess)
        return hip_fail(ctx, e, "film copy");
    if (p.nsamp && (e = hipMemcpyAsync(samples_host, ctx->samples.p, p.nsamp * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess)
        return hip_fail(ctx, e, "sample copy");
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return hip_fail(ctx, e, "path kernel");
    std::memcpy(ctx->last_counters, hc, sizeof hc);
    // counter 8: the launches the sample count was split into (the chunk loop's iterations)
    ctx->last_counters[8] = launched;
    // counter 15: which kernel ran (render_plan.cpp plan_variant_word)
    ctx->last_counters[15] = plan_variant_word(p);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (stats) {
        stats->samples = hc[0];
        stats->rays = hc[1];
        stats->shadow_rays = hc[2];
        stats->path_length_sum = hc[3];
        stats->node_visits = p.stats_mode ? hc[4] : 0;
        stats->tri_tests = p.stats_mode ? hc[5] : 0;
        stats->hits = p.stats_mode ? hc[7] : 0;
        stats->nee_samples = p.stats_mode ? hc[9] : 0;
        stats->sobol_reads = p.stats_mode ? hc[10] : 0;
        stats->kernel_ms = ms;
    }
    if (hc[6]) return fail(ctx, MTSGPU_EDIM, "Lookup dimension exceeds the direction number table size! You may have to "
                                             "reduce the 'maxDepth' parameter of your integrator.");
    return MTSGPU_OK;
}

}  // namespace

static int render_impl(mtsgpu_ctx *ctx, const mtsgpu_render_params *P, float *film_host, float *film_dev,
                       float *samples_host, hipStream_t stream, mtsgpu_stats *stats, const FieldJob *FJ = nullptr) {
    if (!ctx || !P) return MTSGPU_EINVAL;
    if (!ctx->have_scene) return fail(ctx, MTSGPU_ESTATE, "render called before a successful upload_scene");
    if (!launch_layout_error().empty()) return fail(ctx, MTSGPU_ESTATE, launch_layout_error());
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    // what the plan needs to know of the device, the environment once per render, the plan
    DeviceFacts dev = {ctx->num_cus, 0, ctx->contrib.bytes};
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) dev.free_bytes = freeB;
    const RenderKnobs K = read_knobs();
    RenderPlan plan;
    std::string err;
    int rc = plan_render(ctx->host, *P, FJ ? FJ->n : 0u, samples_host != nullptr, dev, K, plan, err);
    if (rc) return fail(ctx, rc, err);
    if (P->cancel && *P->cancel) return fail(ctx, MTSGPU_ECANCEL, "cancelled");

    RenderRun R = {ctx, plan, stream ? stream : ctx->stream};
    std::memset(&R.FA, 0, sizeof R.FA);
    unsigned long long launched = 0;
    if ((rc = render_buffers(R, film_dev)) != MTSGPU_OK) return rc;
    if (FJ && (rc = render_field_args(R, *FJ)) != MTSGPU_OK) return rc;
    if (plan.replay && (rc = render_replay(R, *P)) != MTSGPU_OK) return rc;
    if (plan.engine == MTSG_ENGINE_WAVEFRONT && (rc = render_wavefront_buffers(R, K)) != MTSGPU_OK) return rc;
    if ((rc = render_launches(R, P->cancel, launched)) != MTSGPU_OK) return rc;
    if ((rc = render_readback(R, film_host, samples_host, stats, launched)) != MTSGPU_OK) return rc;
    if (P->cancel && *P->cancel) return fail(ctx, MTSGPU_ECANCEL, "cancelled");
    return MTSGPU_OK;
}

int mtsgpu_render(mtsgpu_ctx *ctx, const mtsgpu_render_params *params, float *film, float *samples, mtsgpu_stats *stats) {
    if (!film) return fail(ctx, MTSGPU_EINVAL, "film buffer is NULL");
    return render_impl(ctx, params, film, nullptr, samples, nullptr, stats);
}

int mtsgpu_render_device(mtsgpu_ctx *ctx, const mtsgpu_render_params *params, float *film_device, void *stream,
                         mtsgpu_stats *stats) {
    if (!film_device) return fail(ctx, MTSGPU_EINVAL, "film buffer is NULL");
    return render_impl(ctx, params, nullptr, film_device, nullptr, (hipStream_t)stream, stats);
}

namespace {
int field_job_check(mtsgpu_ctx *ctx, const mtsgpu_field_desc *fields, uint32_t n) {
    if (!ctx) return MTSGPU_EINVAL;
    if (!fields) return fail(ctx, MTSGPU_EINVAL, "field list is NULL");
    if (n == 0) return fail(ctx, MTSGPU_EINVAL, "No sub-integrators were supplied to the multi-channel integrator!");
    if (n > MTSGPU_MAX_FIELDS) return fail(ctx, MTSGPU_EINVAL, "at most 8 fields per pass");
    for (uint32_t f = 0; f < n; ++f)
        if (fields[f].field < 0 || fields[f].field >= MTSGPU_FIELD_COUNT)
            return fail(ctx, MTSGPU_EINVAL, "Invalid 'field' parameter. Must be one of 'position', 'relPosition', 'distance', "
                                            "'geoNormal', 'shNormal', 'primIndex', 'shapeIndex', or 'uv'!");
    // getDiffuseReflectance of a mixturebsdf / blendbsdf / mask is not restated: the field pass
    // (field_kernel.hip field_albedo) knows the leaves and twosided only
    for (uint32_t f = 0; f < n; ++f)
        if (fields[f].field == MTSGPU_FIELD_ALBEDO && ctx->have_scene && !ctx->host.combos.empty())
            return fail(ctx, MTSGPU_EINVAL, mtsg_albedo_combo_error());
    return MTSGPU_OK;
}
}  // namespace

int mtsgpu_render_fields(mtsgpu_ctx *ctx, const mtsgpu_render_params *params, const mtsgpu_field_desc *fields,
                         uint32_t num_fields, float *films, float *samples, mtsgpu_stats *stats) {
    const int rc = field_job_check(ctx, fields, num_fields);
    if (rc != MTSGPU_OK) return rc;
    if (!films) return fail(ctx, MTSGPU_EINVAL, "film buffer is NULL");
    const FieldJob job = {fields, num_fields};
    return render_impl(ctx, params, films, nullptr, samples, nullptr, stats, &job);
}

int mtsgpu_render_fields_device(mtsgpu_ctx *ctx, const mtsgpu_render_params *params, const mtsgpu_field_desc *fields,
                                uint32_t num_fields, float *films_device, void *stream, mtsgpu_stats *stats) {
    const int rc = field_job_check(ctx, fields, num_fields);
    if (rc != MTSGPU_OK) return rc;
    if (!films_device) return fail(ctx, MTSGPU_EINVAL, "film buffer is NULL");
    const FieldJob job = {fields, num_fields};
    return render_impl(ctx, params, nullptr, films_device, nullptr, (hipStream_t)stream, stats, &job);
}

// hdrfilm develop (film_kernel.hip)
namespace {
int develop_check(mtsgpu_ctx *ctx, const mtsgpu_develop_params *P, size_t *out_bytes) {
    if (!ctx) return MTSGPU_EINVAL;
    if (!P) return fail(ctx, MTSGPU_EINVAL, "develop params are NULL");
    const int ch = mtsg_develop_channels(P->pixel_format);
    if (!ch) return fail(ctx, MTSGPU_EINVAL, "develop: unknown pixel format");
    if (P->component_format < MTSGPU_COMP_FLOAT16 || P->component_format > MTSGPU_COMP_UINT32)
        return fail(ctx, MTSGPU_EINVAL, "develop: unknown component format");
    if (P->film_width <= 2 * P->border || P->film_height <= 2 * P->border)
        return fail(ctx, MTSGPU_EINVAL, "develop: film smaller than its borders");
    const size_t n = (size_t)(P->film_width - 2 * P->border) * (P->film_height - 2 * P->border);
    *out_bytes = n * ch * (P->component_format == MTSGPU_COMP_FLOAT16 ? 2 : 4);
    return MTSGPU_OK;
}
}  // namespace

int mtsgpu_develop_device(mtsgpu_ctx *ctx, const mtsgpu_develop_params *P, const float *film_device,
                          void *out_device, void *stream) {
    size_t ob = 0;
    int rc = develop_check(ctx, P, &ob);
    if (rc != MTSGPU_OK) return rc;
    if (!film_device || !out_device) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    hipError_t e = mtsg_launch_develop(*P, film_device, out_device, ctx->num_cus, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? MTSGPU_OK : hip_fail(ctx, e, "develop");
}

int mtsgpu_develop(mtsgpu_ctx *ctx, const mtsgpu_develop_params *P, const float *film, void *out) {
    size_t ob = 0;
    int rc = develop_check(ctx, P, &ob);
    if (rc != MTSGPU_OK) return rc;
    if (!film || !out) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
    (void)hipSetDevice(ctx->device);
    const size_t ib = (size_t)P->film_width * P->film_height * 5 * sizeof(float);
    hipError_t e;
    if ((e = ctx->dev_in.ensure(ib)) != hipSuccess || (e = ctx->dev_out.ensure(ob)) != hipSuccess)
        return hip_fail(ctx, e, "develop buffers");
    hipStream_t s = ctx->stream;
    if ((e = hipMemcpyAsync(ctx->dev_in.p, film, ib, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = mtsg_launch_develop(*P, (const float *)ctx->dev_in.p, ctx->dev_out.p, ctx->num_cus, s)) != hipSuccess ||
        (e = hipMemcpyAsync(out, ctx->dev_out.p, ob, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(ctx, e, "develop");
    return MTSGPU_OK;
}

namespace {
int develop_multi_check(mtsgpu_ctx *ctx, const mtsgpu_develop_multi_params *P, const float *const *films, size_t *out_bytes) {
    if (!ctx) return MTSGPU_EINVAL;
    if (!P || !films) return fail(ctx, MTSGPU_EINVAL, "develop: NULL argument");
    if (P->num_films == 0 || P->num_films > MTSGPU_MAX_FIELDS + 1) return fail(ctx, MTSGPU_EINVAL, "develop: bad film count");
    size_t ch = 0;
    for (uint32_t f = 0; f < P->num_films; ++f) {
        const int c = mtsg_develop_channels(P->pixel_format[f]);
        if (!c) return fail(ctx, MTSGPU_EINVAL, "develop: unknown pixel format");
        if (!films[f]) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
        ch += (size_t)c;
    }
    if (P->component_format < MTSGPU_COMP_FLOAT16 || P->component_format > MTSGPU_COMP_UINT32)
        return fail(ctx, MTSGPU_EINVAL, "develop: unknown component format");
    if (P->film_width <= 2 * P->border || P->film_height <= 2 * P->border)
        return fail(ctx, MTSGPU_EINVAL, "develop: film smaller than its borders");
    const size_t n = (size_t)(P->film_width - 2 * P->border) * (P->film_height - 2 * P->border);
    *out_bytes = n * ch * (P->component_format == MTSGPU_COMP_FLOAT16 ? 2 : 4);
    return MTSGPU_OK;
}
}  // namespace

int mtsgpu_develop_multi_device(mtsgpu_ctx *ctx, const mtsgpu_develop_multi_params *P, const float *const *films,
                                void *out_device, void *stream) {
    size_t ob = 0;
    const int rc = develop_multi_check(ctx, P, films, &ob);
    if (rc != MTSGPU_OK) return rc;
    if (!out_device) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    hipError_t e = mtsg_launch_develop_multi(*P, films, out_device, ctx->num_cus, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? MTSGPU_OK : hip_fail(ctx, e, "develop");
}

int mtsgpu_develop_multi(mtsgpu_ctx *ctx, const mtsgpu_develop_multi_params *P, const float *const *films, void *out) {
    size_t ob = 0;
    const int rc = develop_multi_check(ctx, P, films, &ob);
    if (rc != MTSGPU_OK) return rc;
    if (!out) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
    (void)hipSetDevice(ctx->device);
    const size_t ib = (size_t)P->film_width * P->film_height * 5 * sizeof(float);
    hipError_t e;
    if ((e = ctx->dev_in.ensure(ib * P->num_films)) != hipSuccess || (e = ctx->dev_out.ensure(ob)) != hipSuccess)
        return hip_fail(ctx, e, "develop buffers");
    hipStream_t s = ctx->stream;
    const float *dev[MTSGPU_MAX_FIELDS + 1] = {};
    for (uint32_t f = 0; f < P->num_films; ++f) {
        dev[f] = (const float *)((const char *)ctx->dev_in.p + f * ib);
        if ((e = hipMemcpyAsync((void *)dev[f], films[f], ib, hipMemcpyHostToDevice, s)) != hipSuccess)
            return hip_fail(ctx, e, "develop");
    }
    if ((e = mtsg_launch_develop_multi(*P, dev, ctx->dev_out.p, ctx->num_cus, s)) != hipSuccess ||
        (e = hipMemcpyAsync(out, ctx->dev_out.p, ob, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(ctx, e, "develop");
    return MTSGPU_OK;
}

// ldrfilm develop (ldrfilm_kernel.hip): LDRFilm::develop (src/films/ldrfilm.cpp:300-321) ->
// Bitmap::convert to uint8 (src/libcore/fmtconv.cpp:955-1005, 1104-1111, 1137-1160) and, for the
// reinhard method, Bitmap::tonemapReinhard (src/libcore/bitmap.cpp:1711-1854)
namespace {
int develop_ldr_check(mtsgpu_ctx *ctx, const mtsgpu_develop_ldr_params *P, const void *out, size_t *out_bytes) {
    if (!ctx) return MTSGPU_EINVAL;
    if (!P) return fail(ctx, MTSGPU_EINVAL, "develop params are NULL");
    if (P->pixel_format < MTSGPU_PIX_LUMINANCE || P->pixel_format > MTSGPU_PIX_RGBA)   // ldrfilm.cpp:159-170
        return fail(ctx, MTSGPU_EINVAL, "develop_ldr: the pixel format must be luminance, luminanceAlpha, rgb or rgba");
    if (P->tonemap_method != MTSGPU_TONEMAP_GAMMA && P->tonemap_method != MTSGPU_TONEMAP_REINHARD)
        return fail(ctx, MTSGPU_EINVAL, "develop_ldr: unknown tonemap method");
    if (P->film_width <= 2 * P->border || P->film_height <= 2 * P->border)
        return fail(ctx, MTSGPU_EINVAL, "develop: film smaller than its borders");
    const size_t ch = (size_t)mtsg_develop_channels(P->pixel_format);
    // a pixel of 2 or 4 bytes is written by one store
    if (out && (ch == 2 || ch == 4) && (uintptr_t)out % ch != 0)
        return fail(ctx, MTSGPU_EINVAL, "develop_ldr: output not aligned to its pixel size");
    *out_bytes = (size_t)(P->film_width - 2 * P->border) * (P->film_height - 2 * P->border) * ch;
    return MTSGPU_OK;
}

// launch on `s`, wait, and hand back {logAvgLuminance, maxLuminance}
int develop_ldr_run(mtsgpu_ctx *ctx, const mtsgpu_develop_ldr_params *P, const float *film_device,
                    uint8_t *out_device, uint8_t *out_host, size_t ob, hipStream_t s, float info2[2]) {
    hipError_t e;
    const size_t sb = mtsg_develop_ldr_scratch(*P);
    if (sb && (e = ctx->ldr_scratch.ensure(sb)) != hipSuccess) return hip_fail(ctx, e, "develop buffers");
    float info[2] = {0.0f, 0.0f};
    if ((e = mtsg_launch_develop_ldr(*P, film_device, out_device, sb ? ctx->ldr_scratch.p : nullptr, ctx->num_cus,
                                     s)) != hipSuccess ||
        (out_host && (e = hipMemcpyAsync(out_host, out_device, ob, hipMemcpyDeviceToHost, s)) != hipSuccess) ||
        (sb && info2 &&
         (e = hipMemcpyAsync(info, (const char *)ctx->ldr_scratch.p + mtsg_develop_ldr_info_offset(), sizeof(info),
                             hipMemcpyDeviceToHost, s)) != hipSuccess) ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(ctx, e, "develop_ldr");
    if (info2) {
        info2[0] = info[0];
        info2[1] = info[1];
    }
    return MTSGPU_OK;
}
}  // namespace

int mtsgpu_develop_ldr_device(mtsgpu_ctx *ctx, const mtsgpu_develop_ldr_params *P, const float *film_device,
                              uint8_t *out_device, void *stream, float info2[2]) {
    size_t ob = 0;
    const int rc = develop_ldr_check(ctx, P, out_device, &ob);
    if (rc != MTSGPU_OK) return rc;
    if (!film_device || !out_device) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
    (void)hipSetDevice(ctx->device);
    return develop_ldr_run(ctx, P, film_device, out_device, nullptr, ob, stream ? (hipStream_t)stream : ctx->stream,
                           info2);
}

int mtsgpu_develop_ldr(mtsgpu_ctx *ctx, const mtsgpu_develop_ldr_params *P, const float *film, uint8_t *out,
                       float info2[2]) {
    size_t ob = 0;
    const int rc = develop_ldr_check(ctx, P, nullptr, &ob);
    if (rc != MTSGPU_OK) return rc;
    if (!film || !out) return fail(ctx, MTSGPU_EINVAL, "develop: NULL buffer");
    (void)hipSetDevice(ctx->device);
    const size_t ib = (size_t)P->film_width * P->film_height * 5 * sizeof(float);
    hipError_t e;
    if ((e = ctx->dev_in.ensure(ib)) != hipSuccess || (e = ctx->dev_out.ensure(ob)) != hipSuccess)
        return hip_fail(ctx, e, "develop buffers");
    hipStream_t s = ctx->stream;
    if ((e = hipMemcpyAsync(ctx->dev_in.p, film, ib, hipMemcpyHostToDevice, s)) != hipSuccess)
        return hip_fail(ctx, e, "develop_ldr");
    return develop_ldr_run(ctx, P, (const float *)ctx->dev_in.p, (uint8_t *)ctx->dev_out.p, out, ob, s, info2);
}

int mtsgpu_albedo_factors_host(const mtsgpu_scene_desc *scene, float *factors, char *msg, size_t cap) {
    if (!scene || !factors) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    const int rc = mtsg_configure_scene(scene, H, err);
    if (rc != MTSGPU_OK) {
        if (msg && cap) std::snprintf(msg, cap, "%s", err.c_str());
        return rc;
    }
    if (!H.combos.empty()) {   // (the `albedo` field refuses such a scene too: field_job_check, below)
        if (msg && cap) std::snprintf(msg, cap, "%s", mtsg_albedo_combo_error());
        return MTSGPU_EINVAL;
    }
    for (uint32_t i = 0; i < scene->num_bsdfs; ++i) {
        const MtsgBsdf &b = H.bsdfs[i];
        // (phong: diffuseReflectance, roughdiffuse: reflectance, as they are; difftrans: 0)
        factors[i] = (b.type == MTSGPU_BSDF_DIFFUSE || b.type == MTSGPU_BSDF_PHONG || b.type == MTSGPU_BSDF_ROUGHDIFFUSE) ? 1.0f
                   : b.type == MTSGPU_BSDF_PLASTIC ? 1 - b.fdr_ext
                   : b.type == MTSGPU_BSDF_ROUGHPLASTIC ? (b.alpha_tex.type ? -1.0f : b.ftr_ext) : 0.0f;
    }
    return MTSGPU_OK;
}

int mtsgpu_combo_host(const mtsgpu_scene_desc *scene, uint32_t bsdf, float *out21, int32_t *flags, char *msg,
                      size_t cap) {
    if (!scene || !out21) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    int rc = mtsg_configure_scene(scene, H, err);
    if (!rc && (bsdf >= scene->num_bsdfs || H.bsdfs[bsdf].type < MTSGPU_BSDF_MIXTURE)) {
        err = "mtsgpu_combo_host: not a mixturebsdf, blendbsdf or mask";
        rc = MTSGPU_EINVAL;
    }
    if (msg && cap) std::snprintf(msg, cap, "%s", err.c_str());
    if (rc) return rc;
    const MtsgCombo &c = H.combos[H.bsdfs[bsdf].nested[0]];
    out21[0] = (float)c.n;
    std::memcpy(out21 + 1, c.w, sizeof c.w);
    std::memcpy(out21 + 9, c.cdf, sizeof c.cdf);
    std::memcpy(out21 + 18, c.value, sizeof c.value);
    if (flags) *flags = H.bsdfs[bsdf].flags;
    return MTSGPU_OK;
}

int mtsgpu_leaf_host(const mtsgpu_scene_desc *scene, uint32_t bsdf, float *out16, int32_t *flags, char *msg,
                     size_t cap) {
    if (!scene || !out16) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    int rc = mtsg_configure_scene(scene, H, err);
    if (!rc && (bsdf >= scene->num_bsdfs || H.bsdfs[bsdf].type < MTSGPU_BSDF_DIFFTRANS)) {
        err = "mtsgpu_leaf_host: not a difftrans, roughdiffuse or phong";
        rc = MTSGPU_EINVAL;
    }
    if (msg && cap) std::snprintf(msg, cap, "%s", err.c_str());
    if (rc) return rc;
    const MtsgBsdf &b = H.bsdfs[bsdf];
    for (int i = 0; i < 3; ++i) {
        out16[i] = b.refl_tex.type ? b.refl_tex.c0[i] : b.refl[i];
        out16[3 + i] = b.refl_tex.type ? b.refl_tex.c1[i] : b.refl[i];
        out16[6 + i] = b.spec_r[i];
        out16[9 + i] = b.spec_t[i];
    }
    out16[12] = b.spec_weight;
    out16[13] = b.eta;
    out16[14] = b.alpha_u;
    out16[15] = (float)b.nonlinear;
    if (flags) *flags = b.flags;
    return MTSGPU_OK;
}

const char *mtsgpu_last_error(mtsgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void mtsgpu_destroy(mtsgpu_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    DevBuf *bufs[] = {&ctx->face_n, &ctx->scan_tris, &ctx->kd_nodes, &ctx->kd_indices, &ctx->kd_tris, &ctx->nodes, &ctx->hnodes, &ctx->tris, &ctx->prim_vtx, &ctx->dpdu, &ctx->positions, &ctx->normals,
                      &ctx->shapes, &ctx->bsdfs, &ctx->emitters, &ctx->area_cdf, &ctx->em_cdf, &ctx->sobol,
                      &ctx->film_own, &ctx->film_spill, &ctx->samples, &ctx->counters, &ctx->contrib,
                      &ctx->env, &ctx->env_texels, &ctx->env_rows, &ctx->env_cols, &ctx->env_weights, &ctx->env_grows, &ctx->env_gcols,
                      &ctx->rtrans, &ctx->texcoords, &ctx->delta, &ctx->combos, &ctx->qrays, &ctx->qhits, &ctx->field_first,
                      &ctx->dev_in, &ctx->dev_out, &ctx->ldr_scratch, &ctx->wf_state, &ctx->wf_ray, &ctx->wf_rslot, &ctx->wf_cls,
                      &ctx->wf_cnt, &ctx->wf_hit, &ctx->wf_hitrec, &ctx->wf_occl, &ctx->wf_live, &ctx->wf_ovf, &ctx->wf_part, &ctx->wf_kind, &ctx->rp_order, &ctx->rp_start, &ctx->rp_sfmt, &ctx->env_grows, &ctx->env_gcols};
    for (DevBuf *b : bufs) b->release();
    for (hipEvent_t &e : ctx->wf_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->wf_live_host) (void)hipHostFree(ctx->wf_live_host);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

namespace {
// the kd-tree over the uploaded scene's triangles (global primitive order: the
// TriAccel slots carry their primitive number), uploaded with TriAccel records
// in that order; scenes with analytic shapes are not supported here
// host part: the tree over the configured scene's triangles in global order
int build_kd_host(const HostScene &H, KdTree &kd, std::vector<MtsgTri> *tg, std::string &err) {
    if (!H.analytic.empty()) { err = "kd-tree: scenes with analytic shapes are not supported"; return MTSGPU_EINVAL; }
    const size_t prims = H.tris.size();
    std::vector<float> P(prims * 9);
    if (tg) tg->assign(prims, MtsgTri());
    for (size_t s = 0; s < prims; ++s) {
        const uint32_t prim = H.tris[s].prim;
        if (prim >= prims) { err = "kd-tree: primitive numbering"; return MTSGPU_EINVAL; }
        if (tg) (*tg)[prim] = H.tris[s];
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k)   // prim_vtx is in global primitive order (only the TriAccel slots are in leaf order)
                P[9 * (size_t)prim + 3 * v + k] = H.positions[3 * (size_t)H.prim_vtx[4 * (size_t)prim + v] + k];
    }
    if (!mtsg_build_kdtree(P.data(), (uint32_t)prims, kd, true)) {
        err = "kd-tree: a child offset exceeds KDNode's 28-bit relative field (indirection nodes are not supported)";
        return MTSGPU_EINVAL;
    }
    return MTSGPU_OK;
}

void kd_export(const KdTree &K, uint32_t *nodes, size_t node_cap, uint32_t *indices, size_t index_cap, uint32_t *info8) {
    const uint32_t v[8] = {(uint32_t)(K.nodes.size() / 2), (uint32_t)K.indices.size(), K.stats.inner, K.stats.leaves,
                           K.stats.nonempty_leaves, K.stats.retracted, K.stats.pruned, K.stats.max_depth};
    std::memcpy(info8, v, sizeof v);
    if (nodes && node_cap >= K.nodes.size()) std::memcpy(nodes, K.nodes.data(), K.nodes.size() * 4);
    if (indices && index_cap >= K.indices.size()) std::memcpy(indices, K.indices.data(), K.indices.size() * 4);
}

int ensure_kdtree(mtsgpu_ctx *ctx) {
    if (ctx->kd_built) return MTSGPU_OK;
    std::vector<MtsgTri> tg;
    std::string err;
    int rc = build_kd_host(ctx->host, ctx->kd, &tg, err);
    if (rc) return fail(ctx, rc, err);
    (void)hipSetDevice(ctx->device);
    hipError_t e;
    // the TriAccel records in leaf-list order (one per primitive reference), so a
    // leaf's records are read without the indices[e] -> record dependence
    if (ctx->kd.nodes.size() / 2 >= (1u << 30)) return fail(ctx, MTSGPU_EINVAL, "kd-tree: more than 2^30 nodes");
    std::vector<MtsgTri> lt(ctx->kd.indices.size());
    for (size_t i = 0; i < lt.size(); ++i) lt[i] = tg[ctx->kd.indices[i]];
    lt.push_back(MtsgTri{});   // one record past the last entry (reading ahead in the leaf loop lost 1-3%, r05)
    if ((e = upload(ctx->kd_nodes, ctx->kd.nodes, ctx->stream)) != hipSuccess ||
        (e = upload(ctx->kd_indices, ctx->kd.indices, ctx->stream)) != hipSuccess ||
        (e = upload(ctx->kd_tris, lt, ctx->stream)) != hipSuccess || (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        return hip_fail(ctx, e, "kd-tree upload");
    ctx->kd_built = true;
    return MTSGPU_OK;
}
}  // namespace

int mtsgpu_trace_rays(mtsgpu_ctx *ctx, const float *rays, uint32_t n, int shadow, float *hits, double *kernel_ms) {
    return mtsgpu_trace_rays_ex(ctx, rays, n, shadow ? MTSGPU_TRACE_SHADOW : 0u, hits, kernel_ms);
}

int mtsgpu_debug_kdtree(mtsgpu_ctx *ctx, uint32_t *nodes, size_t node_cap, uint32_t *indices, size_t index_cap,
                        uint32_t *info8) {
    if (!ctx || !info8) return MTSGPU_EINVAL;
    if (!ctx->have_scene) return fail(ctx, MTSGPU_ESTATE, "debug_kdtree before upload_scene");
    int rc = ensure_kdtree(ctx);
    if (rc) return rc;
    kd_export(ctx->kd, nodes, node_cap, indices, index_cap, info8);
    return MTSGPU_OK;
}

int mtsgpu_bvh_host(const mtsgpu_scene_desc *scene, uint32_t *nodes, size_t node_cap, uint32_t *hnodes,
                    size_t hnode_cap, uint32_t *qnodes, size_t qnode_cap, uint32_t *info4, char *msg, size_t cap) {
    if (!scene || !info4) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    const int rc = mtsg_configure_scene(scene, H, err);
    if (msg && cap) {
        std::strncpy(msg, err.c_str(), cap - 1);
        msg[cap - 1] = 0;
    }
    if (rc) return rc;
    mtsg_build_qnodes(H);
    info4[0] = (uint32_t)H.nodes.size();
    info4[1] = (uint32_t)H.hnodes.size();
    info4[2] = (uint32_t)H.qnodes.size();
    info4[3] = H.qnode_depth;
    if (nodes && node_cap >= H.nodes.size() * 16) std::memcpy(nodes, H.nodes.data(), H.nodes.size() * 64);
    if (hnodes && hnode_cap >= H.hnodes.size() * 8) std::memcpy(hnodes, H.hnodes.data(), H.hnodes.size() * 32);
    if (qnodes && qnode_cap >= H.qnodes.size() * 16) std::memcpy(qnodes, H.qnodes.data(), H.qnodes.size() * 64);
    return MTSGPU_OK;
}

int mtsgpu_scan_host(const mtsgpu_scene_desc *scene, float *records, size_t cap, uint32_t counts[12]) {
    if (!scene || !counts) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    const int rc = mtsg_configure_scene(scene, H, err);
    if (rc) return rc;
    for (int i = 0; i < 12; ++i) counts[i] = 0;
    if (H.tris.size() > MTSG_SCAN_MAX || !H.analytic.empty()) return MTSGPU_OK;   // not a scan scene
    std::vector<MtsgTri> g;
    mtsg_scan_layout(H.tris, g, counts, counts + 6);
    if (records && cap >= g.size() * 12) std::memcpy(records, g.data(), g.size() * sizeof(MtsgTri));
    return MTSGPU_OK;
}

// the per-primitive unit face normals upload_scene forms for LDS scenes (configure_shape.cpp
// mtsg_face_normal), with the vertex positions they were formed from (9 floats per primitive)
int mtsgpu_face_normals_host(const mtsgpu_scene_desc *scene, float *normals, float *corners, size_t prim_cap,
                             uint32_t *num_prims) {
    if (!scene || !num_prims) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    const int rc = mtsg_configure_scene(scene, H, err);
    if (rc) return rc;
    const size_t n = H.face_n.size() / 3;
    *num_prims = (uint32_t)n;
    if (!normals || !corners || prim_cap < n) return MTSGPU_OK;
    std::memcpy(normals, H.face_n.data(), n * 3 * sizeof(float));
    for (size_t p = 0; p < n; ++p)
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k)
                corners[9 * p + 3 * v + k] = H.positions[3 * (size_t)H.prim_vtx[4 * p + v] + k];
    return MTSGPU_OK;
}

// geom = {x0, y0, width, height, row_block, row_stride, row_phase, tile_shard, chunk_spp,
// round_shift, lanes}: the launch's index constants as a render forms them (render_plan.cpp
// launch_geometry, layout.h mtsg_launch_index), then for each
// (lane, round) the megakernel's own stepping (layout.h mtsg_run_init / mtsg_run_step, pixel_of)
int mtsgpu_index_host(const uint32_t geom[11], const uint32_t *lane_round, size_t n, uint32_t *out, uint32_t info2[2]) {
    if (!geom || (n && (!lane_round || !out))) return MTSGPU_EINVAL;
    MtsgLaunch L;
    std::memset(&L, 0, sizeof L);
    launch_geometry(L, geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7] != 0);
    L.chunk_spp = geom[8];
    L.round_shift = geom[9];
    if (!L.num_pixels || !geom[10] || L.round_shift > 6) return MTSGPU_EINVAL;
    mtsg_launch_index(L, geom[10]);
    if (info2) { info2[0] = L.num_pixels; info2[1] = L.tiles_x; }
    for (size_t i = 0; i < n; ++i) {
        const uint32_t g = lane_round[2 * i], target = lane_round[2 * i + 1];
        uint32_t *o = out + 6 * i;
        uint32_t round, pix, jj = 0;
        mtsg_run_init(L, g, round, pix);
        bool more = true;
        for (uint32_t k = 0; k <= target && more; ++k) more = mtsg_run_step(L, round, pix, jj);
        int px = 0, py = 0;
        const bool valid = more && jj < L.chunk_spp && pixel_of(L, pix, px, py);
        o[0] = more ? 1u : 0u;
        o[1] = more ? jj : 0u;
        o[2] = more ? pix : 0u;
        o[3] = valid ? (uint32_t)px : 0u;
        o[4] = valid ? (uint32_t)py : 0u;
        o[5] = valid ? 1u : 0u;
    }
    return MTSGPU_OK;
}

// The plan of a render without a device (include/mtsgpu.h has out[]'s layout): the scene
// configured on the host, the environment read, then the functions render_impl runs
int mtsgpu_plan_host(const mtsgpu_scene_desc *scene, const mtsgpu_render_params *params, uint32_t num_fields,
                     int want_samples, const uint64_t dev[3], uint64_t *out, size_t out_cap, char *msg, size_t msg_cap) {
    if (!scene || !params || !dev || !out || out_cap < 16 || num_fields > MTSGPU_MAX_FIELDS) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    int rc = mtsg_configure_scene(scene, H, err);
    RenderPlan plan;
    const RenderKnobs K = read_knobs();
    if (!rc) {
        std::vector<MtsgTri> g;
        scene_scan_n(H, g, H.launch.scan_n);
        H.launch.one_emitter = scene_one_emitter(H);
        const DeviceFacts facts = {(int)dev[0], (size_t)dev[2], 0};
        rc = plan_render(H, *params, num_fields, want_samples != 0, facts, K, plan, err);
    }
    const MtsgLaunch &L = plan.L;
    const uint64_t launches = rc ? 0 : (L.spp + plan.chunk - 1) / plan.chunk;
    for (uint64_t i = 0; !rc && i < launches; ++i) {
        const LaunchPlan lp = plan_launch(plan, (uint32_t)(i * plan.chunk), dev[1] ? (int)dev[1] : (int)L.waves);
        if (lp.err) { err = lp.err; rc = MTSGPU_EINVAL; break; }
        if (16 + 3 * i + 3 > out_cap) continue;
        out[16 + 3 * i] = lp.chunk_spp;
        out[17 + 3 * i] = (uint64_t)lp.grid;
        out[18 + 3 * i] = lp.round_shift;
    }
    if (msg && msg_cap) std::snprintf(msg, msg_cap, "%s", err.c_str());
    if (rc) return rc;
    const bool wave = plan.engine == MTSG_ENGINE_WAVEFRONT;
    const uint64_t head[16] = {(uint64_t)plan.engine, plan_variant_word(plan), L.num_pixels, plan.chunk, launches, L.waves,
                               L.lds_dims, L.nibbles,
                               L.scene_lds | L.scan << 1 | (mtsg_path_start_queue(L) ? 4u : 0u) | L.gather << 3 | L.replay << 4,
                               L.gather_h, wave ? 0 : mtsg_path_lds_bytes(L), wave ? plan_wavefront(plan, H, K).slots : 0u,
                               0, 0, 0, 0};
    std::memcpy(out, head, sizeof head);
    return MTSGPU_OK;
}

// sobol::look_up for film resolution 2^m through the tables the kernels stage
// (layout.h mtsg_lut_word, sobol_lookup_lds): out[i] = the index of sample j at pixel (px, py)
int mtsgpu_lookup_host(uint32_t m, uint64_t scramble, const uint32_t *px_py_j, size_t n, uint64_t *out) {
    if (m < 1 || m > 16 || (n && (!px_py_j || !out))) return MTSGPU_EINVAL;
    MtsgLookup lut;
    mtsg_sobol_lookup_solve(m, lut);
    uint32_t tab[MTSG_LUT_WORDS];
    for (uint32_t i = 0; i < MTSG_LUT_WORDS; ++i) tab[i] = mtsg_lut_word(lut, i);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t j = px_py_j[3 * i + 2];
        uint32_t indexBits = 0;   // of this sample's index, frame << 2m | 2m bits
        while (indexBits < 64 && (((uint64_t)j << (2 * m)) >> indexBits)) ++indexBits;
        const uint32_t nibbles = sobol_nibbles(indexBits);   // the planner's rule (render_plan.h)
        out[i] = sobol_lookup_lds(lut, (const uint32_t *)tab, nibbles, j, px_py_j[3 * i], px_py_j[3 * i + 1], scramble);
    }
    return MTSGPU_OK;
}

int mtsgpu_kdtree_host(const mtsgpu_scene_desc *scene, uint32_t *nodes, size_t node_cap, uint32_t *indices,
                       size_t index_cap, uint32_t *info8, char *msg, size_t cap) {
    if (!scene || !info8) return MTSGPU_EINVAL;
    HostScene H;
    KdTree K;
    std::string err;
    int rc = mtsg_configure_scene(scene, H, err);
    if (!rc) rc = build_kd_host(H, K, nullptr, err);
    if (msg && cap) {
        std::strncpy(msg, err.c_str(), cap - 1);
        msg[cap - 1] = 0;
    }
    if (!rc) kd_export(K, nodes, node_cap, indices, index_cap, info8);
    return rc;
}

int mtsgpu_trace_rays_ex(mtsgpu_ctx *ctx, const float *rays, uint32_t n, uint32_t flags, float *hits,
                         double *kernel_ms) {
    const int shadow = (flags & MTSGPU_TRACE_SHADOW) ? 1 : 0;
    if (!ctx) return MTSGPU_EINVAL;
    if (!ctx->have_scene) return fail(ctx, MTSGPU_ESTATE, "trace_rays before upload_scene");
    if (!rays || !hits) return fail(ctx, MTSGPU_EINVAL, "trace_rays: NULL buffer");
    if (n == 0) return MTSGPU_OK;
    if (flags & MTSGPU_TRACE_KDTREE) {
        int rc = ensure_kdtree(ctx);
        if (rc) return rc;
    }
    (void)hipSetDevice(ctx->device);
    hipError_t e;
    if ((e = ctx->qrays.ensure((size_t)n * 32)) != hipSuccess || (e = ctx->qhits.ensure((size_t)n * 16)) != hipSuccess)
        return hip_fail(ctx, e, "trace buffers");
    hipStream_t s = ctx->stream;
    if ((e = hipMemcpyAsync(ctx->qrays.p, rays, (size_t)n * 32, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipEventRecord(ctx->ev0, s)) != hipSuccess ||
        (e = (flags & MTSGPU_TRACE_KDTREE)
                 ? mtsg_launch_trace_kd(ctx->dscene, (const uint32_t *)ctx->kd_nodes.p, (const uint32_t *)ctx->kd_indices.p,
                                        (const MtsgTri *)ctx->kd_tris.p, (const float *)ctx->qrays.p, n,
                                        (float *)ctx->qhits.p, shadow != 0, ctx->num_cus, s)
                 : mtsg_launch_trace(ctx->dscene, (const float *)ctx->qrays.p, n, (float *)ctx->qhits.p, shadow != 0,
                                     ctx->host.bvh_depth + 2, ctx->num_cus, s)) != hipSuccess ||
        (e = hipEventRecord(ctx->ev1, s)) != hipSuccess ||
        (e = hipMemcpyAsync(hits, ctx->qhits.p, (size_t)n * 16, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(ctx, e, "trace_rays");
    if (kernel_ms) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        *kernel_ms = ms;
    }
    return MTSGPU_OK;
}

// diagnostics: device arithmetic probe (tests/test_gpu_arith.py)
int mtsgpu_debug_arith(mtsgpu_ctx *ctx, const float *a, const float *b, float *out, int n) {
    if (!ctx || n <= 0) return MTSGPU_EINVAL;
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    hipError_t e;
    if ((e = hipMalloc(&da, n * 4)) != hipSuccess || (e = hipMalloc(&db, n * 4)) != hipSuccess ||
        (e = hipMalloc(&dout, (size_t)n * 32)) != hipSuccess)
        return hip_fail(ctx, e, "malloc");
    (void)hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice);
    e = mtsg_launch_arith_probe(da, db, dout, n, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 32, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return e == hipSuccess ? MTSGPU_OK : hip_fail(ctx, e, "arith probe");
}

// diagnostics: the device's transcendentals over inputs (tests/test_gpu_libm.py)
int mtsgpu_debug_libm(mtsgpu_ctx *ctx, int fn, const float *a, const float *b, float *out, size_t n,
                      uint32_t first) {
    if (!ctx || !out || n == 0 || fn < 0 || fn > 9 || ((fn == 6 || fn == 7) && a && !b)) return MTSGPU_EINVAL;
    (void)hipSetDevice(ctx->device);
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&dout, n * 4);
    if (e == hipSuccess && a) e = hipMalloc(&da, n * 4);
    if (e == hipSuccess && b) e = hipMalloc(&db, n * 4);
    if (e == hipSuccess && a) e = hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && b) e = hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mtsg_launch_libm_probe(fn, da, db, dout, n, first, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost);
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    return e == hipSuccess ? MTSGPU_OK : hip_fail(ctx, e, "libm probe");
}

// diagnostics: n nextULong draws of the device's SFMT19937 from Random(seed), or
// from its clone-th Random(&master) clone (host seeding, device generation)
int mtsgpu_debug_sfmt(mtsgpu_ctx *ctx, uint64_t seed, int clone, uint64_t *out, int n) {
    if (!ctx || !out || n <= 0 || clone < 0) return MTSGPU_EINVAL;
    std::vector<uint32_t> master(MTSG_SFMT_WORDS, 0u), child(MTSG_SFMT_WORDS, 0u);
    mtsg_sfmt_seed(master.data(), seed);
    for (int k = 0; k < clone; ++k) mtsg_sfmt_clone(child.data(), master.data());
    const std::vector<uint32_t> &st = clone > 0 ? child : master;
    uint32_t *dw = nullptr;
    unsigned long long *dout = nullptr;
    hipError_t e;
    (void)hipSetDevice(ctx->device);
    if ((e = hipMalloc(&dw, MTSG_SFMT_WORDS * 4)) != hipSuccess || (e = hipMalloc(&dout, (size_t)n * 8)) != hipSuccess) {
        if (dw) (void)hipFree(dw);
        return hip_fail(ctx, e, "malloc");
    }
    e = hipMemcpy(dw, st.data(), MTSG_SFMT_WORDS * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mtsg_launch_sfmt_probe(dw, dout, n, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(dw);
    (void)hipFree(dout);
    return e == hipSuccess ? MTSGPU_OK : hip_fail(ctx, e, "sfmt probe");
}

int mtsgpu_debug_counters(mtsgpu_ctx *ctx, uint64_t *out16) {
    if (!ctx || !out16) return MTSGPU_EINVAL;
    for (int k = 0; k < 16; ++k) out16[k] = ctx->last_counters[k];
    return MTSGPU_OK;
}

// diagnostics: BVH statistics of the uploaded scene
int mtsgpu_debug_scene_info(mtsgpu_ctx *ctx, uint32_t *info4) {
    if (!ctx || !ctx->have_scene || !info4) return MTSGPU_EINVAL;
    info4[0] = (uint32_t)ctx->host.nodes.size();
    info4[1] = (uint32_t)ctx->host.tris.size();
    info4[2] = ctx->host.bvh_depth;
    info4[3] = (uint32_t)ctx->num_cus;
    return MTSGPU_OK;
}

// diagnostics: host-side environment tables (tests/test_host_configure.py)
int mtsgpu_debug_env_tables(const mtsgpu_scene_desc *scene, float *params, uint16_t *texels, size_t texel_cap,
                            float *rows, float *cols, float *weights) {
    HostScene H;
    std::string err;
    const int rc = mtsg_configure_scene(scene, H, err);
    if (rc) { g_create_error = err; return rc; }
    const MtsgEnv &E = H.env;
    if (E.emitter < 0) { g_create_error = "scene has no environment emitter"; return MTSGPU_EINVAL; }
    if (params) {
        std::memset(params, 0, 64 * sizeof(float));
        params[0] = (float)E.levels; params[1] = (float)E.w0; params[2] = (float)E.h0;
        params[3] = E.normalization; params[4] = E.pixel_x; params[5] = E.pixel_y; params[6] = E.scale;
        params[7] = E.center[0]; params[8] = E.center[1]; params[9] = E.center[2]; params[10] = E.radius;
        params[11] = (float)(H.env_texels.size() / 4);
        for (int l = 0; l < E.levels && l < MTSG_ENV_MAX_LEVELS; ++l) { params[16 + l] = (float)E.lw[l]; params[34 + l] = (float)E.lh[l]; }
    }
    if (texels) {
        if (texel_cap < H.env_texels.size()) return MTSGPU_EINVAL;
        std::memcpy(texels, H.env_texels.data(), H.env_texels.size() * sizeof(uint16_t));
    }
    if (rows) std::memcpy(rows, H.env_cdf_rows.data(), H.env_cdf_rows.size() * sizeof(float));
    if (cols) std::memcpy(cols, H.env_cdf_cols.data(), H.env_cdf_cols.size() * sizeof(float));
    if (weights) std::memcpy(weights, H.env_row_weights.data(), H.env_row_weights.size() * sizeof(float));
    return MTSGPU_OK;
}

// diagnostics: one hash per member of the configured scene (tests/test_scene_digest_host.py)
static uint64_t fnv1a(const void *p, size_t bytes, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int mtsgpu_scene_digest_host(const mtsgpu_scene_desc *scene, uint64_t *out, size_t cap, uint32_t *n, char *msg,
                             size_t msg_cap) {
    if (!scene || !n) return MTSGPU_EINVAL;
    HostScene H;
    std::string err;
    const int rc = mtsg_configure_scene(scene, H, err);
    if (msg && msg_cap) {
        std::strncpy(msg, err.c_str(), msg_cap - 1);
        msg[msg_cap - 1] = 0;
    }
    if (rc) return rc;
    auto vec = [](const auto &v) { return fnv1a(v.data(), v.size() * sizeof(v[0])); };
    const unsigned char ext = H.ext ? 1 : 0;
    uint64_t env = fnv1a(&H.env, offsetof(MtsgEnv, texels));
    env = fnv1a(&H.env.guide_rbits, sizeof H.env.guide_rbits, env);
    env = fnv1a(&H.env.guide_cbits, sizeof H.env.guide_cbits, env);
    const uint64_t d[] = {
        vec(H.nodes), vec(H.hnodes), vec(H.tris), vec(H.prim_vtx), vec(H.dpdu), vec(H.positions),
        vec(H.normals), vec(H.face_n), vec(H.shapes), vec(H.bsdfs), vec(H.emitters), vec(H.deltas),
        vec(H.area_cdf), vec(H.em_cdf), fnv1a(&H.em_norm, sizeof H.em_norm),
        fnv1a(H.aabb_min, sizeof H.aabb_min), fnv1a(H.aabb_max, sizeof H.aabb_max), fnv1a(&H.cam, sizeof H.cam),
        fnv1a(&H.cam_lens, sizeof H.cam_lens), fnv1a(&H.film_w, sizeof H.film_w), fnv1a(&H.film_h, sizeof H.film_h),
        fnv1a(&H.bvh_depth, sizeof H.bvh_depth), env, vec(H.env_texels), vec(H.env_cdf_rows),
        vec(H.env_cdf_cols), vec(H.env_row_weights), vec(H.env_guide_rows), vec(H.env_guide_cols),
        vec(H.rtrans), vec(H.texcoords), fnv1a(&ext, 1), vec(H.analytic)};
    *n = (uint32_t)(sizeof d / sizeof d[0]);
    if (!out || cap < *n) return MTSGPU_EINVAL;
    std::memcpy(out, d, sizeof d);
    return MTSGPU_OK;
}

}  // extern "C"
