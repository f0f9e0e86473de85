// render_plan.h -- what a render will launch, decided on the host without a device.
//
// A render is three things: what was asked (mtsgpu_render_params, the field list), what
// will be launched (this file: plan_render, plan_launch, plan_wavefront), and launching it
// (capi.cpp render_impl).  The planner is plain host code and makes no HIP call, so
// mtsgpu_plan_host runs the very functions render_impl runs (tests/test_plan_host.py).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mtsgpu.h"
#include "layout.h"
#include "scene_build.h"

// The MTSGPU_* environment switches of a render, read once per render (read_knobs): the
// tests and the A/B tools set them between renders of one process.
// (MTSGPU_NO_SCAN_PAIRS is read at upload: mtsg_scan_layout.)
struct RenderKnobs {
    bool wf_hitrec;               // MTSGPU_WF_HITREC=1: the wavefront's trace kernel forms the whole hit record (A/B in DESIGN.md 4)
    uint32_t wf_shade_lds_dims;   // MTSGPU_WF_SHADE_LDS_DIMS caps the Sobol dimensions the shade kernels stage in LDS
                                  // (0: every dimension from HBM/L2); unset: no cap (~0u)
    bool wf_generic;              // MTSGPU_WF_GENERIC: A/B: every hit through the generic kernel
    int round_shift;              // MTSGPU_ROUND_SHIFT=s overrides run_shift (A/B), clamped to 0..6; unset: -1
    bool no_one_emitter;          // MTSGPU_NO_ONE_EMITTER: MtsgLaunch::one_emitter stays 0
    bool no_scene_lds;            // MTSGPU_NO_SCENE_LDS: small scenes are not staged in LDS
    bool no_scan;                 // MTSGPU_NO_SCAN: tiny scenes traverse their BVH (and take no start queue)
    bool no_diff_variant;         // MTSGPU_NO_DIFF_VARIANT: all-diffuse scenes take the generic kernel
    bool no_tiny_set;             // MTSGPU_NO_TINY_SET: the all-diffuse LDS scenes' megakernel launches take the generic
                                  // kernel, as those outside the tiny set do (A/B and tests)
    bool no_bsdf_sets;            // MTSGPU_NO_BSDF_SETS: large scenes take the generic kernel
    bool no_refn_spec;            // MTSGPU_NO_REFN_SPEC: envmap-only scenes keep refN (no MTSG_FEAT_NOREFN)
    uint32_t waves;               // MTSGPU_WAVES: 4 for "4", else 3; unset: 0 (the plan decides)
    bool no_gather;               // MTSGPU_NO_GATHER: wide filters splat with atomics
    int sobol_lds_dims;           // MTSGPU_SOBOL_LDS_DIMS: Sobol dimensions staged in LDS, clamped to 0..1024; unset: -1
    size_t contrib_bytes;         // MTSGPU_CONTRIB_BYTES: the record-buffer budget, at least 1 MiB; unset: 0
    bool engine_wavefront;        // MTSGPU_ENGINE=wavefront (any other value: the megakernel)
    uint64_t wf_slots;            // MTSGPU_WF_SLOTS: the wavefront's path slots, at least 1; unset: 0 (about 2M)
};
RenderKnobs read_knobs();

struct DeviceFacts {
    int num_cus;
    size_t free_bytes;     // hipMemGetInfo's free bytes; 0: unknown
    size_t contrib_held;   // bytes of the record buffer the context already holds
};

enum { MTSG_ENGINE_MEGAKERNEL = 0, MTSG_ENGINE_WAVEFRONT = 1, MTSG_ENGINE_FIELDS = 2 };

struct RenderPlan {
    MtsgLaunch L;          // every non-pointer field; the pointers are null (render_impl patches them in)
    int engine;            // MTSG_ENGINE_*
    bool replay;           // an SFMT replay sampler: L.units, L.order, L.unit_start, L.sfmt come from replay_host.cpp
    bool kdtree;           // MTSGPU_FLAG_KDTREE: the wavefront engine over the reference's kd-tree
    bool instr;            // the instrumented kernels (per-sample records or traversal statistics)
    bool stats_mode;       // MTSGPU_FLAG_TRAVERSAL_STATS
    uint32_t films;        // 1, or the fields of a field pass
    uint32_t chunk;        // samples per pixel of a launch (the last launch may have fewer)
    size_t filmFloats;     // floats of one film
    size_t fieldBytes;     // bytes of one film's record array
    size_t recFloats;      // floats of a per-sample record
    size_t nsamp;          // floats of all per-sample records; 0: none wanted
    float world_to_cam[16];   // field pass: the sensor's world transform inverted
    int num_cus;
    int round_shift_knob;  // RenderKnobs::round_shift
};

// One launch of the chunk loop (megakernel, field pass) or one chunk of the wavefront engine
struct LaunchPlan {
    uint32_t chunk_spp;
    uint64_t num_items;
    int grid;               // megakernel / field kernel blocks; 0: the wavefront engine (WfPlan has its grids)
    uint32_t round_shift;
    const char *err;        // null, or why the launch cannot run (MTSGPU_EINVAL)
};

// The wavefront engine's launch plan: the shade kinds the scene's shapes can
// reach (the MISS kind always), each kernel's grid, the trace grid, the slots,
// and the sizes of its queues: the buffers are sized and addressed by the same numbers
struct WfPlan {
    bool kinds[MTSG_WK_KINDS] = {};
    bool ggx[MTSG_WK_KINDS] = {};
    int shadeGrid[MTSG_WK_KINDS] = {};
    int traceGrid = 0;
    uint32_t slots = 0;
    bool hitrec = false;       // wf_trace forms the hit records (MtsgWave::hitrec)
    bool hitrecUv = false;     // textured scene: the records carry UVs (MtsgWave::hitrec_uv)
    size_t cap = 0, capCls = 0;   // entries per region of a ray queue / of a kind queue (wf_caps)
    size_t ovfDepth = 0;       // traversal stack entries per trace lane beyond the LDS stack
    int partBlocks = 0;        // blocks of the largest grid: rows of the per-block partial counters
    uint32_t shadeLdsDims = 0; // MtsgLaunch::lds_dims of the shade kernels' launch record
    std::vector<uint32_t> shapeKind;   // shape -> shade kind (wf_kinds)
};

// today's parameter checks with the reference's error texts, then every launch decision;
// num_fields 0: a radiance render.  Returns MTSGPU_OK or the error code, `err` its text.
int plan_render(const HostScene &H, const mtsgpu_render_params &P, uint32_t num_fields, bool want_samples,
                const DeviceFacts &dev, const RenderKnobs &K, RenderPlan &plan, std::string &err);
// the launch that starts at sample j0 of every pixel; blocks_per_cu: the kernel's resident blocks
LaunchPlan plan_launch(const RenderPlan &plan, uint32_t j0, int blocks_per_cu);
WfPlan plan_wavefront(const RenderPlan &plan, const HostScene &H, const RenderKnobs &K);
// the word debug counter 15 gets: which kernel runs (include/mtsgpu.h)
uint64_t plan_variant_word(const RenderPlan &plan);

uint32_t run_shift(const MtsgLaunch &L, uint64_t lanes, int knob);
void launch_geometry(MtsgLaunch &L, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t row_block,
                     uint32_t row_stride, uint32_t row_phase, bool tile_shard);
// Sobol direction-number nibbles a sample index of `indexBits` bits needs: 8 while it fits 32 bits
inline uint32_t sobol_nibbles(uint32_t indexBits) { return indexBits <= 32 ? 8u : (uint32_t)MTSG_NIBBLES; }

// Launch constants of a scene, HostScene::launch (mtsgpu_upload_scene and mtsgpu_plan_host form them)
// g: the tiny-scene scan's copy of `tris`, grouped and paired; a copy's -0 n_u / n_v is +0 where
// n_d != 0 (-DMTSG_SCAN_ZERO_SIGN=0: copied as they are), which no scan can tell (render_plan.cpp)
void mtsg_scan_layout(const std::vector<MtsgTri> &tris, std::vector<MtsgTri> &g, uint32_t n[6], uint32_t np[6]);
// the scan's grouped records `g` (empty: not a scan scene) and their packed counts
void scene_scan_n(const HostScene &H, std::vector<MtsgTri> &g, uint32_t scan_n[6]);
uint32_t scene_one_emitter(const HostScene &H);
// the scalar fields of MtsgDeviceScene (mtsg_path_features and mtsg_path_lds_bytes read them)
void scene_scalars(const HostScene &H, MtsgDeviceScene &D);

// replay_host.cpp -- the `independent` sampler replay (MTSGPU_SAMPLER_SFMT_*): stream seeding
// and the reference's render order
void mtsg_sfmt_seed(uint32_t *w, uint64_t seed);
void mtsg_sfmt_clone(uint32_t *w, uint32_t *parent);
void mtsg_render_order(uint32_t width, uint32_t height, uint32_t bs, std::vector<uint32_t> &order,
                       std::vector<uint32_t> &blockStart);
// the replay's three uploads for a width x height crop: pixels in render order, the units'
// first pixels (one unit, or one per 32x32 block), one SFMT stream per unit
void mtsg_replay_tables(uint32_t width, uint32_t height, bool per_block, std::vector<uint32_t> &order,
                        std::vector<uint32_t> &unitStart, std::vector<uint32_t> &streams);
