// launchers.h -- the host-side launchers of libmtsgpu.so's kernels: each is defined in the
// .hip file that holds its kernels and called from capi.cpp, group.cpp and render_plan.cpp.
// The defining files include this header too, so a declaration cannot drift from its
// definition unnoticed (an overload nobody defines fails the link).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mtsgpu.h"
#include "layout.h"

// ---- the megakernel and the film kernels (path_kernel.hip, path_f.hip) ----
typedef void (*PathKernelFn)(MtsgLaunch);
hipError_t mtsg_launch_path(const MtsgLaunch &L, int grid, bool samples, bool stats, hipStream_t stream);
int mtsg_path_kernel_occupancy(const MtsgLaunch &L, int *blocksPerCU);
int mtsg_path_features(const MtsgLaunch &L);   // the scene's MTSG_FEAT_ENV | EXT | ANA bits, or MTSG_FEAT_SET_DELTA / _LENS / _COMBO
int mtsg_path_variant(const MtsgLaunch &L);    // the FEAT template argument mtsg_launch_path runs
size_t mtsg_path_lds_bytes(const MtsgLaunch &L);   // dynamic LDS of the megakernel, direct_kernel and field_kernel
bool mtsg_path_start_queue(const MtsgLaunch &L);   // the launch starts its paths from the LDS queue (dpath.h mtsg_start_queue)
// one object per scene feature set: the megakernel instantiation for L, BSDF-set bits `bits`
#define MTSG_PATH_F_DECL(N) PathKernelFn mtsg_path_pick_f##N(const MtsgLaunch &L, int bits, bool instr);
MTSG_FEAT_SETS(MTSG_PATH_F_DECL)   // (layout.h)
#undef MTSG_PATH_F_DECL
hipError_t mtsg_launch_gather(const MtsgLaunch &L, hipStream_t stream);
hipError_t mtsg_launch_reduce(const MtsgLaunch &L, hipStream_t stream);
hipError_t mtsg_launch_finalize(float *own, const double *spill, size_t n, hipStream_t stream);
hipError_t mtsg_launch_trace(const MtsgDeviceScene &S, const float *rays, uint32_t n, float *out, bool shadow,
                             uint32_t stackDepth, int numCUs, hipStream_t stream);
hipError_t mtsg_launch_trace_kd(const MtsgDeviceScene &S, const uint32_t *kdNodes, const uint32_t *kdIndices,
                                const MtsgTri *kdTris, const float *rays, uint32_t n, float *out, bool shadow,
                                int numCUs, hipStream_t stream);
hipError_t mtsg_launch_arith_probe(const float *a, const float *b, float *out, int n, hipStream_t stream);
hipError_t mtsg_launch_sfmt_probe(uint32_t *w, unsigned long long *out, int n, hipStream_t s);

// ---- the field pass (field_kernel.hip) ----
hipError_t mtsg_launch_field(const MtsgLaunch &L, const MtsgFieldArgs &FA, int grid, hipStream_t stream);
int mtsg_field_occupancy(const MtsgLaunch &L, int *bpc);

// ---- the wavefront engine (wf_kernel.hip; its shade kernels: wf_shade_f.hip) ----
hipError_t mtsg_launch_wf_shade(const MtsgLaunch &L, const MtsgWave &W, unsigned long long *part, int grid, int wk,
                                bool ggx, bool instr, hipStream_t s);
hipError_t mtsg_launch_wf_trace(const MtsgLaunch &L, const MtsgWave &W, unsigned long long *part, int grid,
                                bool stats, hipStream_t s);
hipError_t mtsg_launch_wf_flush(const unsigned long long *part, uint32_t blocks, unsigned long long *counters,
                                hipStream_t s);
int mtsg_wf_occupancy(const MtsgLaunch &L, int wk, bool ggx, int *shadeBpc, int *traceBpc);
size_t mtsg_wf_shade_lds_bytes(const MtsgLaunch &L);
size_t mtsg_wf_trace_lds_bytes(const MtsgLaunch &L);

// ---- film develop (film_kernel.hip, ldrfilm_kernel.hip) and the libm probe (probe_kernel.hip) ----
hipError_t mtsg_launch_develop(const mtsgpu_develop_params &P, const float *film, void *out, int num_cus,
                               hipStream_t s);
hipError_t mtsg_launch_develop_multi(const mtsgpu_develop_multi_params &P, const float *const *films, void *out,
                                     int num_cus, hipStream_t s);
int mtsg_develop_channels(int pixel_format);
hipError_t mtsg_launch_film_accumulate(float *dst, const float *src, size_t n, int num_cus, hipStream_t s);
hipError_t mtsg_launch_develop_ldr(const mtsgpu_develop_ldr_params &P, const float *film, uint8_t *out, void *scratch,
                                   int num_cus, hipStream_t s);
size_t mtsg_develop_ldr_scratch(const mtsgpu_develop_ldr_params &P);
size_t mtsg_develop_ldr_info_offset();
hipError_t mtsg_launch_libm_probe(int fn, const float *a, const float *b, float *out, size_t n, uint32_t first,
                                  hipStream_t s);

// Every object that takes an MtsgLaunch by value reports the size it was compiled with
// (capi.cpp launch_layout_error).
extern "C" {
uint32_t mtsg_launch_bytes_path_kernel();
uint32_t mtsg_launch_bytes_wf_kernel();
uint32_t mtsg_launch_bytes_field_kernel();
#define MTSG_BYTES_DECL(N) uint32_t mtsg_launch_bytes_path_f##N(); uint32_t mtsg_launch_bytes_wf_shade_f##N();
MTSG_FEAT_SETS(MTSG_BYTES_DECL)
#undef MTSG_BYTES_DECL
}
