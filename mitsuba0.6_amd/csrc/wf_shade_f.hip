// wf_shade_f.hip -- the wavefront engine's shade kernels (wf_impl.h) for one
// scene feature set WF_FEAT (MTSG_FEAT_ENV | EXT | ANA bits), built once per
// set by the Makefile (-DWF_FEAT=n -> wf_shade_f<n>.o)
#include "wf_impl.h"
#include "launchers.h"

static_assert(mtsg_is_feat_set(WF_FEAT), "-DWF_FEAT names a set of layout.h's MTSG_FEAT_SETS");
#define MTSG_WF_PICK_NAME2(N) mtsg_wf_pick_##N
#define MTSG_WF_PICK_NAME(N) MTSG_WF_PICK_NAME2(N)
#define MTSG_WF_BYTES_NAME2(N) mtsg_launch_bytes_wf_shade_f##N
#define MTSG_WF_BYTES_NAME(N) MTSG_WF_BYTES_NAME2(N)
// this object's view of the launch record (capi.cpp launch_layout_error)
extern "C" uint32_t MTSG_WF_BYTES_NAME(WF_FEAT)() { return (uint32_t)sizeof(MtsgLaunch); }
WfShadeFn MTSG_WF_PICK_NAME(WF_FEAT)(int wk, bool instr, bool ggx) { return wf_shade_pick_f<WF_FEAT>(wk, instr, ggx); }
