// scene_build.cpp -- host configure() for the MI355X path integrator.
//
// Derives, from the scene description of include/mtsgpu.h, everything the
// reference computes in its configure()/initialize() steps, then lays it out
// for HBM (layout.h).  One unit per subsystem of the reference, each with its
// source-line citations; the stages below are declared in scene_build_impl.h:
//   camera                  configure_sensor.cpp
//   BSDFs, default BSDFs    configure_bsdf.cpp
//   emitters, emitter PDF,  configure_emitter.cpp
//   scene bounds
//   meshes, TriAccel,       configure_shape.cpp
//   analytic shapes
//   BVH                     bvh_build.cpp
// Beside them, not part of a scene's configure: sobol_host.cpp (the sampler's
// tables) and configure_filter.cpp (the reconstruction filter).
#include "scene_build_impl.h"

int mtsg_configure_scene(const mtsgpu_scene_desc *D, HostScene &S, std::string &err) {
    using namespace mtsg_host;
    if (!D) { err = "null scene"; return MTSGPU_EINVAL; }
    S = HostScene();
    std::memset(&S.env, 0, sizeof S.env);
    S.env.emitter = -1;
    SceneBuild B;
    int rc;
    if ((rc = configure_sensor(D->sensor, S, err))) return rc;
    if ((rc = configure_bsdfs(*D, S, err))) return rc;      // with twosided, `ext` and the two defaults
    if ((rc = configure_emitters(*D, S, err))) return rc;
    if ((rc = configure_shapes(*D, S, B, err))) return rc;
    emitter_cdf(S);
    scene_bounds(*D, B, S);                                 // and the emitters' bounding spheres
    return build_bvh(B, S, err);                            // with the triangles in leaf order
}
