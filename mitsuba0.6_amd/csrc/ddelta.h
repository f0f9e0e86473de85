// ddelta.h -- device side of the delta emitters: point, spot, directional.
//
//   PointEmitter::sampleDirect        emitters/point.cpp:131-147
//   SpotEmitter::sampleDirect         emitters/spot.cpp:184-200, falloffCurve :105-125
//                                     (constant texture: `result` is Spectrum(1))
//   DirectionalEmitter::sampleDirect  emitters/directional.cpp:159-180
//
// One NEE candidate each: dRec.pdf = 1, dRec.measure = EDiscrete.  No ray hits
// them, so they have no pdfDirect partner and no emitted-radiance term; the
// integrators weight their estimate with bsdfPdf = 0 (path.cpp:192-197,
// direct.cpp:235, volpath.cpp: emitter->isOnSurface() is false).  Per-emitter
// constants come from the host (configure_emitter.cpp configure_delta,
// directional_bsphere) in an MtsgDelta record.
#pragma once
#include "dmath.h"
#include "layout.h"

typedef const __attribute__((address_space(1))) MtsgDelta GDelta;

// value: the returned Spectrum; d, dist: dRec.d, dRec.dist; p: dRec.p; pdf: dRec.pdf
struct DeltaSample { f3 value, d, p; float dist, pdf; };

__device__ __forceinline__ DeltaSample point_sample_direct(GDelta &e, f3 intensity, f3 ref) {
    DeltaSample r;
    r.p = mk(e.pos[0], e.pos[1], e.pos[2]);
    r.d = sub(r.p, ref);
    r.dist = dsqrt(len2(r.d));
    const float invDist = 1.0f / r.dist;
    r.d = mul(r.d, invDist);
    r.pdf = 1.0f;
    r.value = mul(intensity, invDist * invDist);
    return r;
}

__device__ __forceinline__ DeltaSample spot_sample_direct(GDelta &e, f3 intensity, f3 ref) {
    DeltaSample r;
    r.p = mk(e.pos[0], e.pos[1], e.pos[2]);
    r.d = sub(r.p, ref);
    r.dist = dsqrt(len2(r.d));
    const float invDist = 1.0f / r.dist;
    r.d = mul(r.d, invDist);
    r.pdf = 1.0f;
    // falloffCurve(trafo.inverse()(-dRec.d)): Frame::cosTheta of the local direction
    const f3 nd = neg(r.d);
    const float cosTheta = e.to_local[6] * nd.x + e.to_local[7] * nd.y + e.to_local[8] * nd.z;
    f3 fall = mk(1.0f, 1.0f, 1.0f);
    if (cosTheta <= e.cos_cutoff) fall = mk(0.0f, 0.0f, 0.0f);
    else if (!(cosTheta >= e.cos_beam)) fall = mul(fall, (e.cutoff - d_acos(cosTheta)) * e.inv_transition);
    r.value = mul(mulv(intensity, fall), invDist * invDist);
    return r;
}

__device__ __forceinline__ DeltaSample directional_sample_direct(GDelta &e, f3 irradiance, f3 ref) {
    DeltaSample r;
    const f3 d = mk(e.dir[0], e.dir[1], e.dir[2]);
    const f3 diskCenter = mk(e.pos[0], e.pos[1], e.pos[2]);
    const float distance = dot(sub(ref, diskCenter), d);
    r.value = mk(0.0f, 0.0f, 0.0f);
    r.d = neg(d);
    r.p = ref;
    r.dist = 0.0f;
    // distance < 0: the reference returns zero before it fills the record; no estimate
    r.pdf = 0.0f;
    if (!(distance < 0)) {
        r.p = sub(ref, mul(d, distance));
        r.dist = distance;
        r.pdf = 1.0f;
        r.value = irradiance;
    }
    return r;
}

// sampleDirect of delta emitter record `e` of type `type` (MTSG_EMITTER_POINT / SPOT / DIRECTIONAL)
__device__ __forceinline__ DeltaSample delta_sample_direct(int type, GDelta &e, f3 radiance, f3 ref) {
    if (type == MTSG_EMITTER_POINT) return point_sample_direct(e, radiance, ref);
    if (type == MTSG_EMITTER_SPOT) return spot_sample_direct(e, radiance, ref);
    return directional_sample_direct(e, radiance, ref);
}
