// dsensor.h -- the primary ray of the projective sensors (src/sensors/perspective.cpp,
// thinlens.cpp, orthographic.cpp, telecentric.cpp: sampleRayDifferential), the single
// source of the camera ray of every kernel: PathShader::produce (the megakernel and the
// wavefront engine), direct_kernel and field_kernel, and of the differential directions
// the environment lookup of a missed camera ray takes.  `perspective` has its own
// functions (pinhole_*, camera_ray), which every kernel but the MTSG_FEAT_LENS ones runs;
// those run sensor_ray / sensor_ray_diff.  (The pinhole's differentials stay written out in
// PathShader::shade and path_kernel.hip's env_camera: through a shared function either
// caller compiled to other code.)
//
// The sensor type is a run-time field (MtsgCameraLens, MtsgLaunch::cam_lens).  `thinlens` and `telecentric` set
// ENeedsApertureSample: renderBlock (integrator.cpp:165-186) draws rRec.nextSample2D() for
// them after the sample position and before Li -- sensor_needs_aperture; the caller draws
// (ax, ay) and every later sampler dimension of the sample moves by two.  There is no time
// sample (shutterOpen == shutterClose).
//
// Included by dpath.h; the disk warp is danalytic.h's, its sincosf glibc's.
#pragma once

__device__ __forceinline__ f3 xf_point(const float *m, f3 p) {         // transform.h:108-125
    float x = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    float y = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    float z = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    float w = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    if (w == 1.0f) return mk(x, y, z);
    return divs(mk(x, y, z), w);
}

__device__ __forceinline__ bool sensor_needs_aperture(const MtsgCameraLens &ln) {
    return ln.type == MTSG_SENSOR_THINLENS || ln.type == MTSG_SENSOR_TELECENTRIC;
}

// Transform::transformAffine(Point) (transform.h:108-121): no division by w
__device__ __forceinline__ f3 xf_affine(const float *m, f3 p) {
    return mk(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
              m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
// Transform::operator()(Vector) (transform.h:175-183)
__device__ __forceinline__ f3 xf_vector(const float *m, f3 v) {
    return mk(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z,
              m[8] * v.x + m[9] * v.y + m[10] * v.z);
}

// The pinhole: PerspectiveCameraImpl::sampleRayDifferential (perspective.cpp:271-298).
// nearP of film position (sx, sy), which thinlens shares
__device__ __forceinline__ f3 sensor_near_point(const MtsgCamera &cam, float sx, float sy) {
    return xf_point(cam.sample_to_camera, mk(sx * cam.inv_res_x, sy * cam.inv_res_y, 0.0f));
}
// the ray's direction in camera space and invZ = 1 / its z: the world direction is
// xf_vector(to_world, .), the interval [near_clip, far_clip] * invZ
__device__ __forceinline__ f3 pinhole_dir(const MtsgCamera &cam, float sx, float sy, float &invZ) {
    const f3 dl = normalize(sensor_near_point(cam, sx, sy));
    invZ = 1.0f / dl.z;
    return dl;
}
// every pinhole ray's origin, toWorld(0, 0, 0) (wave-uniform)
__device__ __forceinline__ f3 pinhole_origin(const MtsgCamera &cam) {
    const float *W = cam.to_world;
    return mk(W[0] * 0.0f + W[1] * 0.0f + W[2] * 0.0f + W[3], W[4] * 0.0f + W[5] * 0.0f + W[6] * 0.0f + W[7],
              W[8] * 0.0f + W[9] * 0.0f + W[10] * 0.0f + W[11]);
}
// origin, direction, [mint, maxt]
__device__ __forceinline__ void camera_ray(const MtsgCamera &cam, float sx, float sy, f3 &ro, f3 &rd, float &mint,
                                           float &maxt) {
    float invZ;
    const f3 dl = pinhole_dir(cam, sx, sy, invZ);
    mint = cam.near_clip * invZ;
    maxt = cam.far_clip * invZ;
    ro = pinhole_origin(cam);
    rd = xf_vector(cam.to_world, dl);
}
// the aperture point of (ax, ay): squareToUniformDiskConcentric(apertureSample) * radius
__device__ __forceinline__ void sensor_aperture(const MtsgCameraLens &ln, float ax, float ay, float &tx, float &ty) {
    float dx, dy;
    square_to_disk_concentric(ax, ay, dx, dy);
    tx = dx * ln.aperture_radius;
    ty = dy * ln.aperture_radius;
}

// origin, direction and [mint, maxt] of the sensor ray through film position (sx, sy)
// with aperture sample (ax, ay) (ignored by orthographic)
__device__ __forceinline__ void sensor_ray(const MtsgCamera &cam, const MtsgCameraLens &ln, float sx, float sy, float ax,
                                           float ay, f3 &o, f3 &d, float &mint, float &maxt) {
    const float *W = cam.to_world;
    const f3 film = mk(sx * cam.inv_res_x, sy * cam.inv_res_y, 0.0f);
    if (ln.type == MTSG_SENSOR_ORTHOGRAPHIC) {   // orthographic.cpp:157-179
        f3 nearP = xf_affine(cam.sample_to_camera, film);
        nearP.z = 0.0f;
        o = xf_affine(W, nearP);
        d = ld3(ln.ortho_dir);
        mint = cam.near_clip;
        maxt = cam.far_clip;
    } else if (ln.type == MTSG_SENSOR_TELECENTRIC) {   // telecentric.cpp:224-255
        float tx, ty;
        sensor_aperture(ln, ax, ay, tx, ty);   // (aperture_radius: m_apertureRadius / m_scale.x)
        f3 focusP = xf_affine(cam.sample_to_camera, film);
        focusP.z = ln.focus_distance;          // (m_focusDistance / m_scale.z)
        const f3 orig = mk(tx + focusP.x, ty + focusP.y, 0.0f);
        o = xf_affine(W, orig);
        d = normalize(xf_vector(W, sub(focusP, orig)));
        mint = cam.near_clip;
        maxt = cam.far_clip;
    } else {   // MTSG_SENSOR_THINLENS (thinlens.cpp:324-361); `perspective` never runs these kernels
        const f3 nearP = xf_point(cam.sample_to_camera, film);
        f3 ap = mk(0.0f, 0.0f, 0.0f);
        sensor_aperture(ln, ax, ay, ap.x, ap.y);
        const float fDist = ln.focus_distance / nearP.z;
        const f3 dl = normalize(sub(mul(nearP, fDist), ap));
        const float invZ = 1.0f / dl.z;
        mint = cam.near_clip * invZ;
        maxt = cam.far_clip * invZ;
        o = xf_affine(W, ap);
        d = xf_vector(W, dl);
    }
}

// The directions of the sensor ray's two differential rays after
// RayDifferential::scaleDifferential(scale) (ray.h:163-168), for Scene::evalEnvironment of a
// camera ray that misses (the envmap's filtered lookup reads the directions alone,
// envmap.cpp:380-410).  rd: the ray's own direction (sensor_ray's).  orthographic and
// telecentric set rxDirection = ryDirection = d: d + (d - d) * scale is d, the lookup's
// degenerate ellipse, whatever the scale
__device__ __forceinline__ void sensor_ray_diff(const MtsgCamera &cam, const MtsgCameraLens &ln, float sx, float sy,
                                                float ax, float ay, f3 rd, float scale, f3 &rxd, f3 &ryd) {
    if (ln.type == MTSG_SENSOR_ORTHOGRAPHIC || ln.type == MTSG_SENSOR_TELECENTRIC) {
        rxd = ryd = rd;
    } else {
        const float *W = cam.to_world;
        const f3 nearP = sensor_near_point(cam, sx, sy);
        f3 ap = mk(0.0f, 0.0f, 0.0f);   // thinlens: focusPx, focusPy seen from the aperture point
        sensor_aperture(ln, ax, ay, ap.x, ap.y);
        const float fDist = ln.focus_distance / nearP.z;
        const f3 rxl = normalize(sub(mul(add(nearP, ld3(cam.dx)), fDist), ap));
        const f3 ryl = normalize(sub(mul(add(nearP, ld3(cam.dy)), fDist), ap));
        rxd = xf_vector(W, rxl);
        ryd = xf_vector(W, ryl);
    }
    rxd = add(rd, mul(sub(rxd, rd), scale));
    ryd = add(rd, mul(sub(ryd, rd), scale));
}
