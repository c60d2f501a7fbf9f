// denv.h -- the environment light of the `pt` integrator: lookup, importance sampling and pdf of an equirectangular image.
//
// Mapping (Blender's equirectangular World after the exporter's axis change, Blender (x, y, z) -> scene (x, z, -y)): a world
// direction d is turned into the environment's frame, e = R^T d, and looked up at
//   u = 0.5 + atan2(e.z, e.x) / 2pi,   v = 0.5 + atan2(e.y, hypot(e.x, e.z)) / pi,
// texels addressed as image textures are (row 0 is v = 0, centres at +0.5), u wrapping, v clamped. v is the elevation: the polar
// angle from +y is theta = pi (1 - v), so sin(theta) = hypot(e.x, e.z) and d(omega) = 2 pi^2 sin(theta) du dv.
// Sampling: an alias table over the rows (marginal) and one per row over its columns (conditional), built on the host from the texels'
// 3x3-maximum luminance times sin(theta) at the texel centre (host/scene_env.cpp); the remainders of the two choices place the point
// inside the texel, so pdf(omega) = p_row p_col W H / (2 pi^2 sin(theta)).
#pragma once
#include "dscene.h"

namespace akr {

// atan2 in single precision (Cephes atanf kernel after reduction to |x| <= tan(pi/8)); the same code on the host and the device
AKR_HD float atan_unit_f(float t) {  // t in [0, 1]
    float y0 = 0.0f, x = t;
    if (t > 0.41421356237309503f) {
        x = (t - 1.0f) / (t + 1.0f);
        y0 = 0.78539816339744831f;
    }
    const float z = x * x;
    const float p = (((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z * x + x;
    return y0 + p;
}
AKR_HD float atan2_f(float y, float x) {
    const float ax = abs_f(x), ay = abs_f(y);
    const float hi = max_f(ax, ay), lo = min_f(ax, ay);
    if (hi == 0.0f) return 0.0f;
    float a = atan_unit_f(lo / hi);
    if (ay > ax) a = 1.57079632679489662f - a;
    if (x < 0.0f) a = kPi - a;
    return y < 0.0f ? -a : a;
}

AKR_HD vec3 env_to_local(const DEnv& env, vec3 d) {
    const float* r = env.rot;
    return mk3((r[0] * d.x + r[1] * d.y) + r[2] * d.z, (r[3] * d.x + r[4] * d.y) + r[5] * d.z, (r[6] * d.x + r[7] * d.y) + r[8] * d.z);
}
AKR_HD vec3 env_to_world(const DEnv& env, vec3 e) {  // R e = (R^T)^T e
    const float* r = env.rot;
    return mk3((r[0] * e.x + r[3] * e.y) + r[6] * e.z, (r[1] * e.x + r[4] * e.y) + r[7] * e.z, (r[2] * e.x + r[5] * e.y) + r[8] * e.z);
}
// (u, v) and sin(theta) of an environment-frame direction
AKR_HD vec2 env_uv(vec3 e, float& sin_theta) {
    sin_theta = __builtin_sqrtf(e.x * e.x + e.z * e.z);
    const float u = 0.5f + atan2_f(e.z, e.x) * (0.5f * kInvPi);
    const float v = 0.5f + atan2_f(e.y, sin_theta) * kInvPi;
    return mk2(clamp_f(u, 0.0f, 1.0f), clamp_f(v, 0.0f, 1.0f));  // (in [0, 1] already; a NaN direction reads texel 0)
}
AKR_HD void env_texel_of(const DEnv& env, vec2 uv, uint32_t& x, uint32_t& y) {
    float fx = __builtin_floorf(uv.x * (float)env.w), fy = __builtin_floorf(uv.y * (float)env.h);
    int32_t ix = (int32_t)fx, iy = (int32_t)fy;
    ix = ix < 0 ? 0 : (ix > (int32_t)env.w - 1 ? (int32_t)env.w - 1 : ix);
    iy = iy < 0 ? 0 : (iy > (int32_t)env.h - 1 ? (int32_t)env.h - 1 : iy);
    x = (uint32_t)ix;
    y = (uint32_t)iy;
}
AKR_HD vec3 env_texel(const DEnv& env, int32_t x, int32_t y) {
    const float4 t = env.texels[(size_t)y * env.w + (size_t)x];
    return mk3(t.x, t.y, t.z);
}
// radiance at (u, v): nearest or bilinear (texel centres at +0.5, lerp a + (b - a) t as for image textures), u wraps, v clamps
AKR_HD vec3 env_lookup(const DEnv& env, vec2 uv) {
    const int32_t w = (int32_t)env.w, h = (int32_t)env.h;
    if (env.filter == 0u) {
        uint32_t x, y;
        env_texel_of(env, uv, x, y);
        return env_texel(env, (int32_t)x, (int32_t)y);
    }
    const float fx = uv.x * (float)w - 0.5f, fy = uv.y * (float)h - 0.5f;
    const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
    const float tx = fx - x0f, ty = fy - y0f;
    int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
    int32_t x1 = x0 + 1, y1 = y0 + 1;
    x0 = ((x0 % w) + w) % w;
    x1 = ((x1 % w) + w) % w;
    y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > h - 1 ? h - 1 : y1);
    const vec3 a = env_texel(env, x0, y0), b = env_texel(env, x1, y0), c = env_texel(env, x0, y1), d = env_texel(env, x1, y1);
    const vec3 ab = a + (b - a) * tx, cd = c + (d - c) * tx;
    return ab + (cd - ab) * ty;
}
// radiance arriving from world direction d, in the shading colour space of the launch (`color`: ColorPipeline bits; the texels are in
// its RGB space, as an image texture feeding an emission colour through spectral_uplift)
AKR_HD vec3 env_eval(const DEnv& env, uint32_t color, vec3 d) {
    float st;
    const vec3 c = env_lookup(env, env_uv(env_to_local(env, d), st));
    if (color == 0u) return c;
    return cs_convert(c, (color & COLOR_RGB_ACES) != 0, (color & COLOR_REPR_ACES) != 0);
}
// solid-angle pdf of env_sample at world direction d (0 at the poles)
AKR_D float env_pdf(const DEnv& env, vec3 d) {
    float st;
    const vec2 uv = env_uv(env_to_local(env, d), st);
    if (!(st > 0.0f)) return 0.0f;
    uint32_t x, y;
    env_texel_of(env, uv, x, y);
    const float p_row = env.marginal[y].pdf_i, p_col = env.conditional[(size_t)y * env.w + x].pdf_i;
    return (p_row * p_col) * ((float)env.w * (float)env.h) / ((2.0f * kPi * kPi) * st);
}
// a direction from the tables: u2.y picks the row, u2.x the column, the remainders the point in the texel
AKR_D bool env_sample(const DEnv& env, vec2 u2, vec3& wi, float& pdf) {
    float p_row, p_col, ry, rx;
    const uint32_t y = alias_sample_and_remap(env.marginal, env.h, u2.y, p_row, ry);
    const uint32_t x = alias_sample_and_remap(env.conditional + (size_t)y * env.w, env.w, u2.x, p_col, rx);
    const float u = ((float)x + rx) / (float)env.w, v = ((float)y + ry) / (float)env.h;
    float sp, cp, sl, cl;
    sincos_f((u - 0.5f) * (2.0f * kPi), sp, cp);
    sincos_f((v - 0.5f) * kPi, sl, cl);
    wi = env_to_world(env, mk3(cl * cp, sl, cl * sp));
    pdf = 0.0f;
    if (!(cl > 0.0f)) return false;
    pdf = (p_row * p_col) * ((float)env.w * (float)env.h) / ((2.0f * kPi * kPi) * cl);
    return is_finite(pdf) && pdf > 0.0f;
}

}  // namespace akr
