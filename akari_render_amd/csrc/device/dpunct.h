// dpunct.h -- next-event estimation of the punctual lights: point, spot and sun (DESIGN.md sections 4.14 and 4.15, which are normative: every
// parenthesis below is an operand order). The reference has the schema (akari_scenegraph/src/scene.rs: Light::Point) and no implementation. A light
// without a size is a delta light and draws no random number of its own -- it was chosen with u_select like every other. A light with a size (a
// radius: a disk at q that faces the shading point; an angle: a cap of directions around -a) draws its point from the u_sample an emitter's triangle
// would use. Either way a BSDF-sampled ray never hits one, so the sample carries no MIS partner (LightSample.delta, dpath.h path_step). AKR_HD: the
// test hooks akr_host_light_sample / akr_host_light_sample_soft run this text on the host.
#pragma once
#include "dscene.h"

namespace akr {

struct PunctSample {
    vec3 li, wi, ro;
    float tmax;
    bool valid;
};
// the smoothstep (or step) falloff of a spot light at the cosine ct between its axis and the direction the light leaves in
AKR_HD float punct_spot_falloff(const DPunct& L, float ct) {
    if (L.inv_span != 0.0f) {
        const float t = clamp_f((ct - L.cos_o) * L.inv_span, 0.0f, 1.0f);
        return (t * t) * (3.0f - 2.0f * t);
    }
    return ct > L.cos_o ? 1.0f : 0.0f;
}
// the sample of light L at the surface point p with geometric normal n; u: the two numbers a light with a size draws its point from; any_soft: some light of
// the scene has a size (DScene.n_punct's top bit, the same for every lane) -- without it no record is asked for its size
AKR_HD PunctSample punct_sample(const DPunct& L, vec3 p, vec3 n, vec2 u, bool any_soft) {
    PunctSample s;
    s.li = mk3(0, 0, 0);
    s.wi = mk3(0, 0, 0);
    s.ro = mk3(0, 0, 0);
    s.tmax = 0.0f;
    s.valid = false;
    bool ok = true;
    if (L.kind == PUNCT_SUN) {
        if (any_soft && L.cos_max != 0.0f) {  // a cap of half-angle acos(cos_max) around -a, uniformly radiant: a direction uniform in solid angle
            const float ct = 1.0f - u.x * (1.0f - L.cos_max);
            const float st = sqrt_f(max_f(1.0f - ct * ct, 0.0f));
            float sp, cp;
            sincos_f((2.0f * kPi) * u.y, sp, cp);
            s.wi = to_world(frame_from_n(-L.a), mk3(st * cp, st * sp, ct));
            s.li = L.c * L.k;
        } else {
            s.wi = -L.a;
            s.li = L.c;
        }
        s.tmax = 1e20f;  // closest-ray convention, as the environment's shadow ray
    } else {
        const vec3 d = L.q - p;
        const float dist2 = dot(d, d);
        if (dist2 == 0.0f) return s;
        // w: from p to the point of the light the sample looks at -- q itself, or a point of the disk
        vec3 w = d, nd = mk3(0, 0, 0);
        float w2 = dist2;
        const bool soft = any_soft && L.radius != 0.0f;
        if (soft) {  // a disk of that radius at q whose normal nd points at p, uniformly emitting: a point uniform in area
            nd = -div_s(d, sqrt_f(dist2));
            const Frame fr = frame_from_n(nd);
            const vec2 dd = concentric_disk(u);
            const vec3 y = L.q + (fr.t * (L.radius * dd.x) + fr.s * (L.radius * dd.y));
            w = y - p;
            w2 = dot(w, w);
        }
        const float dist = sqrt_f(w2);
        s.wi = div_s(w, dist);
        vec3 i = L.c;
        if (L.kind == PUNCT_SPOT) {
            const float f = punct_spot_falloff(L, -dot(s.wi, L.a));
            i = L.c * f;
            ok = f > 0.0f;  // no shadow ray outside the cone
        }
        if (soft) {
            const float cosl = -dot(s.wi, nd);
            i = i * cosl;
            ok = ok && cosl > 0.0f;  // (it is, but for rounding at p a millionth of the radius from q)
        }
        s.li = div_s(i, w2);
        s.tmax = dist * (1.0f - 1e-3f);
    }
    s.ro = offset_ray_origin(p, face_forward(n, s.wi));
    s.valid = ok && is_finite(s.li.x) && is_finite(s.li.y) && is_finite(s.li.z);
    return s;
}

// One row of the test hooks akr_host_light_sample_soft / akr_probe_light_sample_soft: in9 = p, n, u_select, u_sample -> out13 = li, wi, pdf, ro, tmax,
// valid, delta and the light chosen; the selection and the punctual branch of sample_direct (dpath.h) over the same tables.
AKR_HD void punct_probe_row(const AliasPacked* light_alias, const LightRec* lights, const DPunct* punct, uint32_t n_lights, const float* in9, float* out13, uint32_t* light_out) {
    for (int k = 0; k < 13; k++) out13[k] = 0.0f;
    *light_out = kInvalid;
    if (n_lights == 0) return;
    float light_choice_pdf, u_sel2;
    const uint32_t light = alias_sample_and_remap(light_alias, n_lights, in9[6], light_choice_pdf, u_sel2);
    *light_out = light;
    out13[6] = light_choice_pdf;
    const LightRec L = lights[light];
    if (L.inst != kPunctInst) return;
    const PunctSample s = punct_sample(punct[L.first_gid], mk3(in9[0], in9[1], in9[2]), mk3(in9[3], in9[4], in9[5]), mk2(in9[7], in9[8]), true);
    out13[0] = s.li.x; out13[1] = s.li.y; out13[2] = s.li.z;
    out13[3] = s.wi.x; out13[4] = s.wi.y; out13[5] = s.wi.z;
    out13[7] = s.ro.x; out13[8] = s.ro.y; out13[9] = s.ro.z;
    out13[10] = s.tmax;
    out13[11] = s.valid ? 1.0f : 0.0f;
    out13[12] = 1.0f;
}

}  // namespace akr
