// dpunct.h -- next-event estimation of the punctual lights: point, spot and sun (which is normative: every parenthesis
// below is an operand order). The reference has the schema (akari_scenegraph/src/scene.rs: Light::Point) and no implementation. All three are delta
// lights: a BSDF-sampled ray never hits one, so the sample carries no MIS partner (LightSample.delta, dpath.h path_step), and it draws no random
// number of its own -- the light was chosen with u_select like every other. AKR_HD: the test hook akr_host_light_sample runs this text on the host.
#pragma once
#include "dscene.h"

namespace akr {

struct PunctSample {
    vec3 li, wi, ro;
    float tmax;
    bool valid;
};
// the sample of light L at the surface point p with geometric normal n
AKR_HD PunctSample punct_sample(const DPunct& L, vec3 p, vec3 n) {
    PunctSample s;
    s.li = mk3(0, 0, 0);
    s.wi = mk3(0, 0, 0);
    s.ro = mk3(0, 0, 0);
    s.tmax = 0.0f;
    s.valid = false;
    bool ok = true;
    if (L.kind == PUNCT_SUN) {
        s.wi = -L.a;
        s.li = L.c;
        s.tmax = 1e20f;  // closest-ray convention, as the environment's shadow ray
    } else {
        const vec3 d = L.q - p;
        const float dist2 = dot(d, d);
        if (dist2 == 0.0f) return s;
        const float dist = sqrt_f(dist2);
        s.wi = div_s(d, dist);
        if (L.kind == PUNCT_POINT) {
            s.li = div_s(L.c, dist2);
        } else {
            const float ct = -dot(s.wi, L.a);
            float f;
            if (L.inv_span != 0.0f) {
                const float t = clamp_f((ct - L.cos_o) * L.inv_span, 0.0f, 1.0f);
                f = (t * t) * (3.0f - 2.0f * t);
            } else {
                f = ct > L.cos_o ? 1.0f : 0.0f;
            }
            s.li = div_s(L.c * f, dist2);
            ok = f > 0.0f;  // no shadow ray outside the cone
        }
        s.tmax = dist * (1.0f - 1e-3f);
    }
    s.ro = offset_ray_origin(p, face_forward(n, s.wi));
    s.valid = ok && is_finite(s.li.x) && is_finite(s.li.y) && is_finite(s.li.z);
    return s;
}

// One row of the test hooks akr_host_light_sample / akr_probe_light_sample: in7 = p, n, u_select -> out13 = li, wi, pdf, ro, tmax, valid, delta and the
// light chosen; the selection and the punctual branch of sample_direct (dpath.h) over the same tables.
AKR_HD void punct_probe_row(const AliasPacked* light_alias, const LightRec* lights, const DPunct* punct, uint32_t n_lights, const float* in7, float* out13, uint32_t* light_out) {
    for (int k = 0; k < 13; k++) out13[k] = 0.0f;
    *light_out = kInvalid;
    if (n_lights == 0) return;
    float light_choice_pdf, u_sel2;
    const uint32_t light = alias_sample_and_remap(light_alias, n_lights, in7[6], light_choice_pdf, u_sel2);
    *light_out = light;
    out13[6] = light_choice_pdf;
    const LightRec L = lights[light];
    if (L.inst != kPunctInst) return;
    const PunctSample s = punct_sample(punct[L.first_gid], mk3(in7[0], in7[1], in7[2]), mk3(in7[3], in7[4], in7[5]));
    out13[0] = s.li.x; out13[1] = s.li.y; out13[2] = s.li.z;
    out13[3] = s.wi.x; out13[4] = s.wi.y; out13[5] = s.wi.z;
    out13[7] = s.ro.x; out13[8] = s.ro.y; out13[9] = s.ro.z;
    out13[10] = s.tmax;
    out13[11] = s.valid ? 1.0f : 0.0f;
    out13[12] = 1.0f;
}

}  // namespace akr
