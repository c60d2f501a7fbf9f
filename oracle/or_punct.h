/* or_punct.h -- the punctual lights of the CPU oracle, delta and soft (TEST INFRASTRUCTURE ONLY).
 *
 * A restatement of DESIGN.md sections 4.14 and 4.15 (the reference has the schema of a point light and no code behind it, so those two
 * sections are the specification): the description checked and normalised as akr_scene_add_punctual_light does ("Lights", "Validation"),
 * the fold of a light into its sixteen-word record in f64 with each value rounded once ("Host fold", "Record, fold"), the selection
 * weight of each kind ("Light list") and the light sample in the f32 operand order the two "Sampling" blocks make normative. It is
 * written from that text, not from the library's sources, and calls nothing of the library.
 */
#ifndef OR_PUNCT_H
#define OR_PUNCT_H
#include "or_api.h"
#include "or_geom.h"
#include "or_math.h"
#include "or_tex.h"
#include <math.h>

#define OR_PUNCT_INST 0xfffffffeu /* what the light list reports as the instance of a punctual light (4.14 "Light list") */

/* 4.14 "Host fold" / 4.15 "Record, fold": q | kind, a | cos_o, c | cos_i, inv_span, radius, cos_max, k -- 64 bytes */
typedef struct {
    v3 q; uint32_t kind;
    v3 a; float cos_o;
    v3 c; float cos_i;
    float inv_span, radius, cos_max, k;
} or_punct;

/* 4.14 "Lights" + the setter's refusals, 4.15 "Validation": -1 = refused, 0 = accepted and no light (strength 0 or an all-zero
 * colour), 1 = a light. *out: the description with what its kind does not read stored as zero. */
static int or_punct_check(const or_punctual_light_desc *d, or_punctual_light_desc *out) {
    if (d->type > OR_LIGHT_SUN) return -1;
    if (!or_isfinite(d->strength) || d->strength < 0.0f) return -1;
    int lit = 0;
    for (int k = 0; k < 3; k++) {
        if (!or_isfinite(d->color[k]) || d->color[k] < 0.0f) return -1;
        if (d->color[k] > 0.0f) lit = 1;
    }
    if (d->type != OR_LIGHT_SUN)
        for (int k = 0; k < 3; k++)
            if (!or_isfinite(d->position[k])) return -1;
    if (d->type != OR_LIGHT_POINT) { /* a zero or non-finite axis is refused */
        double l2 = 0.0;
        for (int k = 0; k < 3; k++) {
            if (!or_isfinite(d->direction[k])) return -1;
            l2 += (double)d->direction[k] * (double)d->direction[k];
        }
        if (!(l2 > 0.0)) return -1;
    }
    if (d->type == OR_LIGHT_SPOT) { /* cone_angle in (0, pi/2] -- pi/2 as the f32 nearest to it --, blend in [0, 1] */
        if (!or_isfinite(d->cone_angle) || !(d->cone_angle > 0.0f) || d->cone_angle > 1.57079637f) return -1;
        if (!or_isfinite(d->blend) || d->blend < 0.0f || d->blend > 1.0f) return -1;
    }
    /* 4.15: the size the kind reads; the other kind's is not looked at, whatever it holds. The angle is compared with pi in double. */
    if (d->type != OR_LIGHT_SUN && (!or_isfinite(d->radius) || d->radius < 0.0f)) return -1;
    if (d->type == OR_LIGHT_SUN && (!or_isfinite(d->angle) || d->angle < 0.0f || (double)d->angle >= M_PI)) return -1;
    *out = *d;
    if (d->type == OR_LIGHT_SUN) out->position[0] = out->position[1] = out->position[2] = 0.0f;
    if (d->type == OR_LIGHT_POINT) out->direction[0] = out->direction[1] = out->direction[2] = 0.0f;
    if (d->type != OR_LIGHT_SPOT) out->cone_angle = out->blend = 0.0f;
    if (d->type == OR_LIGHT_SUN || d->radius == 0.0f) out->radius = 0.0f; /* "read back as 0"; a -0 is the +0 that says "delta" */
    if (d->type != OR_LIGHT_SUN || d->angle == 0.0f) out->angle = 0.0f;
    return lit && d->strength > 0.0f;
}

/* 4.14 "Host fold", 4.15 "Record, fold", for the colour pipeline `color` (OR_COLOR_* bits) */
static or_punct or_punct_fold(const or_punctual_light_desc *d, uint32_t color) {
    or_punct r;
    memset(&r, 0, sizeof r);
    r.kind = d->type;
    if (d->type != OR_LIGHT_SUN) r.q = V3(d->position[0], d->position[1], d->position[2]);
    if (d->type != OR_LIGHT_POINT) { /* a normalised in f64, each component rounded once */
        const double x = d->direction[0], y = d->direction[1], z = d->direction[2];
        const double len = sqrt((x * x + y * y) + z * z);
        r.a = V3((float)(x / len), (float)(y / len), (float)(z / len));
    }
    if (d->type == OR_LIGHT_SPOT) {
        r.cos_o = (float)cos((double)d->cone_angle);
        r.cos_i = (float)cos((double)d->cone_angle * (1.0 - (double)d->blend));
        r.inv_span = r.cos_i == r.cos_o ? 0.0f : 1.0f / (r.cos_i - r.cos_o); /* one f32 division of the two stored values */
    }
    if (d->type != OR_LIGHT_SUN) r.radius = d->radius;
    else if (d->angle > 0.0f) {
        const double cm = cos(0.5 * (double)d->angle);
        r.cos_max = (float)cm;
        r.k = (float)(2.0 / (1.0 + cm));
    }
    /* c = color . strength per channel in f32, then the way of an Emission material's constant colour (tagged sRGB) into the pipeline:
     * the given space -> the pipeline's RGB space -> the space it shades in (or_tex.h or_material_at) */
    float c[3] = {d->color[0] * d->strength, d->color[1] * d->strength, d->color[2] * d->strength};
    or_cs_convert(c, 0, (color & OR_COLOR_RGB_ACES) != 0);
    or_cs_convert(c, (color & OR_COLOR_RGB_ACES) != 0, (color & OR_COLOR_REPR_ACES) != 0);
    r.c = V3(c[0], c[1], c[2]);
    return r;
}

/* 4.14 "Light list": the selection weight, in f64 and rounded once; m of the default pipeline's record, R half the diagonal of the world
 * bounds (1 without geometry), as for the environment. 4.15: it does not look at radius or angle. */
static double or_punct_bounds_radius(const float lo[3], const float hi[3]) {
    double r2 = 0.0;
    for (int a = 0; a < 3; a++) { const double ext = (double)hi[a] - (double)lo[a]; r2 += ext * ext; }
    const double rad = 0.5 * sqrt(r2);
    return (!(rad > 0.0) || !isfinite(rad)) ? 1.0 : rad;
}
static float or_punct_power(const or_punct *r, double R) {
    const double m = (double)v3max(r->c);
    if (r->kind == OR_LIGHT_POINT) return (float)((4.0 * M_PI) * m);
    if (r->kind == OR_LIGHT_SPOT) return (float)(((2.0 * M_PI) * (1.0 - 0.5 * ((double)r->cos_i + (double)r->cos_o))) * m);
    return (float)(((M_PI * R) * R) * m);
}

/* Shirley-Chiu, unit square -> unit disk (4.9 step 2; 4.15 uses the lens's warp) */
static inline v2 or_concentric_disk(v2 u) {
    const float sx = 2.0f * u.x - 1.0f, sy = 2.0f * u.y - 1.0f;
    if (sx == 0.0f && sy == 0.0f) return V2(0.0f, 0.0f);
    float r, theta;
    if (fabsf(sx) > fabsf(sy)) { r = sx; theta = 0.785398163397448310f * (sy / sx); }
    else { r = sy; theta = 1.570796326794896619f - 0.785398163397448310f * (sx / sy); }
    float sn, cs;
    or_sincosf(theta, &sn, &cs);
    return V2(r * cs, r * sn);
}

/* the spot's falloff from ct = -dot(wi, a): smoothstep between the two cosines, or the step when they are equal (4.14) */
static inline float or_punct_falloff(const or_punct *L, float ct) {
    if (L->inv_span != 0.0f) {
        const float s = or_clamp((ct - L->cos_o) * L->inv_span, 0.0f, 1.0f); /* a NaN goes to 0 */
        return (s * s) * (3.0f - 2.0f * s);
    }
    return ct > L->cos_o ? 1.0f : 0.0f;
}

typedef struct { v3 li, wi, ro; float tmax; int valid; } or_punct_ls;

/* 4.14 / 4.15 "Sampling": the light's sample at p with the geometric normal n; u is the u_sample every light choice draws, read only
 * by a light with a size. With p == q nothing is computed: zeros, invalid. */
static or_punct_ls or_punct_sample(const or_punct *L, v3 p, v3 n, v2 u) {
    or_punct_ls s;
    memset(&s, 0, sizeof s);
    int ok = 1;
    if (L->kind == OR_LIGHT_SUN) {
        if (L->cos_max != 0.0f) { /* a cap of half-angle angle / 2 around -a, uniform in solid angle */
            const float ct = 1.0f - u.x * (1.0f - L->cos_max);
            const float st = sqrtf(or_max(1.0f - ct * ct, 0.0f));
            float sp, cp;
            or_sincosf((2.0f * OR_PI) * u.y, &sp, &cp);
            const or_frame f = or_frame_from_n(v3neg(L->a));
            s.wi = or_to_world(&f, V3(st * cp, st * sp, ct)); /* not normalised again */
            s.li = v3scale(L->c, L->k);
        } else {
            s.wi = v3neg(L->a);
            s.li = L->c;
        }
        s.tmax = 1e20f;
    } else if (L->radius != 0.0f) { /* a disk of `radius` around q whose normal points at p */
        const v3 d = v3sub(L->q, p);
        const float dist2c = v3dot(d, d);
        if (dist2c == 0.0f) return s;
        const v3 nd = v3neg(v3divs(d, sqrtf(dist2c)));
        const or_frame f = or_frame_from_n(nd);
        const v2 dd = or_concentric_disk(u);
        const v3 y = v3add(L->q, v3add(v3scale(f.t, L->radius * dd.x), v3scale(f.s, L->radius * dd.y)));
        const v3 w = v3sub(y, p);
        const float w2 = v3dot(w, w), dist = sqrtf(w2);
        s.wi = v3divs(w, dist);
        const float cosl = -v3dot(s.wi, nd);
        if (L->kind == OR_LIGHT_POINT) s.li = v3divs(v3scale(L->c, cosl), w2);
        else {
            const float fo = or_punct_falloff(L, -v3dot(s.wi, L->a)); /* at the sampled direction */
            s.li = v3divs(v3scale(v3scale(L->c, fo), cosl), w2);
            if (!(fo > 0.0f)) ok = 0;
        }
        if (!(cosl > 0.0f)) ok = 0;
        s.tmax = dist * (1.0f - 1e-3f);
    } else {
        const v3 d = v3sub(L->q, p);
        const float dist2 = v3dot(d, d);
        if (dist2 == 0.0f) return s;
        const float dist = sqrtf(dist2);
        s.wi = v3divs(d, dist);
        if (L->kind == OR_LIGHT_POINT) s.li = v3divs(L->c, dist2);
        else {
            const float fo = or_punct_falloff(L, -v3dot(s.wi, L->a));
            s.li = v3divs(v3scale(L->c, fo), dist2);
            if (!(fo > 0.0f)) ok = 0; /* no shadow ray outside the cone */
        }
        s.tmax = dist * (1.0f - 1e-3f);
    }
    s.ro = or_offset_ray_origin(p, or_face_forward(n, s.wi));
    s.valid = ok && or_isfinite(s.li.x) && or_isfinite(s.li.y) && or_isfinite(s.li.z);
    return s;
}
#endif
