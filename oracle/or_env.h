/* or_env.h -- the environment light of the CPU oracle (TEST INFRASTRUCTURE ONLY).
 *
 * A restatement of DESIGN.md section 4.8 (the reference's hit_envmap returns zero, so that section is the specification): the
 * description checked as akr_scene_set_environment checks it, the texels with the strength applied, the 2D piecewise-constant
 * distribution (3x3-maximum x sin(theta) weights, one alias table over the rows, one per row over its columns), the environment's
 * weight 4 pi R^2 Lbar in the light table, and the mapping, lookup, sampling and pdf in the f32 evaluation order 4.8 makes normative.
 * The world-direction <-> (u, v) mapping is Blender's equirectangular World after the exporter's axis change.
 */
#ifndef OR_ENV_H
#define OR_ENV_H
#include "or_api.h"
#include "or_geom.h"
#include "or_math.h"
#include "or_tex.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define OR_ENV_CONST_W 32u /* a constant colour is stored as a 32 x 16 image of that colour */
#define OR_ENV_CONST_H 16u

typedef struct {
    uint32_t w, h, filter;       /* filter: OR_TEX_NEAREST / OR_TEX_LINEAR (a constant colour: nearest) */
    float *texels;               /* RGBA32F, w x h, row 0 = v = 0, strength applied, alpha 1 */
    float R[9];                  /* environment -> world, row-major, as given */
    or_alias_table marginal;     /* h entries */
    or_alias_table *conditional; /* h tables of w entries */
    float power;                 /* 4 pi R^2 Lbar */
} or_env;

static void or_env_free(or_env *e) {
    if (!e) return;
    or_alias_free(&e->marginal);
    for (uint32_t y = 0; y < e->h; y++) or_alias_free(&e->conditional[y]);
    free(e->conditional);
    free(e->texels);
    free(e);
}

static inline int or_clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

/* The checks of akr_scene_set_environment (4.8): returns 0 and *out (NULL = "no environment": strength 0, or nothing above 0), or
 * -1 for a description the library refuses. `lo` / `hi`: the scene's world bounds over every triangle corner (lo > hi: no geometry). */
static int or_env_create(const or_environment_desc *d, const float lo[3], const float hi[3], or_env **out) {
    *out = 0;
    if (!or_isfinite(d->strength) || d->strength < 0.0f) return -1;
    if ((d->width == 0) != (d->height == 0)) return -1;
    if (d->filter != OR_TEX_NEAREST && d->filter != OR_TEX_LINEAR) return -1;
    if ((uint64_t)d->width * d->height > (1ull << 28)) return -1;
    for (int k = 0; k < 9; k++)
        if (!or_isfinite(d->rotation[k])) return -1;
    { /* a rotation within 1e-4: R R^T = I (largest deviation of an entry) and det R = +1, in f64 */
        const float *r = d->rotation;
        double dev = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double s = 0.0;
                for (int k = 0; k < 3; k++) s += (double)r[3 * i + k] * (double)r[3 * j + k];
                s -= (i == j) ? 1.0 : 0.0;
                if (fabs(s) > dev) dev = fabs(s);
            }
        double det = (double)r[0] * ((double)r[4] * r[8] - (double)r[5] * r[7]) - (double)r[1] * ((double)r[3] * r[8] - (double)r[5] * r[6]) +
                     (double)r[2] * ((double)r[3] * r[7] - (double)r[4] * r[6]);
        if (dev > 1e-4 || fabs(det - 1.0) > 1e-4) return -1;
    }
    int lit = 0;
    if (d->width) {
        if (!d->texels) return -1;
        for (size_t t = 0; t < (size_t)d->width * d->height; t++)
            for (int c = 0; c < 3; c++) {
                float v = d->texels[4 * t + c];
                if (!or_isfinite(v) || v < 0.0f) return -1;
                if (v > 0.0f) lit = 1;
            }
    } else {
        for (int c = 0; c < 3; c++) {
            if (!or_isfinite(d->color[c]) || d->color[c] < 0.0f) return -1;
            if (d->color[c] > 0.0f) lit = 1;
        }
    }
    if (!lit || !(d->strength > 0.0f)) return 0;

    const int constant = d->width == 0;
    const uint32_t W = constant ? OR_ENV_CONST_W : d->width, H = constant ? OR_ENV_CONST_H : d->height;
    const size_t n = (size_t)W * H;
    or_env *e = (or_env *)calloc(1, sizeof(or_env));
    e->w = W; e->h = H; e->filter = constant ? OR_TEX_NEAREST : d->filter;
    memcpy(e->R, d->rotation, sizeof e->R);
    e->texels = (float *)malloc(16 * n);
    float *lum = (float *)malloc(4 * n);   /* max(r, g, b) of each texel, strength applied */
    float *wgt = (float *)malloc(4 * n);   /* sampling weight */
    float *rows = (float *)malloc(4 * H);  /* per-row sum of the weights */
    for (size_t t = 0; t < n; t++) {
        for (int c = 0; c < 3; c++) e->texels[4 * t + c] = (constant ? d->color[c] : d->texels[4 * t + c]) * d->strength;
        e->texels[4 * t + 3] = 1.0f;
        lum[t] = or_max(or_max(e->texels[4 * t], e->texels[4 * t + 1]), e->texels[4 * t + 2]);
    }
    /* weight = (f32)(m3 * sin(theta_y)), sin(theta_y) = sin(pi (y + 0.5) / H) in f64; row sums and the quadrature of Lbar in f64,
     * texels in row-major order */
    double lnum = 0.0, lden = 0.0;
    for (uint32_t y = 0; y < H; y++) {
        const double s = sin(M_PI * ((double)y + 0.5) / (double)H);
        double acc = 0.0;
        for (uint32_t x = 0; x < W; x++) {
            float m3 = lum[(size_t)y * W + x];
            if (e->filter == OR_TEX_LINEAR) /* 3x3 neighbourhood: u wraps, v clamps */
                for (int dy = -1; dy <= 1; dy++) {
                    const int yy = or_clampi((int)y + dy, 0, (int)H - 1);
                    for (int dx = -1; dx <= 1; dx++) m3 = or_max(m3, lum[(size_t)yy * W + (size_t)(((int)x + dx + (int)W) % (int)W)]);
                }
            wgt[(size_t)y * W + x] = (float)((double)m3 * s);
            acc += (double)wgt[(size_t)y * W + x];
            lnum += (double)lum[(size_t)y * W + x] * s;
            lden += s;
        }
        rows[y] = (float)acc;
    }
    double total = 0.0;
    for (uint32_t y = 0; y < H; y++) total += (double)rows[y];
    if (!(total > 0.0)) { /* every weight rounded to 0: nothing to sample, no environment */
        free(lum); free(wgt); free(rows); free(e->texels); free(e);
        return 0;
    }
    or_alias_build(&e->marginal, rows, H);
    e->conditional = (or_alias_table *)calloc(H, sizeof(or_alias_table));
    float *ones = (float *)malloc(4 * W);
    for (uint32_t x = 0; x < W; x++) ones[x] = 1.0f;
    for (uint32_t y = 0; y < H; y++) /* a row the marginal never picks gets the uniform table */
        or_alias_build(&e->conditional[y], rows[y] > 0.0f ? wgt + (size_t)y * W : ones, W);
    free(ones);
    /* R: half the diagonal of the world bounds (1 without geometry); power = ((4 pi R) R) (lnum / lden), f64, rounded once */
    double r2 = 0.0;
    for (int a = 0; a < 3; a++) { double ext = (double)hi[a] - (double)lo[a]; r2 += ext * ext; }
    double rad = 0.5 * sqrt(r2);
    if (!(rad > 0.0) || !isfinite(rad)) rad = 1.0;
    e->power = (float)(4.0 * M_PI * rad * rad * (lnum / lden));
    free(lum); free(wgt); free(rows);
    *out = e;
    return 0;
}

/* atan2 in f32: reduction to t = lo / hi in [0, 1], t > tan(pi/8) folded by (t - 1) / (t + 1) + pi/4, the Cephes atanf polynomial,
 * then the octant. atan2(+-0, x < 0) = +pi (the seam either way); atan2(0, 0) = 0. */
static inline float or_atan_unit(float t) {
    float base = 0.0f, x = t;
    if (t > 0.41421356237309503f) { x = (t - 1.0f) / (t + 1.0f); base = 0.78539816339744831f; }
    const float z = x * x;
    float p = 8.05374449538e-2f * z - 1.38776856032e-1f;
    p = p * z + 1.99777106478e-1f;
    p = p * z - 3.33329491539e-1f;
    p = ((p * z) * x) + x;
    return base + p;
}
static inline float or_atan2f(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float big = or_max(ax, ay), small = or_min(ax, ay);
    if (big == 0.0f) return 0.0f;
    float a = or_atan_unit(small / big);
    if (ay > ax) a = 1.57079632679489662f - a;
    if (x < 0.0f) a = OR_PI - a;
    return y < 0.0f ? -a : a;
}

/* e = R^T d: e_i = (R[0][i] d.x + R[1][i] d.y) + R[2][i] d.z; d = R e: d_i = (R[i][0] e.x + R[i][1] e.y) + R[i][2] e.z */
static inline v3 or_env_local(const or_env *e, v3 d) {
    const float *R = e->R;
    return V3((R[0] * d.x + R[3] * d.y) + R[6] * d.z, (R[1] * d.x + R[4] * d.y) + R[7] * d.z, (R[2] * d.x + R[5] * d.y) + R[8] * d.z);
}
static inline v3 or_env_world(const or_env *e, v3 l) {
    const float *R = e->R;
    return V3((R[0] * l.x + R[1] * l.y) + R[2] * l.z, (R[3] * l.x + R[4] * l.y) + R[5] * l.z, (R[6] * l.x + R[7] * l.y) + R[8] * l.z);
}
/* (u, v) of an environment-frame direction, clamped to [0, 1] (a NaN goes to 0); *sin_theta = sqrt(x x + z z) */
static inline v2 or_env_uv(v3 l, float *sin_theta) {
    const float st = sqrtf(l.x * l.x + l.z * l.z);
    *sin_theta = st;
    const float u = 0.5f + or_atan2f(l.z, l.x) * (0.5f * OR_INV_PI);
    const float v = 0.5f + or_atan2f(l.y, st) * OR_INV_PI;
    return V2(or_clamp(u, 0.0f, 1.0f), or_clamp(v, 0.0f, 1.0f));
}
static inline int or_env_index(float c, uint32_t n) { return or_clampi((int)floorf(c * (float)n), 0, (int)n - 1); } /* c in [0, 1] */
static inline v3 or_env_texel(const or_env *e, int x, int y) {
    const float *p = e->texels + 4 * ((size_t)y * e->w + (size_t)x);
    return V3(p[0], p[1], p[2]);
}
/* nearest: the texel containing (u, v); bilinear: centres at +0.5, t = f - floor(f), a + (b - a) t along u, then along v;
 * u wraps, v clamps */
static inline v3 or_env_lookup(const or_env *e, v2 uv) {
    if (e->filter == OR_TEX_NEAREST) return or_env_texel(e, or_env_index(uv.x, e->w), or_env_index(uv.y, e->h));
    const int W = (int)e->w, H = (int)e->h;
    const float fx = uv.x * (float)W - 0.5f, fy = uv.y * (float)H - 0.5f;
    const float flx = floorf(fx), fly = floorf(fy);
    const float tx = fx - flx, ty = fy - fly;
    const int ix = (int)flx, iy = (int)fly; /* in [-1, W - 1] and [-1, H - 1] */
    const int xa = (ix + W) % W, xb = (ix + 1) % W, ya = or_clampi(iy, 0, H - 1), yb = or_clampi(iy + 1, 0, H - 1);
    const v3 a = or_env_texel(e, xa, ya), b = or_env_texel(e, xb, ya), c = or_env_texel(e, xa, yb), d = or_env_texel(e, xb, yb);
    const v3 top = V3(or_lerp(a.x, b.x, tx), or_lerp(a.y, b.y, tx), or_lerp(a.z, b.z, tx));
    const v3 bot = V3(or_lerp(c.x, d.x, tx), or_lerp(c.y, d.y, tx), or_lerp(c.z, d.z, tx));
    return V3(or_lerp(top.x, bot.x, ty), or_lerp(top.y, bot.y, ty), or_lerp(top.z, bot.z, ty));
}
/* radiance from world direction d in the shading space of the pipeline (`color`: OR_COLOR_* bits): the texels are in its RGB space
 * and are converted as spectral_uplift converts an emission texture */
static inline v3 or_env_eval(const or_env *e, uint32_t color, v3 d) {
    float st;
    v3 c = or_env_lookup(e, or_env_uv(or_env_local(e, d), &st));
    float a[3] = {c.x, c.y, c.z};
    or_cs_convert(a, (color & OR_COLOR_RGB_ACES) != 0, (color & OR_COLOR_REPR_ACES) != 0);
    return V3(a[0], a[1], a[2]);
}
/* the solid-angle pdf: ((p_row p_col) ((f32)W (f32)H)) / ((2 pi pi) sin(theta)) */
static inline float or_env_pdf_of(const or_env *e, float p_row, float p_col, float sin_theta) {
    const float two_pi2 = 2.0f * OR_PI * OR_PI;
    return (p_row * p_col) * ((float)e->w * (float)e->h) / (two_pi2 * sin_theta);
}
/* 0 where sin(theta) is not > 0 (the poles, a NaN direction) */
static inline float or_env_pdf(const or_env *e, v3 d) {
    float st;
    const v2 uv = or_env_uv(or_env_local(e, d), &st);
    if (!(st > 0.0f)) return 0.0f;
    const int x = or_env_index(uv.x, e->w), y = or_env_index(uv.y, e->h);
    return or_env_pdf_of(e, e->marginal.pdf[y], e->conditional[y].pdf[x], st);
}
/* u.y picks the row, u.x the column (alias tables, remapped remainders); the point in the texel at u = (x + rx) / W,
 * v = (y + ry) / H; wi = R (cos(lat) cos(phi), sin(lat), cos(lat) sin(phi)), phi = (u - 0.5) 2 pi, lat = (v - 0.5) pi.
 * Valid when cos(lat) > 0 and the pdf is finite and > 0. */
static inline int or_env_sample(const or_env *e, v2 u, v3 *wi, float *pdf) {
    float p_row, p_col, ry, rx;
    const uint32_t y = or_alias_sample_and_remap(&e->marginal, u.y, &p_row, &ry);
    const uint32_t x = or_alias_sample_and_remap(&e->conditional[y], u.x, &p_col, &rx);
    const float uu = ((float)x + rx) / (float)e->w, vv = ((float)y + ry) / (float)e->h;
    float sp, cp, sl, cl;
    or_sincosf((uu - 0.5f) * (2.0f * OR_PI), &sp, &cp);
    or_sincosf((vv - 0.5f) * OR_PI, &sl, &cl);
    *wi = or_env_world(e, V3(cl * cp, sl, cl * sp));
    *pdf = 0.0f;
    if (!(cl > 0.0f)) return 0;
    *pdf = or_env_pdf_of(e, p_row, p_col, cl);
    return or_isfinite(*pdf) && *pdf > 0.0f;
}
#endif
