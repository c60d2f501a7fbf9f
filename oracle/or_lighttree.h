/* or_lighttree.h -- the light tree of the CPU oracle (TEST INFRASTRUCTURE ONLY).
 *
 * A restatement of DESIGN.md section 4.16 (the reference has no light tree, so that section is the specification): the build over the
 * point and spot lights ("Build") and the walk a shading point makes with the number its light choice left ("Walk"), in f32 with
 * the operand order the section's block makes normative. It is written from that text, not from the library's sources, and calls
 * nothing of the library. The light table's one entry for the tree ("Light table with a tree") is made in akr_oracle.c.
 */
#ifndef OR_LIGHTTREE_H
#define OR_LIGHTTREE_H
#include "or_math.h"
#include "or_punct.h"
#include <stdlib.h>
#include <string.h>

#define OR_PUNCT_TREE_INST 0xfffffffdu /* what the light list reports as the instance of the tree's entry (4.16 "Light table with a tree") */
#define OR_LT_LEAF 0x80000000u
#define OR_LT_NO_RECORD 0xffffffffu
#define OR_LT_MAX_STEPS 32

/* 4.16 "Build", layout: lo.xyz, power | hi.xyz, child -- 32 bytes; child = the left child's index, or the leaf bit | record index */
typedef struct { v3 lo; float power; v3 hi; uint32_t child; } or_lt_node;

/* 4.16 "Which lights": the point and the spot lights, soft or delta; a sun has no position */
static inline int or_lt_is_local(const or_punct *r) { return r->kind != OR_LIGHT_SUN; }

static inline float or_lt_axis(v3 q, int axis) { return axis == 0 ? q.x : axis == 1 ? q.y : q.z; }

/* 4.16 "Build": the order of a range, by (q[axis], index in the order given) ascending; -0 == +0 is a tie. qsort takes no context, the
 * build is single-threaded by the section's word, so the key's operands sit here for the time of one sort. */
static const or_punct *g_or_lt_sort_records;
static int g_or_lt_sort_axis;
static int or_lt_compare(const void *a, const void *b) {
    const uint32_t ia = *(const uint32_t *)a, ib = *(const uint32_t *)b;
    const float qa = or_lt_axis(g_or_lt_sort_records[ia].q, g_or_lt_sort_axis), qb = or_lt_axis(g_or_lt_sort_records[ib].q, g_or_lt_sort_axis);
    if (qa < qb) return -1;
    if (qa > qb) return 1;
    return ia < ib ? -1 : ia > ib ? 1 : 0;
}

/* 4.16 "Build": records = every punctual record of the default pipeline in the order given, weights = their f32 selection weights
 * (4.14 "Light list"). Returns the 2 L - 1 nodes (the caller frees them) and their count, or NULL and 0 with fewer than two local lights. */
static or_lt_node *or_lt_build(const or_punct *records, const float *weights, uint32_t n_records, uint32_t *n_nodes) {
    *n_nodes = 0;
    uint32_t L = 0;
    for (uint32_t k = 0; k < n_records; k++) L += or_lt_is_local(&records[k]) ? 1u : 0u;
    if (L < 2) return 0;
    const uint32_t cap = 2 * L - 1;
    uint32_t *items = (uint32_t *)malloc(4ull * L);  /* the local lights; a node's range is items[start .. start + count) */
    uint32_t *start = (uint32_t *)malloc(4ull * cap), *count = (uint32_t *)malloc(4ull * cap);
    or_lt_node *nodes = (or_lt_node *)calloc(cap, sizeof(or_lt_node));
    for (uint32_t k = 0, m = 0; k < n_records; k++)
        if (or_lt_is_local(&records[k])) items[m++] = k;
    /* breadth-first from a queue: root = node 0; an inner node taken off the queue gives its children the next two indices */
    uint32_t n = 1;
    start[0] = 0; count[0] = L;
    for (uint32_t head = 0; head < n; head++) {
        uint32_t *range = items + start[head];
        const uint32_t c = count[head];
        if (c == 1) { nodes[head].child = OR_LT_LEAF | range[0]; continue; }
        /* the axis with the largest f32 extent max - min of the POSITIONS of the range; ties: the lowest axis */
        v3 mn = records[range[0]].q, mx = mn;
        for (uint32_t i = 1; i < c; i++) {
            const v3 q = records[range[i]].q;
            mn = V3(or_min(mn.x, q.x), or_min(mn.y, q.y), or_min(mn.z, q.z));
            mx = V3(or_max(mx.x, q.x), or_max(mx.y, q.y), or_max(mx.z, q.z));
        }
        const float ext[3] = {mx.x - mn.x, mx.y - mn.y, mx.z - mn.z};
        int axis = 0;
        if (ext[1] > ext[axis]) axis = 1;
        if (ext[2] > ext[axis]) axis = 2;
        g_or_lt_sort_records = records; g_or_lt_sort_axis = axis;
        qsort(range, c, sizeof(uint32_t), or_lt_compare);
        const uint32_t nl = (c + 1) / 2; /* the left child gets the first (n + 1) / 2 */
        nodes[head].child = n;
        start[n] = start[head]; count[n] = nl;
        start[n + 1] = start[head] + nl; count[n + 1] = c - nl;
        n += 2;
    }
    /* boxes and powers, children before their parent (they sit behind it): a leaf's box is q -+ radius per component in f32 and its power the
     * item's weight; an inner node's the componentwise min / max and left.power + right.power, one f32 addition */
    for (uint32_t k = n; k-- > 0;) {
        or_lt_node *N = &nodes[k];
        if (N->child & OR_LT_LEAF) {
            const or_punct *r = &records[N->child & ~OR_LT_LEAF];
            N->lo = V3(r->q.x - r->radius, r->q.y - r->radius, r->q.z - r->radius);
            N->hi = V3(r->q.x + r->radius, r->q.y + r->radius, r->q.z + r->radius);
            N->power = weights[N->child & ~OR_LT_LEAF];
        } else {
            const or_lt_node *A = &nodes[N->child], *B = &nodes[N->child + 1];
            N->lo = V3(or_min(A->lo.x, B->lo.x), or_min(A->lo.y, B->lo.y), or_min(A->lo.z, B->lo.z));
            N->hi = V3(or_max(A->hi.x, B->hi.x), or_max(A->hi.y, B->hi.y), or_max(A->hi.z, B->hi.z));
            N->power = A->power + B->power;
        }
    }
    free(items); free(start); free(count);
    *n_nodes = n;
    return nodes;
}

/* div_s(a, s) of two scalars (4.16 "Walk"): a . (1 / s), one IEEE division, one multiplication */
static inline float or_lt_div_s(float a, float s) { const float inv = 1.0f / s; return a * inv; }

/* 4.16 "Walk", importance(N, p): power over the squared distance to the box's centre, never below the box's squared half-diagonal */
static inline float or_lt_importance(const or_lt_node *N, v3 p) {
    const v3 c = v3scale(v3add(N->lo, N->hi), 0.5f);
    const v3 h = v3scale(v3sub(N->hi, N->lo), 0.5f);
    const float r2 = v3dot(h, h);
    const v3 d = v3sub(p, c);
    const float d2 = v3dot(d, d);
    return or_lt_div_s(N->power, or_max(d2, r2));
}

/* 4.16 "Walk": from the root with u = the remapped u_sel2 and *pdf = light_choice_pdf coming in. Returns 1 at a leaf (*record = its
 * record index, *pdf = the walked product), 0 when the 32-step bound was reached on an inner node (*record = the child word's low bits). */
static int or_lt_walk(const or_lt_node *nodes, v3 p, float u, float *pdf, uint32_t *record) {
    uint32_t child = nodes[0].child;
    float f = *pdf;
    for (int step = 0; step < OR_LT_MAX_STEPS && !(child & OR_LT_LEAF); step++) {
        const or_lt_node *A = &nodes[child], *B = &nodes[child + 1];
        const float wl = or_lt_importance(A, p), wr = or_lt_importance(B, p);
        const float s = wl + wr;
        float pl = or_lt_div_s(wl, s);
        if (!(s > 0.0f && or_isfinite(s))) pl = or_lt_div_s(A->power, A->power + B->power); /* the fallback: by the powers */
        pl = or_clamp(pl, 0x1p-16f, 1.0f - 0x1p-16f); /* no contributing light ever has probability 0 */
        if (u < pl) {
            child = A->child; f = f * pl; u = or_lt_div_s(u, pl);
        } else {
            const float qr = 1.0f - pl;
            child = B->child; f = f * qr; u = or_lt_div_s(u - pl, qr);
        }
        u = or_min(u, 0x1.fffffep-1f);
    }
    *pdf = f;
    *record = child & 0x7fffffffu;
    return (child & OR_LT_LEAF) != 0;
}
#endif
