// dlighttree.h -- the light tree over the point and spot lights of a scene (which is normative: every parenthesis below is an
// operand order). Compiled into the LTREE kernels (pt_punct_tree*_kernels.hip) only. The light table of a scene with a tree has ONE entry for all of them (LightRec.inst = kPunctTreeInst); a lane that the alias table sends
// there descends a balanced binary tree with the selection number it already drew, weighting the two children by power / distance^2 at its own shading
// point. No sampler dimension more, no MIS partner (no ray hits these lights). The nodes (host/scene_punct.cpp build_light_tree builds them) sit behind the DPunct records
// in the same device array: node k = the two float4 at punct + punct_tree records + 32 k bytes, `lo.xyz, power | hi.xyz, child`; the two children of an
// inner node are adjacent, so one step reads one 64-byte line. AKR_HD: the test hook akr_host_light_tree_sample runs this text on the host.
#pragma once
#include "dpunct.h"

namespace akr {

constexpr uint32_t kLightTreeLeafBit = 0x80000000u;  // LightTreeNode.child: a leaf, the low bits are the record's index in DScene.punct
constexpr int kLightTreeMaxSteps = 32;               // the walk's bound, whatever the array holds (a tree the host built is no deeper than 32)

struct LightTreeNode {
    vec3 lo;
    float power;
    vec3 hi;
    uint32_t child;  // inner: the left child's index (the right one is child + 1); leaf: kLightTreeLeafBit | record
};
AKR_HD LightTreeNode light_tree_node(const float4* __restrict__ nodes, uint32_t k) {
    const float4 a = nodes[2 * (size_t)k], b = nodes[2 * (size_t)k + 1];
    return LightTreeNode{mk3(a.x, a.y, a.z), a.w, mk3(b.x, b.y, b.z), f2u(b.w)};
}
// a / s := a * (1 / s), as dmath.h's div_s of a vector: one IEEE division and one multiplication
AKR_HD float div_s(float a, float s) { return a * rcp_f(s); }

// power over the squared distance from p to the node's centre, the distance taken as no less than the box's half diagonal: distance only -- no cone
// term of a spot, no cosine of the surface normal, so every light that can contribute keeps a positive probability
AKR_HD float light_tree_importance(const LightTreeNode& N, vec3 p) {
    const vec3 c = (N.lo + N.hi) * 0.5f;
    const vec3 h = (N.hi - N.lo) * 0.5f;
    const float r2 = dot(h, h);
    const vec3 d = p - c;
    const float d2 = dot(d, d);
    return div_s(N.power, max_f(d2, r2));
}
// From the root to a leaf with the number u (the u_sel2 the light table's alias step left); pdf comes in as the probability of the tree's entry and
// leaves multiplied by every level's. false: the bound was reached on an inner node (the sample is invalid; not on a tree the host built).
AKR_HD bool light_tree_walk(const float4* __restrict__ nodes, vec3 p, float u, float& pdf, uint32_t& record) {
    uint32_t child = light_tree_node(nodes, 0).child;
    for (int step = 0; step < kLightTreeMaxSteps && !(child & kLightTreeLeafBit); step++) {
        const LightTreeNode A = light_tree_node(nodes, child), B = light_tree_node(nodes, child + 1);
        const float wl = light_tree_importance(A, p), wr = light_tree_importance(B, p);
        const float s = wl + wr;
        float pl = div_s(wl, s);
        if (!(s > 0.0f && is_finite(s))) pl = div_s(A.power, A.power + B.power);
        pl = clamp_f(pl, 0x1p-16f, 1.0f - 0x1p-16f);
        if (u < pl) {
            child = A.child;
            pdf = pdf * pl;
            u = div_s(u, pl);
        } else {
            const float qr = 1.0f - pl;
            child = B.child;
            pdf = pdf * qr;
            u = div_s(u - pl, qr);
        }
        u = min_f(u, 0x1.fffffep-1f);
    }
    record = child & ~kLightTreeLeafBit;
    return (child & kLightTreeLeafBit) != 0;
}

// One row of the test hooks akr_host_light_tree_sample / akr_probe_light_tree_sample: punct_probe_row's row (in9 = p, n, u_select, u_sample -> out13 = li,
// wi, pdf, ro, tmax, valid, delta and the light chosen) over a scene that may have a tree (punct_tree != 0): an entry that says kPunctTreeInst is walked,
// out13[6] is the full pdf and *record_out the DPunct record the walk ended at; kInvalid where the entry was not the tree.
AKR_HD void light_tree_probe_row(const AliasPacked* light_alias, const LightRec* lights, const DPunct* punct, uint32_t punct_tree, uint32_t n_lights, const float* in9,
                                 float* out13, uint32_t* light_out, uint32_t* record_out) {
    for (int k = 0; k < 13; k++) out13[k] = 0.0f;
    *light_out = kInvalid;
    *record_out = kInvalid;
    if (n_lights == 0) return;
    float pdf, u_sel2;
    const uint32_t light = alias_sample_and_remap(light_alias, n_lights, in9[6], pdf, u_sel2);
    *light_out = light;
    out13[6] = pdf;
    const LightRec L = lights[light];
    if (L.inst != kPunctInst && L.inst != kPunctTreeInst) return;
    const vec3 p = mk3(in9[0], in9[1], in9[2]);
    uint32_t record = L.first_gid;
    bool walked = true;
    if (L.inst == kPunctTreeInst) {
        if (punct_tree == 0) return;
        walked = light_tree_walk((const float4*)(punct + punct_tree), p, u_sel2, pdf, record);
        out13[6] = pdf;
        *record_out = record;
        out13[12] = 1.0f;
        if (!walked) return;
    }
    const PunctSample s = punct_sample(punct[record], p, mk3(in9[3], in9[4], in9[5]), mk2(in9[7], in9[8]), true);
    out13[0] = s.li.x; out13[1] = s.li.y; out13[2] = s.li.z;
    out13[3] = s.wi.x; out13[4] = s.wi.y; out13[5] = s.wi.z;
    out13[7] = s.ro.x; out13[8] = s.ro.y; out13[9] = s.ro.z;
    out13[10] = s.tmax;
    out13[11] = s.valid ? 1.0f : 0.0f;
    out13[12] = 1.0f;
}

}  // namespace akr
