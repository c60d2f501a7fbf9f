// disect.h -- ray/triangle test and the two scene intersectors (exhaustive for tiny scenes, 6-wide compressed BVH of 64-byte nodes otherwise).
//
// Replaces LuisaCompute's rtx::Accel ray queries (crates/akari_render/src/scene.rs:88-185). Semantics kept from
// the reference: a candidate is rejected when its (inst, prim) equals one of the ray's two exclusion slots
// (scene.rs:98-100) or fails the stochastic alpha test (scene.rs:49-86); closest hit = smallest t.
// Added so that results do not depend on traversal order: ties in t go to the lowest global triangle id.
#pragma once
#include "drng.h"
#include "dscene.h"
#include "../kernels.h"  // CY_*: the columns of a carried traversal

namespace akr {

// compile-time flags passed to generic lambdas (the headers keep clear of <type_traits>: they are also compiled by hiprtc, which has no host headers)
template <bool V>
struct BoolTag {
    static constexpr bool value = V;
};

struct Hit {
    float t, u, v;
    uint32_t gid;
};

// Triangle test in Woop's precomputed-transform form. (r0|c0), (r1|c1), (r2|c2) map world space to the space in
// which the triangle is (0,0,0),(1,0,0),(0,1,0); 27 flops + one division, no cross products at run time.
struct PlaneHit {  // the plane solve: t and the hit point from the third row
    float t, px, py, pz;
};
AKR_HD PlaneHit tri_plane(vec3 o, vec3 d, float4 r2) {
    float dz = __builtin_fmaf(r2.x, d.x, __builtin_fmaf(r2.y, d.y, r2.z * d.z));
    float oz = __builtin_fmaf(r2.x, o.x, __builtin_fmaf(r2.y, o.y, __builtin_fmaf(r2.z, o.z, r2.w)));
    PlaneHit h;
    h.t = div_f(-oz, dz);
    h.px = __builtin_fmaf(h.t, d.x, o.x);
    h.py = __builtin_fmaf(h.t, d.y, o.y);
    h.pz = __builtin_fmaf(h.t, d.z, o.z);
    return h;
}
// the inside test: the two affine coordinates of the hit point in the triangle's frame, from the first two rows
AKR_HD void tri_uv(const PlaneHit& h, float4 r0, float4 r1, float& u, float& v) {
    u = __builtin_fmaf(r0.x, h.px, __builtin_fmaf(r0.y, h.py, __builtin_fmaf(r0.z, h.pz, r0.w)));
    v = __builtin_fmaf(r1.x, h.px, __builtin_fmaf(r1.y, h.py, __builtin_fmaf(r1.z, h.pz, r1.w)));
}
AKR_HD bool tri_test(vec3 o, vec3 d, float4 r0, float4 r1, float4 r2, float tmin, float tmax, float& t_out, float& u_out,
                     float& v_out) {
    PlaneHit h = tri_plane(o, d, r2);
    float u, v;
    tri_uv(h, r0, r1, u, v);
    t_out = h.t;
    u_out = u;
    v_out = v;
    return (h.t >= tmin) & (h.t <= tmax) & (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f);
}

// SvmEvalMode::Alpha for a texture-fed base colour (principled.rs:15-21): the graph at the candidate's uv
// (surface_interaction_for_alpha_test, mesh.rs:426-485), alpha = w of the node feeding base_color. Inlined on purpose: a
// call inside the triangle loop makes the compiler give up the scalar (SGPR) path of the wave-uniform record loads.
AKR_D float textured_alpha(const DScene& sc, const float4* r, uint32_t material, float u, float v) {
    float w = 1.0f - u - v;
    vec2 uv = mk2((r[0].w * w + r[2].w * u) + r[4].w * v, (r[1].w * w + r[3].w * u) + r[5].w * v);
    return material_alpha_at(sc.tex, sc.materials[material], material, uv);  // = w of the node feeding base_color
}
// scene.rs:49-86 for folded materials: alpha = alpha channel of the base-colour node
template <bool TEX>
AKR_D bool alpha_test(const DScene& sc, uint32_t gid, float u, float v) {
    const float4* r = sc.shade + (size_t)gid * SHADE_ROWS;
    float4 q6 = r[6];
    const DMaterial& m = sc.materials[f2u(q6.y)];
    float alpha = (m.kind == MAT_PRINCIPLED || m.kind == MAT_DIFFUSE) ? m.base_alpha : 1.0f;
    if (TEX) {  // only the TEX kernels carry the graph evaluation (and its scratch array)
        if (m.flags & MF_ALPHA_TEXTURED)
            alpha = textured_alpha(sc, r, f2u(q6.y), u, v);
    }
    if (alpha >= 1.0f) return true;
    uint32_t inst = f2u(q6.z);
    uint32_t prim = gid - sc.inst_tri_offset[inst];
    float h = (float)xxhash32_4(inst, prim, f2u(u), f2u(v)) * 2.3283064365386963e-10f;
    return alpha > h;
}

// The five conditions of the test as ONE number: inside the triangle and inside (0, tmax) <=> margin >= 0. For finite values
// this is the comparison chain of tri_test exactly (a - b >= 0 <=> a >= b in IEEE arithmetic, and the minimum of numbers
// is >= 0 iff all of them are); a NaN t makes u, v and every operand NaN, and NaN >= 0 is false, as in the chain. Why: each
// comparison of the chain leaves a lane mask in SGPRs and the masks are combined on the scalar unit, which the four SIMDs of a
// CU share -- at 60 scalar instructions per record the loops below were bound by that unit, not by the VALU.
AKR_D float next_up(float x) {  // the next float above a finite x
    uint32_t b = f2u(x);
    return x > 0.0f ? u2f(b + 1u) : (x < 0.0f ? u2f(b - 1u) : u2f(1u));
}
AKR_D float hit_margin(float t, float u, float v, float tmax) {
    // (v_min3_f32 instead of two v_min_f32 was measured in round 4: a min3 costs two issue slots, -1.3 %; profiles/r4_ab_walk.txt)
    return __builtin_fminf(__builtin_fminf(__builtin_fminf(u, v), 1.0f - (u + v)), __builtin_fminf(t, tmax - t));
}

// Exhaustive intersector: every lane of the wave walks the same triangle list, so the 48-byte records are
// wave-uniform and come in through the scalar cache (s_load_dwordx4 x3), leaving the VALU for the test itself.
template <bool ANY_HIT, bool TEX = false>
AKR_D bool trace_exhaustive(const DScene& sc, vec3 o, vec3 d, float tmin, float tmax, uint32_t ex0, uint32_t ex1, Hit& hit) {
    float best_t = next_up(tmax);  // see trace_pair_exhaustive
    uint32_t best = kInvalid;
    float best_u = 0.0f, best_v = 0.0f;
    const uint32_t n = sc.n_tris;
    // constant address space (4) + wave-uniform index => s_load_dwordx4 into SGPRs; the records are read-only for
    // the whole launch, which is what makes the scalar (non-coherent) cache legal here
    typedef const float __attribute__((address_space(4))) * ConstF;
    ConstF recs = (ConstF)(uintptr_t)sc.woop;
    auto load_rec = [&](uint32_t k, float4& a, float4& b, float4& c) {
        ConstF r = recs + 12 * (size_t)k;
        a = make_float4(r[0], r[1], r[2], r[3]);
        b = make_float4(r[4], r[5], r[6], r[7]);
        c = make_float4(r[8], r[9], r[10], r[11]);
    };
    // software prefetch: the record of triangle k+1 is requested before triangle k is tested, so the scalar-cache
    // latency overlaps the ~40 VALU instructions of the test (the buffer is padded by one record, scene_build.cpp)
    float4 n0, n1, n2;
    load_rec(0, n0, n1, n2);
    PlaneHit ph{0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < n; k++) {
        const float4 r0 = n0, r1 = n1, r2 = n2;
        load_rec(k + 1, n0, n1, n2);
        if (!((sc.plane_share_mask >> k) & 1ull)) ph = tri_plane(o, d, r2);  // wave-uniform: one solve per coplanar pair of records
        float u, v;
        const float t = ph.t;
        tri_uv(ph, r0, r1, u, v);
        float m = __builtin_fminf(hit_margin(t, u, v, tmax), t - tmin);
        m = (k == ex0) ? -1.0f : m;
        m = (k == ex1) ? -1.0f : m;
        if (sc.has_alpha) {
            if (m >= 0.0f && !alpha_test<TEX>(sc, k, u, v)) m = -1.0f;
        }
        if (ANY_HIT) {
            if (m >= 0.0f) best = k;
            if (__builtin_amdgcn_ballot_w64(best == kInvalid) == 0) break;  // every lane of the wave is occluded
        } else {
            // ascending k: a strict '<' keeps the lowest id among equal t
            const float tc = (m >= 0.0f) ? t : __builtin_inff();
            const bool better = tc < best_t;
            best_t = better ? tc : best_t;
            best_u = better ? u : best_u;
            best_v = better ? v : best_v;
            best = better ? k : best;
        }
    }
    hit.t = best != kInvalid ? best_t : tmax;
    hit.u = best_u;
    hit.v = best_v;
    hit.gid = best;
    return best != kInvalid;
}

// Exhaustive intersector for a PAIR of rays per lane: the closest-hit ray of the next path vertex and the shadow ray
// of the current one are both known once a vertex has been shaded, so one walk over the records serves both: half the
// loads and loop overhead of two separate walks, and two independent dependency chains per record for the VALU to
// overlap. A ray that does not exist for a lane is passed with tmax < tmin and can never hit.
//
// The records are read from LDS (`lds_recs`: pt_pass.h stages them behind the shading tables, padded by two records): every lane reads
// the same address, a broadcast ds_read_b128, so all of the test's arithmetic is VGPR-only. A SIMD accepts one scalar-operand VALU
// instruction per ~4.3 cycles against ~2.15 for a VGPR-only one (tools/micro/valu_rate.hip), and the rows of a record read through the
// scalar cache come 16 such instructions in a row. The bookkeeping per record is cut down too (a v_cmp costs 4.4 cycles and a v_cndmask
// on its result 3.7): the alpha test is unswitched out of the loop, min / max come without the compiler's canonicalising v_max x, x, the
// shadow ray's margin is folded with one v_max, and only (t, id) of the best hit are selected per record -- its (u, v) are recomputed
// once after the walk. Operations whose result nothing reads are left out (profiles/walk_unread_ops.md): the closest-hit ray's margin has
// no tmax - t where no alpha test reads the margin (t < best_t says it), the shadow ray's range term min(t, stmax - t) is computed with
// its plane solve, not per record, and the best hit is chosen by one test and two selects. Two records per trip on alternating register
// sets: a one-record software prefetch without the moves that rotating a single set costs. In the walk without an alpha test a trip's
// bookkeeping is shared by its two records (WalkOpt PLANE_LT, PLANE_EXCL below): one comparison per excluded id, and one t < best_t where
// the records share a plane -- 6 v_cmp and 5 v_cndmask per trip for 10 and 6. The id of the best hit is kept as the trip's even id and a
// lane mask for "its second record" (HALF_MASK: one select and one v_mov per trip for two and two), and the trip's six LDS reads take one
// address register (ONE_ADDR: one v_add per trip for two v_mov).
// Five other forms were measured and retired (records through the scalar cache, both rays packed into v_pk_fma_f32 with and
// without op_sel broadcast, lockstep pairs of coplanar records); this one was +4.2 % on C2 and +3.3 % on C3 over the next best:
// HISTORY.md, profiles/r4_ab_walk.txt. The arithmetic (operation order, fma placement) is tri_plane / tri_uv / hit_margin's.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
// IEEE minNum / maxNum as the instruction computes them, without the v_max x, x the compiler puts in front of fminf / fmaxf to quiet
// a possible signalling NaN (4.4 cycles of the SIMD each, tools/micro/vgpr_bank.hip; arithmetic never produces one)
AKR_D float min_raw(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
AKR_D float max_raw(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// min(a, |b|), one instruction (the abs is a source modifier)
AKR_D float min_abs_raw(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// max(|a|, |b|, |c|); a NaN operand is ignored (maxNum)
AKR_D float max3_abs_raw(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// A truth value per lane as a mask in a scalar register pair, and back: Boolean algebra written on such masks stays on the scalar unit
// (lanes that are switched off read as 0)
AKR_D uint64_t lanes_of(bool c) { return __builtin_amdgcn_ballot_w64(c); }
AKR_D bool in_lanes(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// tri_plane with the division's range-scaling steps left out (dmath.h div_f_unscaled), and the smallest |numerator| seen so far in `lo`
AKR_D PlaneHit tri_plane_unscaled(vec3 o, vec3 d, float4 r2, float& lo) {
    float dz = __builtin_fmaf(r2.x, d.x, __builtin_fmaf(r2.y, d.y, r2.z * d.z));
    float oz = __builtin_fmaf(r2.x, o.x, __builtin_fmaf(r2.y, o.y, __builtin_fmaf(r2.z, o.z, r2.w)));
    lo = min_abs_raw(lo, oz);
    PlaneHit h;
    h.t = div_f_unscaled(-oz, dz);
    h.px = __builtin_fmaf(h.t, d.x, o.x);
    h.py = __builtin_fmaf(h.t, d.y, o.y);
    h.pz = __builtin_fmaf(h.t, d.z, o.z);
    return h;
}

// The shortcuts of the pair walk, all bit-neutral, switched per instantiation of the walk (what UNSCALED_DIV buys where:
// profiles/walk_div_mask_ab.md).
//
// UNSCALED_DIV -- speculate and validate. The plane solves use div_f_unscaled (8 instructions for the compiler's 12; dmath.h says on which
// set S of operands it is the contract's quotient). Whether a solve's operands are in S is not tested per solve -- a compare and a branch
// would cost what the shortcut saves -- but once per walk, and a wave with a lane that fails repeats the walk with the compiler's division
// (walk_ieee below: rolled, one record per trip; it runs in a vanishing share of the walks) and takes that result. What is checked, per
// ray that exists (tmax >= 0; a ray that does not exist is never accepted whatever its t: the shadow ray because min(t, stmax - t) < 0 or NaN
// for stmax < 0, the closest-hit ray because its margin >= 0 needs t >= 0 and t < best_t needs t <= tmax < 0):
//   before the walk   |o| <= B and |d| <= 2 per component, tmax <= 1e20. The host chose B (dscene.h walk_bound_word) so that under these
//                     bounds every plane row of the scene gives |oz| < 2^46 and |dz| < 2^46 (api_scene.cpp; a negative bound = no such
//                     bound exists, the scene always takes walk_ieee). A NaN component passes the test (maxNum ignores it), harmlessly:
//                     it makes oz or dz NaN for EVERY row (0 * NaN = NaN), t is NaN on either path and no record is accepted on either.
//   after the walk    lo = the smallest |oz| over the solves >= 2^-47. (One v_min_f32 per solve. A zero numerator must not stay:
//                     the sequence returns +0 for -0 / b where IEEE gives -0.)
// Why that suffices. For a solve of a checked lane, a = -oz and b = dz have 2^-47 <= |a| < 2^47 and |b| < 2^47. Of the conditions of S,
// "a's biased exponent >= 24" holds (it is >= 80), "|b| <= 2^125" holds, and exp(a) - exp(b) >= -47 - 46 > -125. So (a, b) can leave S
// only through b zero or denormal, or through exp(a) - exp(b) >= 96. In both cases the exact quotient has |t| > 2^79 (|a| >= 2^-47 over
// |b| < 2^-126; or 2^(96 - 1)), which is > 1e20 >= tmax: IEEE's quotient (+-inf for b = 0) fails the range test, the record is
// rejected. The unscaled sequence returns for such a pair a value of magnitude > 1e20, +-inf or NaN (checked on the device for both kinds
// of exit, tests/test_gpu_div_unscaled.py), which fails the same test. The range test is, for the shadow ray and for the closest-hit ray
// of a walk with an alpha test, min(t, tmax - t) >= 0: false for |t| > tmax and for NaN. For the closest-hit ray of a walk without one it
// is (t >= 0) & (t < best_t), the margin's last operand being t alone (tmax - t is left out: best_t starts at next_up(tmax) and only
// decreases, so t < best_t implies t <= tmax and fl(tmax - t) >= 0 -- the term could only have lowered a margin whose record fails
// t < best_t anyway): a positive |t| > 1e20 fails t < best_t (best_t <= next_up(1e20)), a negative one fails t >= 0, and for t = NaN
// every operand of the margin is NaN and every comparison false. The record is
// rejected on both paths, and no bit of its t reaches the result: best_t, the recomputed (u, v) and the sign of occ_margin come from
// accepted records only, whose pairs are in S.
// (The alpha walks keep tmax - t in the margin because they read it once more: alpha_test is guarded by m >= 0 and must not be evaluated at
// the (u, v) of a record beyond tmax.)
// (tmax and stmax are taken to be numbers: a NaN would read as "the ray does not exist" and skip the checks while min(t, NaN) = t could still
// accept a record. The callers pass 1e20, -1 or a light sample's distance, which is finite by construction: dpath.h sample_direct.)
// (Measured with it and retired: the excluded ids as bit masks, v_bfe_i32 + v_or on the margin's bits per ray and record in place of the
// comparisons below -- the compiler already folds the three comparisons into three v_cmp and one v_cndmask; -1.7 % on C2, same file.)
//
// PLANE_LT, PLANE_EXCL -- the bookkeeping of a two-record trip once per trip, not once per record (profiles/walk_plane_bookkeeping.md;
// what each buys: profiles/walk_plane_bookkeeping_ab.md). Both apply to the two-record trips of the walk without an alpha test only; the
// odd last record, the alpha walks and walk_ieee keep the per-record code. The arithmetic -- the solves, (u, v), the margins -- is the
// per-record code's, operation for operation; only Boolean combinations of its comparisons change, and those are written as lane masks
// (lanes_of / in_lanes) so that they run on the scalar unit.
//   PLANE_LT    A trip whose second record takes the plane of its first (plane_share_mask bit k + 1 set): both records see the same T and
//               the same best_t on entry, b0. With A, B = "margin >= 0 and not excluded" of the first and the second record, the per-record
//               code computes better_a = A & (T < b0), then better_b = B & (T < b1) with b1 = better_a ? T : b0. Where better_a holds, b1 = T
//               and T < T is false; elsewhere b1 = b0. So better_b = B & !better_a & (T < b0): one comparison lt = (T < b0) serves both
//               records, and best_t = ((A | B) & lt) ? T : b0 is one select. (A NaN T makes lt false, as it made both comparisons.) The id is
//               selected for the second record first and for the first one over it: k wins over k + 1, the lowest-id rule among equal t.
//               A trip whose second record solves a plane of its own chooses the first record per record, before that solve, and runs the
//               same text with A = 0 (nothing left to choose for the first record): one more select there, and one text for the compiler.
//   PLANE_EXCL  Per excluded id e (ex0, sex0, sex1), once per walk: q = e | 1 and the lane mask H = "e is odd". Every trip starts at an even
//               k (the loop steps by two from 0), so e is k or k + 1 exactly if q == k + 1 -- one comparison E -- and then the first record
//               is the excluded one where E & !H, the second where E & H. kInvalid | 1 = 0xffffffff equals no k + 1 <= 64. Three comparisons
//               per trip for six, whether the two records share a plane or not.
//
// HALF_MASK, ONE_ADDR -- instructions taken out of the two-record trip of the walk without an alpha test (profiles/walk_half_mask.md; what each
// buys: profiles/walk_half_mask_ab.md). Neither touches a comparison or a float.
//   HALF_MASK   (with PLANE_LT) The mask upd = (A | B) & lt that selects best_t already says that the trip wins; only which of its two records
//               did is new, one bit per lane. So during the loop `best` is the even id k of the winning trip -- one select on upd -- and
//               the lane mask `half`, in a scalar register pair, holds the bit: half = (half & ~upd) | (B & ~A & lt). A lane in both A and B
//               takes the first record (k wins over k + 1 at one t: the lowest-id rule), so its bit is clear. A trip whose second record
//               solves a plane of its own chooses its first record before that solve (choose), which clears `half` for the lanes it updates,
//               and runs the merged text with A = 0. After the loop best |= half, once: `half` is set under upd only, where `best` is an
//               even id, so kInvalid stays kInvalid. The tail record and the (u, v) of the hit read the id after that.
//   ONE_ADDR    The LDS byte address of the trip's first record in one VGPR, advanced by 96 per trip; the trip's six ds_read_b128 (its
//               second record, and the next trip's first) are immediate offsets 48 .. 128 from it. Left to the compiler the address lives
//               in an SGPR and is copied into a VGPR twice per trip.
#ifndef AKR_WALK_PLANE_LT
#define AKR_WALK_PLANE_LT 1  // (0 / 1 from the command line: an A/B build of one part, akari_render_amd/build.py build_variant)
#endif
#ifndef AKR_WALK_PLANE_EXCL
#define AKR_WALK_PLANE_EXCL 1
#endif
#ifndef AKR_WALK_HALF_MASK
#define AKR_WALK_HALF_MASK 1  // (0 / 1 from the command line, like the two above)
#endif
#ifndef AKR_WALK_ONE_ADDR
#define AKR_WALK_ONE_ADDR 1
#endif
template <bool DIV, bool LT = DIV && AKR_WALK_PLANE_LT, bool EXCL = DIV && AKR_WALK_PLANE_EXCL, bool HALF = LT && AKR_WALK_HALF_MASK, bool ADDR = DIV && AKR_WALK_ONE_ADDR>
struct WalkOpt {
    static constexpr bool unscaled_div = DIV;
    static constexpr bool plane_lt = LT;
    static constexpr bool plane_excl = EXCL;
    static constexpr bool half_mask = HALF && LT;
    static constexpr bool one_addr = ADDR;
};
template <int V>
struct IntTag {
    static constexpr int value = V;
};

template <bool TEX = false, class OPT = WalkOpt<true>>
AKR_D void trace_pair_exhaustive(const DScene& sc, vec3 o, vec3 d, float tmax, uint32_t ex0, vec3 so, vec3 sd, float stmax,
                                 uint32_t sex0, uint32_t sex1, Hit& hit, bool& found, bool& occluded, const float4* lds_recs, uint32_t* took_ieee_walk = nullptr) {
    constexpr bool UNSCALED = OPT::unscaled_div && !AKR_RX;
    // best_t starts one ulp above tmax: "t < best_t" then admits a first hit at t == tmax and keeps, among equal t, the
    // lowest id afterwards (ascending k, strict '<') without a separate "no hit yet" test
    float best_t = next_up(tmax);
    uint32_t best = kInvalid;
    float best_u = 0.0f, best_v = 0.0f;
    float occ_margin = -1.0f;  // max over the records of the shadow ray's margin: >= 0 <=> something occludes
    const uint32_t n = sc.n_tris;
    const v4f* lrec = (const v4f*)lds_recs;
    const bool has_alpha = __builtin_amdgcn_readfirstlane((int)sc.has_alpha) != 0;  // (a scalar branch per walk, nothing per lane)
    // the two rays' plane solves of the current plane: the hit points as pairs {closest-hit ray, shadow ray}; of the distances, the
    // closest-hit ray's t and the shadow ray's range term min(t, stmax - t) -- all a record reads of the shadow ray's t, so it is computed
    // once per solve and a record that takes its neighbour's plane spends nothing on it
    float T = 0.0f, srange = 0.0f;
    v2f hx2 = {0.0f, 0.0f}, hy2 = {0.0f, 0.0f}, hz2 = {0.0f, 0.0f};
    float lo = __builtin_inff(), slo = __builtin_inff();  // UNSCALED: the smallest |oz| of the walk, per ray
    // alpha_tag: 0 = no alpha test, 1 = alpha test, 2 = has_alpha decides at run time; div_tag: the plane solves use div_f_unscaled
    auto solve = [&](auto div_tag, const v4f& q2) {
        constexpr bool FAST = decltype(div_tag)::value;
        const float4 r2 = make_float4(q2.x, q2.y, q2.z, q2.w);
        const PlaneHit a = FAST ? tri_plane_unscaled(o, d, r2, lo) : tri_plane(o, d, r2), b = FAST ? tri_plane_unscaled(so, sd, r2, slo) : tri_plane(so, sd, r2);
        T = a.t;
        srange = min_raw(b.t, stmax - b.t);
        hx2 = (v2f){a.px, b.px}; hy2 = (v2f){a.py, b.py}; hz2 = (v2f){a.pz, b.pz};
    };
    // the margins of one record against the current plane's solves, before the exclusions: m the closest-hit ray's, sm the shadow ray's
    auto margins = [&](auto alpha_tag, const v4f& q0, const v4f& q1, v2f& u2, v2f& v2, float& m, float& sm) {
        constexpr int ALPHA = decltype(alpha_tag)::value;
        float u, v, su, sv;
        tri_uv(PlaneHit{T, hx2.x, hy2.x, hz2.x}, make_float4(q0.x, q0.y, q0.z, q0.w), make_float4(q1.x, q1.y, q1.z, q1.w), u, v);
        tri_uv(PlaneHit{0.0f, hx2.y, hy2.y, hz2.y}, make_float4(q0.x, q0.y, q0.z, q0.w), make_float4(q1.x, q1.y, q1.z, q1.w), su, sv);
        u2 = (v2f){u, su}; v2 = (v2f){v, sv};
        // hit_margin per ray: min(min(min(u, v), 1 - (u + v)), range), with the range terms described above the WalkOpt struct
        const v2f s2 = {1.0f - (u2.x + v2.x), 1.0f - (u2.y + v2.y)};
        const float range = ALPHA == 0 ? T : min_raw(T, tmax - T);
        m = min_raw(min_raw(min_raw(u2.x, v2.x), s2.x), range);
        sm = min_raw(min_raw(min_raw(u2.y, v2.y), s2.y), srange);
    };
    auto record = [&](auto alpha_tag, auto div_tag, uint32_t k, const v4f& q0, const v4f& q1, const v4f& q2) {
        constexpr int ALPHA = decltype(alpha_tag)::value;
        if (!((sc.plane_share_mask >> k) & 1ull)) solve(div_tag, q2);  // wave-uniform: one plane solve per ray per coplanar pair of records
        v2f u2, v2;
        float m, sm;
        margins(alpha_tag, q0, q1, u2, v2, m, sm);
        m = (k == ex0) ? -1.0f : m;
        sm = (k == sex0) ? -1.0f : sm;
        sm = (k == sex1) ? -1.0f : sm;
        if (ALPHA == 1 || (ALPHA == 2 && has_alpha)) {
            // k through readfirstlane: opaque to loop strength reduction, which otherwise keeps this block's record pointer and
            // hash constant as induction variables updated on the scalar unit every trip
            const uint32_t ka = __builtin_amdgcn_readfirstlane(k);
            if (m >= 0.0f && !alpha_test<TEX>(sc, ka, u2.x, v2.x)) m = -1.0f;
            if (sm >= 0.0f && !alpha_test<TEX>(sc, ka, u2.y, v2.y)) sm = -1.0f;
        }
        // only the distance and the id of the best hit are tracked here; its (u, v) are recomputed after the walk (below)
        // (one test, two selects: "m >= 0 ? t : inf" in front of the comparison would be a third select per record for the same truth
        // value -- inf < best_t is false, a NaN t has a NaN margin)
        const bool better = (m >= 0.0f) & (T < best_t);
        best_t = better ? T : best_t;
        best = better ? k : best;
        // max over the records of the shadow ray's margin (a NaN margin leaves it as it is, like the comparison it replaces; only
        // the sign of the result is read)
        occ_margin = max_raw(occ_margin, sm);
    };
    // The loop exists twice, with and without the alpha test of a candidate: left as a run-time branch inside ONE loop, the
    // (wave-uniform) flag is turned into a lane mask and back by every record of every scene -- a v_cndmask and a v_cmp, 8.8
    // cycles of 240 -- to merge the two values of the margins behind the branch.
    auto walk = [&](auto alpha_tag) {
        const BoolTag<UNSCALED> div_tag{};
        // the plane-wise bookkeeping (WalkOpt PLANE_LT, PLANE_EXCL): only in the walk without an alpha test
        constexpr bool PLANE_LT = OPT::plane_lt && decltype(alpha_tag)::value == 0, PLANE_EXCL = OPT::plane_excl && decltype(alpha_tag)::value == 0;
        constexpr bool HALF = OPT::half_mask && PLANE_LT, ONE_ADDR = OPT::one_addr && decltype(alpha_tag)::value == 0;
        v4f a0 = lrec[0], a1 = lrec[1], a2 = lrec[2], b0, b1, b2;
        uint32_t k = 0;
        if (PLANE_LT || PLANE_EXCL || ONE_ADDR) {
            // One body for every trip (a second copy of the trip for the pairs alone made the register allocator keep the plane's
            // solves twice and spill). Truth values are lane masks in scalar registers, written as such (lanes_of / in_lanes): left as
            // bools, the compiler turns part of the mask algebra into 0 / 1 VGPRs with a select and a comparison each.
            const uint32_t qex0 = ex0 | 1u, qsex0 = sex0 | 1u, qsex1 = sex1 | 1u;                                           // the trip an excluded id falls into ...
            const uint64_t hex0 = lanes_of((ex0 & 1u) != 0), hsex0 = lanes_of((sex0 & 1u) != 0), hsex1 = lanes_of((sex1 & 1u) != 0);  // ... and the half of it
            uint64_t half = 0;  // HALF_MASK: the lanes whose best hit is the second record of its trip (`best` holds the trip's even id meanwhile)
            auto choose = [&](uint64_t acc, uint32_t id) {  // the per-record choice: record()'s
                const uint64_t better = acc & lanes_of(T < best_t);
                best_t = in_lanes(better) ? T : best_t;
                best = in_lanes(better) ? id : best;
                if (HALF) half &= ~better;  // (called with a trip's first record only where HALF is on)
            };
            // ONE_ADDR: the LDS byte address of the trip's first record in a vector register of its own (what a ds_read takes), advanced once
            // per trip; the trip's six reads are immediate offsets from it. (Opaque to the compiler in every trip: left to itself it keeps the
            // address on the scalar unit and copies it into a vector register twice per trip; given a vector register that it may rebase, it
            // counts from the trip's last read backwards -- negative offsets, which a ds_read has not, so one v_add per read.)
            uint32_t rec_addr = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) v4f*)lrec;
            auto rec_row = [&](uint32_t k_rec, uint32_t rel, uint32_t row) -> v4f {  // row `row` of record k_rec + rel, k_rec the trip's first
                if (ONE_ADDR) return *(const __attribute__((address_space(3))) v4f*)(uintptr_t)(rec_addr + 48u * rel + 16u * row);
                return lrec[3 * (k_rec + rel) + row];
            };
            for (; k + 1 < n; k += 2, rec_addr += 96u) {
                if (ONE_ADDR) asm("" : "+v"(rec_addr));
                b0 = rec_row(k, 1, 0); b1 = rec_row(k, 1, 1); b2 = rec_row(k, 1, 2);
                const uint32_t k1 = k + 1;
                const bool own_b = !((sc.plane_share_mask >> k1) & 1ull);  // wave-uniform: the second record solves a plane of its own
                uint64_t xa, xb, sxa, sxb;  // the lanes whose closest-hit ray excludes the first / the second record; whose shadow ray does
                if (PLANE_EXCL) {  // (k is even in every trip, whether the records share a plane or not)
                    const uint64_t e = lanes_of(qex0 == k1), s0 = lanes_of(qsex0 == k1), s1 = lanes_of(qsex1 == k1);
                    xa = e & ~hex0; xb = e & hex0;
                    sxa = (s0 & ~hsex0) | (s1 & ~hsex1); sxb = (s0 & hsex0) | (s1 & hsex1);
                } else {
                    xa = lanes_of(k == ex0); xb = lanes_of(k1 == ex0);
                    sxa = lanes_of(k == sex0) | lanes_of(k == sex1); sxb = lanes_of(k1 == sex0) | lanes_of(k1 == sex1);
                }
                v2f u2, v2;
                float ma, sma, mb, smb;
                if (!((sc.plane_share_mask >> k) & 1ull)) solve(div_tag, a2);
                margins(alpha_tag, a0, a1, u2, v2, ma, sma);
                sma = in_lanes(sxa) ? -1.0f : sma;
                uint64_t acc_a = lanes_of(ma >= 0.0f) & ~xa;
                a0 = rec_row(k, 2, 0); a1 = rec_row(k, 2, 1); a2 = rec_row(k, 2, 2);
                if (!PLANE_LT) choose(acc_a, k);
                if (own_b) {
                    if (PLANE_LT) {  // the first record is chosen on its own T, before the second one's solve overwrites it, and is settled
                        choose(acc_a, k);
                        acc_a = 0;
                    }
                    solve(div_tag, b2);
                }
                margins(alpha_tag, b0, b1, u2, v2, mb, smb);
                smb = in_lanes(sxb) ? -1.0f : smb;
                const uint64_t acc_b = lanes_of(mb >= 0.0f) & ~xb;
                if (PLANE_LT) {
                    // both records on one T and one best_t (or the first one settled: acc_a = 0): one comparison, one select of best_t -- the
                    // identity above the WalkOpt struct. One text for both kinds of trip: two made the compiler carry T < best_t into them as a 0 / 1 VGPR.
                    const uint64_t lt = lanes_of(T < best_t);
                    const uint64_t upd = (acc_a | acc_b) & lt;  // the trip wins ...
                    best_t = in_lanes(upd) ? T : best_t;
                    if (HALF) {  // ... and which half of it did is a bit per lane: the second one only where the first did not accept
                        best = in_lanes(upd) ? k : best;
                        half = (half & ~upd) | (acc_b & ~acc_a & lt);
                    } else {
                        best = in_lanes(acc_b & lt) ? k1 : best;
                        best = in_lanes(acc_a & lt) ? k : best;
                    }
                } else {
                    choose(acc_b, k1);
                }
                occ_margin = max_raw(max_raw(occ_margin, sma), smb);
            }
            if (HALF) best |= in_lanes(half) ? 1u : 0u;  // (kInvalid stays: `half` is set under `upd` only, where `best` is an even id)
        } else {
            for (; k + 1 < n; k += 2) {
                b0 = lrec[3 * (k + 1)]; b1 = lrec[3 * (k + 1) + 1]; b2 = lrec[3 * (k + 1) + 2];
                record(alpha_tag, div_tag, k, a0, a1, a2);
                a0 = lrec[3 * (k + 2)]; a1 = lrec[3 * (k + 2) + 1]; a2 = lrec[3 * (k + 2) + 2];
                record(alpha_tag, div_tag, k + 1, b0, b1, b2);
            }
        }
        if (k < n) record(alpha_tag, div_tag, k, a0, a1, a2);
    };
    // the same walk with the compiler's division, kept small: one record per trip, the alpha flag read at run time
    auto walk_ieee = [&] {
        best_t = next_up(tmax); best = kInvalid; occ_margin = -1.0f;
#pragma clang loop unroll(disable)
        for (uint32_t k = 0; k < n; k++) {
            record(IntTag<2>{}, BoolTag<false>{}, k, lrec[3 * k], lrec[3 * k + 1], lrec[3 * k + 2]);
        }
    };
    if (UNSCALED) {
        const float ob = lds_recs[3u * (n + 1u) + 2u].w;  // dscene.h walk_bound_word: the last word of the records' padding
        const bool pre_bad = ((tmax >= 0.0f) & !((max3_abs_raw(o.x, o.y, o.z) <= ob) & (max3_abs_raw(d.x, d.y, d.z) <= 2.0f) & (tmax <= 1e20f))) |
                             ((stmax >= 0.0f) & !((max3_abs_raw(so.x, so.y, so.z) <= ob) & (max3_abs_raw(sd.x, sd.y, sd.z) <= 2.0f) & (stmax <= 1e20f)));
        bool redo = __builtin_amdgcn_ballot_w64(pre_bad) != 0;
        if (!redo) {
            if (has_alpha) walk(IntTag<1>{});
            else walk(IntTag<0>{});
            const bool bad = ((tmax >= 0.0f) & (lo < 0x1p-47f)) | ((stmax >= 0.0f) & (slo < 0x1p-47f));
            redo = __builtin_amdgcn_ballot_w64(bad) != 0;
        }
        if (redo) walk_ieee();
        if (took_ieee_walk) *took_ieee_walk = redo ? 1u : 0u;
    } else {
        if (has_alpha) walk(IntTag<1>{});
        else walk(IntTag<0>{});
        if (took_ieee_walk) *took_ieee_walk = 0u;
    }
    // (u, v) of the closest hit, once per walk instead of two selects per record: the record's rows from LDS again (a per-lane
    // address now) and the hit point o + t d with the t the walk kept -- the very operations on the very operands of the walk
    // (tri_plane's px = fma(t, d.x, o.x), tri_uv's fma chain over row 0), so the bits are the walk's.
    if (best != kInvalid) {
        const v4f q0 = lrec[3 * best], q1 = lrec[3 * best + 1];
        const float px = __builtin_fmaf(best_t, d.x, o.x), py = __builtin_fmaf(best_t, d.y, o.y), pz = __builtin_fmaf(best_t, d.z, o.z);
        best_u = __builtin_fmaf(q0.x, px, __builtin_fmaf(q0.y, py, __builtin_fmaf(q0.z, pz, q0.w)));
        best_v = __builtin_fmaf(q1.x, px, __builtin_fmaf(q1.y, py, __builtin_fmaf(q1.z, pz, q1.w)));
    }
    found = best != kInvalid;
    hit.t = found ? best_t : tmax;
    hit.u = best_u;
    hit.v = best_v;
    hit.gid = best;
    occluded = occ_margin >= 0.0f;
}

// ------------------------------------------------------------------------------------------------------------
// Compressed wide-BVH traversal: six children in eight octant positions, 64-byte nodes (layout and builder: host/bvh.cpp; after
// Ylitie, Karras & Laine, HPG 2017).
//
// One ray per lane. A lane's state is a NODE GROUP G = child_base (24 bits) | hit bits of the (at most 6) sibling nodes in their 8 octant
// positions, in visiting order (bits 24..31), a TRIANGLE GROUP (tbase, T) = the pending triangles of the node visited last (at most 18:
// six leaves of three; 24 bits), and a
// stack of node groups in LDS (strided by the workgroup size: lane i of every wave touches bank i). A node's children are
// tested together; those the ray enters become the new G, ordered by octant: slot s sits at bit 24 + (s ^ octinv), the
// highest bit is the nearest child, so "pop the nearest" is one count-leading-zeros and nothing is sorted. The siblings
// left over go to the stack as ONE entry: a traversal holds at most one entry per tree level and the stack
// (kBvhStackDepth levels, checked against the tree's depth when the scene is built) cannot overflow.
//
// Every step a lane does ONE thing -- test its next pending triangle, or fetch and test its next node -- and both kinds
// of lane fetch through the SAME four 16-byte loads from a per-lane address (64-byte triangle record: Woop rows + global
// id; 64-byte node: one memory sector each). The wave waits once per step whatever mix of nodes and triangles its lanes are at: on the
// 10 M-triangle hall round 1's while-while loop over a 4-wide BVH ran at 26 % lane utilisation, all of it waiting on dependent
// fetches.
// The box test only culls and does not have to follow the AKR-F32 contract (the oracle has no BVH): it must be conservative,
// which the padding of the boxes (host/bvh.cpp) guarantees; so it may use v_rcp_f32, fma and min3 / max3.
constexpr uint32_t kBvhDone = 0xfffffffeu;

struct TraceCounters {
    uint32_t nodes, tris, overflow;
};

// 1/d for the slab test, |d| floored at 1e-20 so that 0 * inf never appears.
AKR_D float safe_inv(float d) {
    float a = abs_f(d) < 1e-20f ? __builtin_copysignf(1e-20f, d) : d;
    return __builtin_amdgcn_rcpf(a);
}
AKR_D uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 0xffu; }

struct Trav {  // one ray in flight
    vec3 o, d, inv, noi;   // t = plane * inv + noi
    float tmin, tmax, best_t, best_u, best_v;
    uint32_t ex0, ex1, best;
    uint32_t G, T, tbase, sp, octinv4;
    bool active;
};
AKR_D void trav_begin(Trav& s, vec3 o, vec3 d, float tmin, float tmax, uint32_t ex0, uint32_t ex1) {
    s.o = o; s.d = d;
    s.inv = mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    s.noi = mk3(-o.x * s.inv.x, -o.y * s.inv.y, -o.z * s.inv.z);
    s.tmin = tmin; s.tmax = tmax;
    s.best_t = tmax; s.best_u = 0.0f; s.best_v = 0.0f; s.best = kInvalid;
    s.ex0 = ex0; s.ex1 = ex1;
    // octinv: bit a set = the ray travels towards +a, i.e. meets the children on the low side of axis a first
    const uint32_t oi = (s.inv.x >= 0.0f ? 1u : 0u) | (s.inv.y >= 0.0f ? 2u : 0u) | (s.inv.z >= 0.0f ? 4u : 0u);
    s.octinv4 = oi * 0x01010101u;
    s.G = 1u << (24u + oi);  // the group {root}: base 0, slot 0 at bit 24 + (0 ^ oi)
    s.T = 0; s.tbase = 0; s.sp = 0;
    s.active = tmax >= tmin;
}

// ---- pieces of a step that exist once: trav_step_staged and trav_step below and dinst_trav.h trav_step_inst (a TravI is a Trav) ----
// Take the nearest pending sibling of the lane's node group; the others wait on the stack as one entry. Returns the child's index
// (relative to the tree's first node).
AKR_D uint32_t node_pop(Trav& s, uint32_t* __restrict__ stack, uint32_t depth, TraceCounters& cnt) {
    const uint32_t j = 31u - (uint32_t)__builtin_clz(s.G);  // nearest pending sibling
    s.G &= ~(1u << j);
    if ((s.G >> 24) != 0) {  // the others wait as one entry
        if (s.sp < depth) {
            stack[s.sp * 256u] = s.G;
            s.sp++;
        } else {
            cnt.overflow = 1;  // unreachable for a tree scene_build.cpp accepted; kept as a tripwire (akr_pt_stats)
        }
    }
    const uint32_t slot = (j - 24u) ^ (s.octinv4 & 7u);
    return (s.G & 0xffffffu) + slot;
}
// A candidate that passed every test: an any-hit ray is done, a closest-hit ray keeps the smaller t and, among equal t, the lower id.
AKR_D void hit_commit(Trav& s, bool any_hit, uint32_t gid, float t, float u, float v) {
    if (any_hit) {
        s.best = gid;
        s.T = 0; s.G = 0; s.sp = 0;  // any hit: done
    } else {
        const bool better = (s.best == kInvalid) | (t < s.best_t) | ((t == s.best_t) & (gid < s.best));
        if (better) { s.best_t = t; s.best_u = u; s.best_v = v; s.best = gid; }
    }
}
// A triangle that passed tri_test: the ray's two exclusion slots, the stochastic alpha test, then hit_commit.
template <bool TEX>
AKR_D void hit_accept(const DScene& sc, Trav& s, bool any_hit, uint32_t gid, float t, float u, float v) {
    bool h = (gid != s.ex0) & (gid != s.ex1);
    if (h && sc.has_alpha) h = alpha_test<TEX>(sc, gid, u, v);
    if (h) hit_commit(s, any_hit, gid, t, u, v);
}

// One step of one lane: a triangle test if one is pending, else the next node. MODE 0: closest hit, 1: any hit, 2: `any_rt`
// decides per lane (the wavefront schedule traces both kinds of ray in one loop).
// TILE: the launch keeps the first sc.bvh_tile_nodes nodes (the top levels, breadth-first order: host/bvh.cpp) in LDS at `tile`;
// a lane whose next node is one of them reads it with four ds_read_b128 instead of going through the texture addresser and L1 --
// on the 10 M-triangle hall the traversal keeps that path 58 % busy, and every ray starts with three to five such nodes.
// The same step in two stages: a lane that leaves the node test with leaf triangles tests the first one in the SAME step (two
// dependent fetches per step, a fifth fewer steps per ray). Same visits in the same order. Measured (round 5): BVH kernel of the
// textured room 602 -> 630 Msamples/s, 1 M-triangle hall unchanged, 10 M-triangle hall 317 -> 299: used by the kernels of scenes with
// textures only (trav_step below picks it iff TEX).
template <int MODE, bool TEX, bool TILE = false>
AKR_D void trav_step_staged(const DScene& sc, Trav& s, uint32_t* __restrict__ stack, TraceCounters& cnt, bool any_rt = false, const uint4* tile = nullptr) {
    const bool any_hit = MODE == 2 ? any_rt : (MODE == 1);
    if (s.T == 0) {
        if ((s.G >> 24) == 0) {  // the caller guarantees sp > 0 here
            s.sp--;
            s.G = stack[s.sp * 256u];
        }
        const uint32_t idx = node_pop(s, stack, sc.bvh_stack_depth, cnt);
        const uint4* p = sc.bvh_nodes + (size_t)idx * (kBvhNodeWords / 4);
        uint4 w0, w1, w2, w3;
        if (TILE && idx < sc.bvh_tile_nodes) {
            typedef const volatile uint32_t __attribute__((address_space(3))) * LdsW;
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            typedef const volatile u32x4 __attribute__((address_space(3))) * LdsU4;
            LdsU4 pt = (LdsU4)((LdsW)(const uint32_t*)tile + idx * kBvhNodeWords);
            const u32x4 t0 = pt[0], t1 = pt[1], t2 = pt[2], t3 = pt[3];
            w0 = make_uint4(t0.x, t0.y, t0.z, t0.w); w1 = make_uint4(t1.x, t1.y, t1.z, t1.w); w2 = make_uint4(t2.x, t2.y, t2.z, t2.w);
            w3 = make_uint4(t3.x, t3.y, t3.z, t3.w);
        } else {
            w0 = p[0]; w1 = p[1]; w2 = p[2]; w3 = p[3];
        }
        cnt.nodes++;
        const float limit = s.best_t;
        const float bx = u2f((w0.w & 0xffu) << 23) * s.inv.x, by = u2f(((w0.w >> 8) & 0xffu) << 23) * s.inv.y, bz = u2f(((w0.w >> 16) & 0xffu) << 23) * s.inv.z;
        const float ax = __builtin_fmaf(u2f(w0.x), s.inv.x, s.noi.x), ay = __builtin_fmaf(u2f(w0.y), s.inv.y, s.noi.y), az = __builtin_fmaf(u2f(w0.z), s.inv.z, s.noi.z);
        const bool nx = s.inv.x < 0.0f, ny = s.inv.y < 0.0f, nz = s.inv.z < 0.0f;
        const uint32_t xb = nx ? ((w3.y >> 16) | (w3.y << 16)) : w3.y, yb = ny ? ((w3.z >> 16) | (w3.z << 16)) : w3.z, zb = nz ? ((w3.w >> 16) | (w3.w << 16)) : w3.w;
        const uint32_t qnx[2] = {nx ? w2.z : w1.w, xb}, qfx[2] = {nx ? w1.w : w2.z, xb >> 16};
        const uint32_t qny[2] = {ny ? w2.w : w2.x, yb}, qfy[2] = {ny ? w2.x : w2.w, yb >> 16};
        const uint32_t qnz[2] = {nz ? w3.x : w2.y, zb}, qfz[2] = {nz ? w2.y : w3.x, zb >> 16};
        uint32_t hitmask = 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t meta4 = h ? (w1.x >> 16) : w1.y;
            const uint32_t is_inner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
            const uint32_t inner_mask4 = (is_inner4 >> 4) * 0xffu;
            const uint32_t bit_index4 = (meta4 ^ (s.octinv4 & inner_mask4)) & 0x1f1f1f1fu;
            const uint32_t child_bits4 = (meta4 >> 5) & 0x07070707u;
#pragma unroll
            for (int i = 0; i < (h ? 2 : 4); i++) {
                const float tnx = __builtin_fmaf((float)byte_of(qnx[h], i), bx, ax), tfx = __builtin_fmaf((float)byte_of(qfx[h], i), bx, ax);
                const float tny = __builtin_fmaf((float)byte_of(qny[h], i), by, ay), tfy = __builtin_fmaf((float)byte_of(qfy[h], i), by, ay);
                const float tnz = __builtin_fmaf((float)byte_of(qnz[h], i), bz, az), tfz = __builtin_fmaf((float)byte_of(qfz[h], i), bz, az);
                const float tn = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, s.tmin));
                const float tf = __builtin_fminf(__builtin_fminf(tfx, tfy), __builtin_fminf(tfz, limit));
                if (tn <= tf) hitmask |= byte_of(child_bits4, i) << byte_of(bit_index4, i);
            }
        }
        s.G = ((w0.w >> 24) | ((w1.x & 0xffffu) << 8)) | (hitmask & 0xff000000u);
        s.T = hitmask & 0x00ffffffu;
        s.tbase = w1.z;
    }
    if (s.T != 0) {
        const uint32_t b = (uint32_t)__builtin_ctz(s.T);
        s.T &= s.T - 1u;
        const uint4* p = (const uint4*)sc.woop + (size_t)(s.tbase + b) * (kBvhTriWords / 4);
        const uint4 w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
        cnt.tris++;
        float t, u, v;
        bool h = tri_test(s.o, s.d, make_float4(u2f(w0.x), u2f(w0.y), u2f(w0.z), u2f(w0.w)), make_float4(u2f(w1.x), u2f(w1.y), u2f(w1.z), u2f(w1.w)),
                          make_float4(u2f(w2.x), u2f(w2.y), u2f(w2.z), u2f(w2.w)), s.tmin, s.tmax, t, u, v);
        if (h) hit_accept<TEX>(sc, s, any_hit, w3.x, t, u, v);
    }
    s.active = (s.T != 0) | ((s.G >> 24) != 0) | (s.sp != 0);
}
template <int MODE, bool TEX, bool TILE = false>
AKR_D void trav_step(const DScene& sc, Trav& s, uint32_t* __restrict__ stack, TraceCounters& cnt, bool any_rt = false, const uint4* tile = nullptr) {
    if constexpr (TEX) {
        trav_step_staged<MODE, TEX, TILE>(sc, s, stack, cnt, any_rt, tile);
        return;
    }
    const bool any_hit = MODE == 2 ? any_rt : (MODE == 1);
    const bool do_tri = s.T != 0;
    const uint4* p;
    bool in_tile = false;
    uint32_t tile_idx = 0;
    if (do_tri) {
        const uint32_t b = (uint32_t)__builtin_ctz(s.T);
        s.T &= s.T - 1u;
        p = (const uint4*)sc.woop + (size_t)(s.tbase + b) * (kBvhTriWords / 4);
    } else {
        if ((s.G >> 24) == 0) {  // the caller guarantees sp > 0 here
            s.sp--;
            s.G = stack[s.sp * 256u];
        }
        const uint32_t idx = node_pop(s, stack, sc.bvh_stack_depth, cnt);
        p = sc.bvh_nodes + (size_t)idx * (kBvhNodeWords / 4);
        if (TILE && idx < sc.bvh_tile_nodes) {
            in_tile = true;
            tile_idx = idx;
        }
    }
    // the one fetch of the step: four 16-byte loads, a 64-byte triangle record or a 64-byte node -- one sector either way
    uint4 w0, w1, w2, w3;
    if (TILE && in_tile) {
        // explicitly an LDS address: left generic, the compiler folds the two branches into ONE flat load of a selected pointer
        // (and volatile: two plain loads in the arms of an if / else are sunk into one load of a selected -- generic -- pointer)
        typedef const volatile uint32_t __attribute__((address_space(3))) * LdsW;
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        typedef const volatile u32x4 __attribute__((address_space(3))) * LdsU4;
        LdsU4 pt = (LdsU4)((LdsW)(const uint32_t*)tile + tile_idx * kBvhNodeWords);
        const u32x4 t0 = pt[0], t1 = pt[1], t2 = pt[2], t3 = pt[3];
        w0 = make_uint4(t0.x, t0.y, t0.z, t0.w); w1 = make_uint4(t1.x, t1.y, t1.z, t1.w); w2 = make_uint4(t2.x, t2.y, t2.z, t2.w);
        w3 = make_uint4(t3.x, t3.y, t3.z, t3.w);
    } else {
        w0 = p[0]; w1 = p[1]; w2 = p[2]; w3 = p[3];
    }
    // All four loads are in flight before anything waits. Without this fence the compiler sinks the words only the node test
    // reads into the node branch -- a second dependent round trip to memory for every node step.
    asm volatile("" : "+v"(w0.x), "+v"(w0.y), "+v"(w0.z), "+v"(w0.w), "+v"(w1.x), "+v"(w1.y), "+v"(w1.z), "+v"(w1.w), "+v"(w2.x), "+v"(w2.y),
                      "+v"(w2.z), "+v"(w2.w), "+v"(w3.x), "+v"(w3.y), "+v"(w3.z), "+v"(w3.w));
    if (do_tri) {
        cnt.tris++;
        float t, u, v;
        bool h = tri_test(s.o, s.d, make_float4(u2f(w0.x), u2f(w0.y), u2f(w0.z), u2f(w0.w)), make_float4(u2f(w1.x), u2f(w1.y), u2f(w1.z), u2f(w1.w)),
                          make_float4(u2f(w2.x), u2f(w2.y), u2f(w2.z), u2f(w2.w)), s.tmin, s.tmax, t, u, v);
        if (h) {  // hit_accept, written out: as a call here it costs the non-textured BVH kernels of mcmc / gpt 4 to 12 bytes of scratch
            const uint32_t gid = w3.x;
            h = (gid != s.ex0) & (gid != s.ex1);
            if (h && sc.has_alpha) h = alpha_test<TEX>(sc, gid, u, v);
            if (h) {
                if (any_hit) {
                    s.best = gid;
                    s.T = 0; s.G = 0; s.sp = 0;  // any hit: done
                } else {
                    const bool better = (s.best == kInvalid) | (t < s.best_t) | ((t == s.best_t) & (gid < s.best));
                    if (better) { s.best_t = t; s.best_u = u; s.best_v = v; s.best = gid; }
                }
            }
        }
    } else {
        cnt.nodes++;
        const float limit = s.best_t;  // closest hit: culls with the best distance so far (non-strict: equal-t lower ids stay reachable)
        const float bx = u2f((w0.w & 0xffu) << 23) * s.inv.x, by = u2f(((w0.w >> 8) & 0xffu) << 23) * s.inv.y, bz = u2f(((w0.w >> 16) & 0xffu) << 23) * s.inv.z;
        const float ax = __builtin_fmaf(u2f(w0.x), s.inv.x, s.noi.x), ay = __builtin_fmaf(u2f(w0.y), s.inv.y, s.noi.y), az = __builtin_fmaf(u2f(w0.z), s.inv.z, s.noi.z);
        // Node words (host/bvh.cpp): w0 = origin | exponents + child_base[7:0]; w1 = child_base[23:8] + meta[4..5] | meta[0..3] | tri_base |
        // lo.x of entries 0..3; w2 = lo.y, lo.z, hi.x, hi.y of entries 0..3; w3 = hi.z of entries 0..3 | x, y, z of entries 4, 5 (lo lo hi hi).
        // per axis: the byte planes the ray enters through (near) and leaves through (far)
        const bool nx = s.inv.x < 0.0f, ny = s.inv.y < 0.0f, nz = s.inv.z < 0.0f;
        const uint32_t xb = nx ? ((w3.y >> 16) | (w3.y << 16)) : w3.y, yb = ny ? ((w3.z >> 16) | (w3.z << 16)) : w3.z, zb = nz ? ((w3.w >> 16) | (w3.w << 16)) : w3.w;
        // [0]: entries 0..3 (four bytes), [1]: entries 4, 5 (near in bytes 0, 1; far in bytes 2, 3 after the swap above)
        const uint32_t qnx[2] = {nx ? w2.z : w1.w, xb}, qfx[2] = {nx ? w1.w : w2.z, xb >> 16};
        const uint32_t qny[2] = {ny ? w2.w : w2.x, yb}, qfy[2] = {ny ? w2.x : w2.w, yb >> 16};
        const uint32_t qnz[2] = {nz ? w3.x : w2.y, zb}, qfz[2] = {nz ? w2.y : w3.x, zb >> 16};
        uint32_t hitmask = 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t meta4 = h ? (w1.x >> 16) : w1.y;  // (h = 1: entries 4, 5; the two upper bytes are zero = empty)
            // inner children (index bits 3 and 4 set: 24..31) get their bit position xor-ed with the ray's octant
            const uint32_t is_inner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
            const uint32_t inner_mask4 = (is_inner4 >> 4) * 0xffu;
            const uint32_t bit_index4 = (meta4 ^ (s.octinv4 & inner_mask4)) & 0x1f1f1f1fu;
            const uint32_t child_bits4 = (meta4 >> 5) & 0x07070707u;
#pragma unroll
            for (int i = 0; i < (h ? 2 : 4); i++) {
                const float tnx = __builtin_fmaf((float)byte_of(qnx[h], i), bx, ax), tfx = __builtin_fmaf((float)byte_of(qfx[h], i), bx, ax);
                const float tny = __builtin_fmaf((float)byte_of(qny[h], i), by, ay), tfy = __builtin_fmaf((float)byte_of(qfy[h], i), by, ay);
                const float tnz = __builtin_fmaf((float)byte_of(qnz[h], i), bz, az), tfz = __builtin_fmaf((float)byte_of(qfz[h], i), bz, az);
                const float tn = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, s.tmin));
                const float tf = __builtin_fminf(__builtin_fminf(tfx, tfy), __builtin_fminf(tfz, limit));
                if (tn <= tf) hitmask |= byte_of(child_bits4, i) << byte_of(bit_index4, i);  // empty entries have no child bits
            }
        }
        s.G = ((w0.w >> 24) | ((w1.x & 0xffffu) << 8)) | (hitmask & 0xff000000u);
        s.T = hitmask & 0x00ffffffu;
        s.tbase = w1.z;
    }
    s.active = (s.T != 0) | ((s.G >> 24) != 0) | (s.sp != 0);
}

template <bool ANY_HIT, bool TEX = false>
AKR_D bool trace_bvh(const DScene& sc, vec3 o, vec3 d, float tmin, float tmax, uint32_t ex0, uint32_t ex1, Hit& hit,
                     uint32_t* __restrict__ stack, TraceCounters& cnt) {
    Trav s;
    trav_begin(s, o, d, tmin, tmax, ex0, ex1);
    while (s.active) trav_step<ANY_HIT ? 1 : 0, TEX>(sc, s, stack, cnt);
    hit.t = s.best_t; hit.u = s.best_u; hit.v = s.best_v; hit.gid = s.best;
    return s.best != kInvalid;
}

// ---- a traversal that goes on later: the wavefront schedule's carried rays (wf_kernels.hip) ----
// What is kept of a ray in flight, in the order of kernels.h CY_*: the best hit so far and the place in the tree, a group of four words each. The ray
// itself is begun again from the path state before trav_resume; the stack stays where it is (LDS) or travels with the record (wavefront).
AKR_D uint4 carry_best(const Trav& s) { return make_uint4(f2u(s.best_t), f2u(s.best_u), f2u(s.best_v), s.best); }
AKR_D uint4 carry_place(const Trav& s) { return make_uint4(s.G, s.T, s.tbase, s.sp); }
AKR_D void trav_resume(const DScene& sc, Trav& s, uint4 best, uint4 place) {
    s.best_t = u2f(best.x); s.best_u = u2f(best.y); s.best_v = u2f(best.z); s.best = best.w;
    s.G = place.x; s.T = place.y; s.tbase = place.z; s.sp = place.w;
    s.active = (s.T != 0) | ((s.G >> 24) != 0) | (s.sp != 0);
}

}  // namespace akr
