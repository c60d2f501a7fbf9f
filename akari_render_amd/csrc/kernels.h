// kernels.h -- kernel parameter block and host-callable launchers (implemented in the .hip file of the kernel; the test hooks: probe_kernels.hip).
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#endif

#include "device/drng.h"
#include "device/dscene.h"

// The tables a pt kernel stages in LDS, in the order they lie there: the index of PtParams::stage_bytes, of the sizes the host computes
// (host/scene_build.cpp stage_table_bytes, host/pt_plan.cpp) and of the copy loop (device/dpath.h stage_scene_tables). Outside the namespace
// like PtVariant below, and for its reason.
enum StageTable : int {
    ST_SHADE, ST_NORMALS,  // per triangle: the exhaustive kernels only
    ST_INST, ST_MATERIALS, ST_LIGHT_ALIAS, ST_AREA_ALIAS, ST_LIGHTS, ST_LIGHT_PDF, ST_AREA_PDF,
    ST_TEX_NODES, ST_TEX_IMAGES, ST_MAT_INPUTS,  // the TEX kernels only
    ST_GGX,  // the GGX albedo table: the full-graph exhaustive kernels of textured scenes, where the LDS budget allows
    ST_COUNT
};

#if !defined(__HIPCC_RTC__)
#include <algorithm>
// Which instantiation of pt_pass_body (device/pt_pass.h) a pt session runs, decided once per session (host/api_pt.cpp pt_plan) and
// carried by the session; the launchers, the per-scene kernel's wrapper text and akr_pt_kernel_info all read it. Host side only, and
// outside the namespace: the relaxed tier's translation unit compiles this header inside another one (pt_kernels_relaxed.hip).
// Every member is filled by name (pt_scene_facts, pt_variant_from_bits, pt_flat_variant): the order of the members means nothing.
struct PtVariant {
    bool bvh = false, fd = false, tex = false, pmj = false, stage = false, defer = false, simple = false, inst = false, env = false, lens = false;
    bool feat = false;   // the session collects the denoiser's guides (device/dpath.h FEAT)
    bool punct = false;  // the scene has punctual lights (device/dpunct.h PUNCT)
    bool ltree = false;  // ... and a light tree over the point and spot ones (device/dlighttree.h LTREE): the PUNCT kernels that walk it
};
// The combinations that exist as precompiled kernels -- the one statement of the exclusion rules: the exhaustive kernels always stage;
// DEFER only in full-graph kernels, of BVH scenes those with textures; SIMPLE only in full-graph kernels of scenes without textures;
// neither with an environment light, a lens, collected guides or punctual lights; a kept scene runs the BVH kernel without staged tables, DEFER or
// SIMPLE, collects no guides and has no punctual lights; nor does a session that collects guides.
constexpr bool pt_variant_compiled(const PtVariant& v) {
    return (v.bvh || v.stage) && !(v.defer && (v.fd || (v.bvh && !v.tex))) && !(v.simple && (v.fd || v.tex)) && !((v.env || v.lens || v.feat || v.punct) && (v.defer || v.simple)) &&
           !(v.inst && !(v.bvh && !v.stage && !v.defer && !v.simple && !v.feat)) && !(v.punct && (v.feat || v.inst)) && !(v.ltree && !v.punct);
}
// The flags of a per-scene kernel request as one integer: akr_host_spec_compile(_text), the helper process's command line (fd = false,
// tex = true, no SIMPLE: a per-scene kernel is the full-graph kernel of a scene with textures).
constexpr uint32_t pt_variant_bits(const PtVariant& v) {
    return (v.bvh ? 1u : 0u) | (v.pmj ? 2u : 0u) | (v.stage ? 4u : 0u) | (v.defer ? 8u : 0u) | (v.inst ? 16u : 0u) | (v.env ? 32u : 0u) | (v.lens ? 64u : 0u) |
           (v.feat ? 128u : 0u) | (v.punct ? 256u : 0u) | (v.ltree ? 512u : 0u);  // (neither is ever set in a per-scene kernel's request: FEAT sessions and scenes with punctual lights run the interpreter kernels)
}
constexpr PtVariant pt_variant_from_bits(uint32_t f) {
    PtVariant v;
    v.tex = true;
    v.bvh = (f & 1u) != 0;
    v.pmj = (f & 2u) != 0;
    v.stage = (f & 4u) != 0;
    v.defer = (f & 8u) != 0;
    v.inst = (f & 16u) != 0;
    v.env = (f & 32u) != 0;
    v.lens = (f & 64u) != 0;
    v.feat = (f & 128u) != 0;
    v.punct = (f & 256u) != 0;
    v.ltree = (f & 512u) != 0;
    return v;
}
// The translation units that hold the precompiled pt kernels. A unit fixes (kind, ENV, LENS): pt_unit_kernels.hip is compiled once per
// unit (build.py PT_KINDS: the same kinds in the same order -- the two lists go together), and launch_pt_pass (pt_kernels.hip) goes
// through one table of kPtUnits entries to the unit of a session's variant. The ONE statement of which unit holds which variant.
enum PtKind : uint32_t {
    PT_KIND_PLAIN,       // flattened scenes: k_pt_pass
    PT_KIND_INST,        // scenes kept as meshes + instances: k_pt_pass_inst (pt_inst_kernel.h)
    PT_KIND_FEAT,        // sessions that collect the denoiser's guides: k_pt_pass<.., FEAT>
    PT_KIND_PUNCT,       // scenes with punctual lights: k_pt_pass<.., PUNCT>
    PT_KIND_PUNCT_TREE,  // ... and a light tree over them: k_pt_pass<.., PUNCT, LTREE>
    PT_KIND_COUNT
};
constexpr uint32_t kPtUnits = PT_KIND_COUNT * 4u;
constexpr uint32_t pt_unit_index(const PtVariant& v) {
    const uint32_t kind = v.inst ? PT_KIND_INST : v.feat ? PT_KIND_FEAT : v.punct ? (v.ltree ? PT_KIND_PUNCT_TREE : PT_KIND_PUNCT) : PT_KIND_PLAIN;
    return kind * 4u + (v.env ? 2u : 0u) + (v.lens ? 1u : 0u);
}
// ... and back: the flags a unit fixes (the others false)
constexpr PtVariant pt_unit_flags(uint32_t unit) {
    const uint32_t kind = unit / 4u;
    PtVariant v;
    v.inst = kind == PT_KIND_INST;
    v.feat = kind == PT_KIND_FEAT;
    v.punct = kind == PT_KIND_PUNCT || kind == PT_KIND_PUNCT_TREE;
    v.ltree = kind == PT_KIND_PUNCT_TREE;
    v.env = (unit & 2u) != 0;
    v.lens = (unit & 1u) != 0;
    return v;
}
// Every variant that exists as a kernel is routed to the unit that was compiled for it, and the two functions are each other's inverse.
constexpr bool pt_units_hold_every_variant() {
    for (uint32_t unit = 0; unit < kPtUnits; unit++)
        if (pt_unit_index(pt_unit_flags(unit)) != unit) return false;
    for (uint32_t f = 0; f < (1u << 13); f++) {
        PtVariant v;
        v.bvh = f & 1u, v.fd = f & 2u, v.tex = f & 4u, v.pmj = f & 8u, v.stage = f & 16u, v.defer = f & 32u, v.simple = f & 64u;
        v.inst = f & 128u, v.env = f & 256u, v.lens = f & 512u, v.feat = f & 1024u, v.punct = f & 2048u, v.ltree = f & 4096u;
        if (!pt_variant_compiled(v)) continue;
        const uint32_t unit = pt_unit_index(v);
        const PtVariant u = pt_unit_flags(unit);
        if (unit >= kPtUnits || u.inst != v.inst || u.env != v.env || u.lens != v.lens || u.feat != v.feat || u.punct != v.punct || u.ltree != v.ltree) return false;
    }
    return true;
}
static_assert(pt_units_hold_every_variant(), "a compiled variant is routed to a unit that fixes other flags");
// pt_lds_layout (below): what it is given ...
struct PtLdsSizes {
    uint32_t stack_depth, n_tris, n_nodes;  // DScene.bvh_stack_depth, n_tris, n_nodes
    uint32_t tex_slots;                     // graph value slots per lane (0: a per-scene kernel keeps them in registers)
    uint32_t stage_bytes;                   // PtParams.stage_total
    bool bluenoise;                         // the pmj02bn sampler's blue-noise table is there to be staged
};
// ... and what it answers: word offsets of the blocks, the node count of the tile, bytes
struct PtLdsLayout {
    uint32_t stage_offset, recs_offset, tile_offset, tile_nodes, park_offset, carry_offset, bn_offset, val_offset_words;
    size_t required_bytes, total_bytes;  // without / with the blocks that only take what room is left (node tile, blue-noise columns)
};
#endif

namespace akr {

// ---- build switches of k_pt_pass (device/pt_pass.h); each default is the winner of a same-box A/B run ----
#ifndef AKR_PT_STRAGGLERS
#define AKR_PT_STRAGGLERS 8  // BVH kernels: n > 0 = an intersection phase ends when at most 1/n of the lanes that entered it are still
                             // tracing; those lanes keep their traversal and go on in the next phase (device/pt_pass.h)
#endif
#ifndef AKR_PT_STRAGGLERS_TEX
#define AKR_PT_STRAGGLERS_TEX 0  // the same for the BVH kernels of scenes with textures (measured separately)
#endif
#ifndef AKR_PT_STRAGGLERS_INST
#define AKR_PT_STRAGGLERS_INST 8  // the same for the kernels of scenes kept as meshes + instances (dinst_trav.h trace_pair_inst)
#endif
// LDS columns per lane (one word per slot, slot s of lane i at word s * 256 + i): cold path state parked while a vertex is shaded
// (dpath.h: PARK), and a traversal carried over to the next intersection phase (device/pt_pass.h).
constexpr uint32_t kParkSlots = 16, kParkSlotsNoDefer = 13;  // dpath.h: PK_*
constexpr uint32_t kParkSlotsFeat = 19;                      // FEAT kernels (never DEFER): the 13 and the two guide accumulators (PK_FEAT_*)
// The columns of a carried traversal (device/pt_pass.h, dinst_trav.h trace_pair_inst): best hit so far | place in the tree | which of the vertex's
// two rays | the first ray's hit | kept scenes (dinst_trav.h): TLAS leaf of the instance the ray is in, the candidate waiting for its exact test.
// A carried ray of the wavefront schedule (wf_kernels.hip, WfBuffers::carry) keeps the same groups of four (carry_best, carry_place, carry_inst).
enum : uint32_t { CY_BEST_T = 0, CY_BEST_U, CY_BEST_V, CY_BEST, CY_G, CY_T, CY_TBASE, CY_SP, CY_PHASE, CY_HIT_T, CY_HIT_U, CY_HIT_V, CY_HIT_GID, CY_END,
                  CY_LEAF = CY_END, CY_PEND_REC, CY_PEND_INST, CY_END_INST };
constexpr uint32_t kCarrySlots = CY_END, kCarrySlotsInstanced = CY_END_INST;  // 13, 16
constexpr size_t kBlueNoiseColumnBytes = 48 * 256 * 2;          // dpath.h pmj_bluenoise_stage: one u16 per array and lane
#if !defined(__HIPCC_RTC__)
// Dynamic LDS of a pt launch (k_pt_pass, k_pt_pass_inst, a per-scene kernel) and where its blocks start, in this order:
// [traversal stacks][staged tables][triangle records (exhaustive kernels: disect.h trace_pair_exhaustive)][node tile (BVH kernels of scenes
// without textures: disect.h TILE)][park columns (full-graph kernels of scenes with textures: dpath.h PARK)][carry columns (BVH kernels that
// let a wave's longest rays run on: device/pt_pass.h)][blue-noise columns (pmj02bn, exhaustive kernels)][graph values]. The tile and the
// blue-noise columns take what room is left; `required_bytes` is the rest. The ONE place that lays a launch out: launch_pt_pass places
// the blocks with it, and session_params (host/api_pt.cpp) decides the staging by asking it whether the launch fits.
// a workgroup's share of the CU's 160 KB: a quarter (four waves per SIMD), a third for the kernels of textured scenes (three)
inline size_t pt_lds_budget(bool tex) { return (tex ? 53 : 40) * 1024; }
// plan_larger_park: size the park block for a DEFER kernel whatever the variant says. The staging decision has always planned that way; a
// textured full-graph launch without deferral whose required bytes come within 3 * 1024 of the budget is therefore refused staging
// that would fit. (Kept as it is: granting it changes which kernel such a scene runs.)
inline PtLdsLayout pt_lds_layout(const PtVariant& v, const PtLdsSizes& s, bool plan_larger_park = false) {
    PtLdsLayout L{};
    const size_t slots = v.tex ? (size_t)s.tex_slots * kTexValStride * sizeof(TexVal) : 0;
    const int stragglers = v.inst ? AKR_PT_STRAGGLERS_INST : (v.tex ? AKR_PT_STRAGGLERS_TEX : AKR_PT_STRAGGLERS);
    const size_t park = (!v.fd && v.tex) ? (size_t)(v.feat ? kParkSlotsFeat : (v.defer || plan_larger_park ? kParkSlots : kParkSlotsNoDefer)) * 256 * 4 : 0;
    const size_t carry = (v.bvh && stragglers > 0) ? (size_t)(v.inst ? kCarrySlotsInstanced : kCarrySlots) * 256 * 4 : 0;
    auto align = [](size_t b) { return (b + 15) & ~(size_t)15; };
    size_t base = v.bvh ? (size_t)s.stack_depth * 256 * 4 : 0;
    L.stage_offset = (uint32_t)(base / 4);
    base += s.stage_bytes;
    L.recs_offset = (uint32_t)(base / 4);
    base = align(base + (!v.bvh ? (size_t)(s.n_tris + 2) * 48 : 0));
    L.required_bytes = align(base + park + carry) + slots;
    L.tile_offset = (uint32_t)(base / 4);
    if (v.bvh && !v.tex && !v.inst) {  // what is left of the workgroup's share after the launch's other blocks
        const size_t other = base + park + carry + slots, budget = pt_lds_budget(v.tex) - 256;
        if (other < budget) L.tile_nodes = (uint32_t)std::min<size_t>({(budget - other) / (kBvhNodeWords * 4), (size_t)s.n_nodes, (size_t)1024});
        base = align(base + (size_t)L.tile_nodes * kBvhNodeWords * 4);
    }
    L.park_offset = (uint32_t)(base / 4);
    base += park;
    L.carry_offset = (uint32_t)(base / 4);
    base += carry;
    // pmj02bn: the lanes' blue-noise columns, if the workgroup's share has room for them (exhaustive kernels of small scenes: 24 KB next to
    // ~13 KB of staged tables; the BVH kernels' traversal stacks leave none)
    if (s.bluenoise && !v.bvh && base + slots + kBlueNoiseColumnBytes <= pt_lds_budget(v.tex)) {
        L.bn_offset = (uint32_t)(align(base) / 4);
        base = align(base) + kBlueNoiseColumnBytes;
    }
    L.val_offset_words = (uint32_t)((base = align(base)) / 4);
    L.total_bytes = base + slots;
    return L;
}
#endif

// Launch counters (akr_pt_stats) are kStatStripes copies of 8 u64, a workgroup adding to copy blockIdx % kStatStripes: the wavefront
// schedule flushes them once per wave and ITERATION (32 k waves x 7 atomics on seven addresses per k_wf_shade launch serialise at the
// L2 -- measured: a large part of that kernel's time); the host sums the copies when it reads them.
constexpr uint32_t kStatStripes = 256;
// Everything one pass of the path tracer needs; passed by value as the kernel argument (lands in SGPRs).
struct PtParams {
    DScene sc;
    // PerspectiveCameraData (camera/mod.rs:105-118): raster->camera and camera->world, column-major
    float r2c[16];
    float c2w[16];
    uint32_t c2w_identity;
    uint32_t width, height;
    // pt::Config (pt.rs:916-929)
    uint32_t max_depth, rr_depth, use_nee, indirect_only, force_diffuse;
    int32_t debug_depth;
    int32_t pixel_offset[2];
    uint32_t filter_type;
    float filter_radius;
    uint32_t color;          // ColorPipeline bits (device/dbsdf.h COLOR_*): the space the path shades in
    uint32_t pass_spp;       // samples per pixel per pass (spp_per_pass)
    uint32_t n_passes;       // passes fused into this launch (>= 1)
    uint32_t last_pass_spp;  // samples of the launch's last pass (<= pass_spp)
    PcgStartConsts start;
    // per-pixel sampler states (Pcg32[N]), film accumulator (f32[7N], reference layout), counters (u64[8])
    Pcg32* states;
    float* film;
    uint64_t* counters;
    // sampler (sampler/mod.rs:282-295): 0 = independent (PCG32 state per pixel), 1 = pmj02bn (index-based: point sets +
    // blue-noise offsets; states[pix].state holds the pixel's sample index, .inc its coordinates)
    uint32_t sampler;
    uint32_t smp_seed, smp_spp, smp_w;      // Pmj02BnState.{seed, spp, w}
    uint64_t smp_mod_magic;                 // fastmod_magic(smp_spp): x % spp without a division (drng.h)
    const uint32_t* pmj_sets;               // [5][65536][2] u32 fixed point
    const uint16_t* bluenoise;              // [48][128][128] unorm16
    // The tables the shading phase gathers from, staged in LDS by k_pt_pass: bytes per table, by StageTable (above); 0 total = not staged.
    uint32_t stage_bytes[ST_COUNT];
    uint32_t stage_total;
    uint32_t simple_scene;   // no coat, no transmission, no normal map, no glass material, no textures: the full-graph kernels without that code
    uint32_t defer_metal;    // iterations with (iteration & defer_metal) != 0 put hits on "expensive" materials off by one iteration (device/pt_pass.h: DEFER)
    uint32_t defer_flags;    // ... expensive = (DMaterial.flags & defer_flags) != 0: MF_EVAL_METAL (the conductor lobe), MF_TEXTURED (a graph to evaluate)
    uint32_t tex_slots;      // TEX scenes: value slots per lane of the graph evaluation (LDS, after the launch's other blocks)
    uint32_t tile_offset;    // BVH kernels with a node tile (disect.h: TILE): word offset of the tile; its size is sc.bvh_tile_nodes
    uint32_t park_offset;    // kernels that park cold path state in LDS while shading (dpath.h: PARK): word offset of the columns
    uint32_t carry_offset;   // BVH kernels that let a wave's longest rays run on into the next iteration (device/pt_pass.h): their columns
    uint32_t bn_offset;      // pmj02bn sampler, k_pt_pass: word offset of the lanes' blue-noise columns (48 x 256 x 2 B, dpath.h), 0 = the table in HBM
    // wavefront schedule, option wf_sort: the ray queues are sorted by (Morton code of the origin in the scene's box, octant of the direction)
    uint32_t wf_sort;
    float sort_lo[3], sort_scale[3];  // cell = (o - lo) * scale, 128 cells per axis
    // work distribution
    uint32_t n_items;
    uint32_t shard_rank, shard_count;
    uint32_t tile_w, tile_h, tiles_x, tiles_y;
    const uint32_t* owned_tiles;  // shard_count > 1: the tiles (row-major ids) this rank owns, in Morton order (tile_owner below); else null
    // cost order (host/api_pt.cpp pt_plan decides): a pt session's first launch stores every lane's closest-hit rays in item_cost[item]
    // (pt_pass.h, after the loop; room for n_items rounded up to 256); later launches take item -> pixel from item_pixels, the session's
    // pixels sorted by that cost, dearest first (kInvalid = no pixel: padding up to a multiple of 256). Either may be null: nothing
    // recorded / items dealt by position (dpath.h item_to_pixel).
    uint32_t* item_cost;
    const uint32_t* item_pixels;
    // thin lens (dpath.h generate_ray_lens_from): radius > 0 = the session runs the LENS kernels, which alone read these
    float lens_radius, lens_focal;
    // FEAT kernels alone read these: the accumulators (7 N floats, the film's layout) of the albedo and the shading-normal guide
    float *feat_albedo, *feat_normal;
    // the camera's projection (dpath.h generate_ray_lens_from): PROJ_*; anything but PROJ_PERSPECTIVE = the session runs the LENS
    // kernels, which alone read these. Orthographic needs its r2c only; the panorama's window folded by the host (camera_params).
    uint32_t projection;
    float pano_lon0, pano_dlon, pano_lat1, pano_dlat, pano_inv_w, pano_inv_h;
};
enum : uint32_t { PROJ_PERSPECTIVE = 0, PROJ_ORTHOGRAPHIC = 1, PROJ_PANORAMA = 2 };  // akr_projection_type
// "this camera needs the LENS kernels": the one statement of it, for the router (pt_plan.cpp), the launchers with a [lens] table and the test hooks
AKR_HD bool camera_runs_lens_kernels(float lens_radius, uint32_t projection) { return lens_radius > 0.0f || projection != PROJ_PERSPECTIVE; }

// Which rank owns tile (tx, ty) of a frame shared by `count` ranks: its position on the Z-order (Morton) curve, modulo the ranks
// ("tile t owned by GPU t mod G in Morton order"): 8 ranks each get one tile of every aligned 4 x 2 block of tiles, so every
// rank sees the same mix of cheap and expensive regions whatever the row length is. One definition for the kernels (dpath.h
// item_to_pixel through the session's owned_tiles list, gpt_kernels.hip), the host (api_pt.cpp, api_aux.cpp), and -- restated -- the
// oracle (akr_oracle.c or_pixel_owned) and the Python mirror (distributed.owned_pixel_mask).
AKR_HD uint32_t morton_spread16(uint32_t x) {
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
AKR_HD uint32_t tile_morton(uint32_t tx, uint32_t ty) { return morton_spread16(tx) | (morton_spread16(ty) << 1); }
AKR_HD uint32_t tile_owner(uint32_t tx, uint32_t ty, uint32_t count) { return tile_morton(tx, ty) % count; }

// Path state of the wavefront schedule (wf_kernels.hip): structure-of-arrays, one slot per pixel of the launch.
struct WfBuffers {
    float4 *ray_o, *ray_d;          // next closest-hit ray: o | exclude id ; d
    float4 *sh_o, *sh_d, *sh_c;     // pending shadow ray: o | exclude0 ; d | tmax ; contribution | exclude1
    float4* hit;                    // written by k_wf_trace: gid, u, v | occluded
    float4 *beta, *rad, *base;      // beta | prev_bsdf_pdf ; radiance | depth ; base | flags
    float4* film;                   // film accumulator of the slot's pixel: rgb | weight
    uint4 *rng, *misc;              // pcg state, dim, samples_done ; pass_idx, cur_spp, pcg inc
    uint32_t* queue_closest[2];     // ray queues (slot ids), double-buffered
    uint32_t* queue_shadow[2];
    uint32_t* key_closest[2];       // option wf_sort: sort key of every queue entry (wf_kernels.hip wf_ray_key), same indexing as the queues
    uint32_t* key_shadow[2];
    uint32_t* qcount;               // [4]: closest/shadow counts of queue 0, of queue 1
    uint32_t* qhead;                // next unclaimed ray id of the queue being traced
    uint32_t* n_active;             // slots still active after the last shade
    // Rays a trace launch did not finish (wf_kernels.hip: "carried rays"): a wave that finds the queue empty and has few lanes left saves those
    // lanes' traversals and ends; the ray goes on in the next trace launch, its slot is not shaded meanwhile. nullptr = every launch traces to the end.
    uint32_t* pend;                 // per slot: bit 0 = its closest-hit ray is carried, bit 1 = its shadow ray
    uint32_t* carry;                // per (kind, slot) carry_words words: best t, u, v, id | G, T, tbase, sp | leaf, pend_rec, pend_inst, - | the stack
    uint32_t carry_words, n_slots;  // (record of kind k, slot s at carry + (k * n_slots + s) * carry_words)
    uint32_t carry_queue;           // launches of fewer rays than this trace to the end
    uint32_t carry_lanes, carry_steps;  // a wave hands over when at most carry_lanes lanes are left and each has had carry_steps steps (16, 48; tests: 56, 4)
    // The slots [slot_base, slot_end) this set of queues and counters serves: a session's slots are divided into GROUPS, each with its own
    // queues, counters and stream, so that one group's kernels fill the chip while another's trace launch waits for its last rays
    // (host/api_pt.cpp wf_run). The state arrays above are the session's, indexed by slot.
    uint32_t slot_base, slot_end;
};

// Scratch and accumulators of the gpt integrator (gpt_kernels.hip), all f32 RGB: per-pixel splat slots of one sample (own,
// shifted[i]); with a reconstruction, the sums / sums of squares of the primal image and the (W+1) x (H+1) gradient images.
struct GptParams {
    float* own;
    float* shifted[4];
    float *acc_p, *acc_gx, *acc_gy, *sqr_p, *sqr_gx, *sqr_gy;
    uint32_t reconnect, stride, separate_weights, reconstruction;
    // Sharded render (akr_gpt_begin with an akr_shard): k_gpt_sample runs the pixels of `item_pixels` -- the rank's own tiles plus
    // the halo whose offset paths land in them -- and k_gpt_update folds only the pixels of the rank's own tiles.
    const uint32_t* item_pixels;  // pixel index per work item, or nullptr = PtParams' tile enumeration
    uint32_t shard_rank, shard_count, tile_w, tile_h, tiles_x;
};

// mcmc_opt integrator (mcmc_kernels.hip)
struct PssSample {  // mcmc_opt.rs:21-26
    float cur, backup;
    uint32_t last_modified, modified_backup;
};
struct MarkovState {  // mcmc_opt.rs:41-51
    uint32_t cur_pixel[2], chain_id;
    float cur_f, b;
    uint32_t b_cnt, n_accepted, n_mutations, cur_iter, last_large_iter;
};
struct McmcParams {
    PssSample* pss;          // [dim][n_chains]
    MarkovState* states;     // [n_chains]
    float4* cur_colors;      // [n_chains]
    Pcg32* rngs;             // [n_chains] the chains' independent samplers
    const Pcg32* seeds;      // [max(n_bootstrap, n_chains)] init_pcg32_buffer_with_seed(seed)
    float* fs;               // [n_bootstrap] bootstrap contributions
    const uint32_t* resampled;  // [n_chains] bootstrap path each chain starts from
    float* film;             // the film (7 N floats); the chains splat into its splat channels
    uint32_t n_chains, n_bootstrap, dim, width, height;
    uint32_t chain_begin, chain_count;  // the chains this launch runs: [chain_begin, chain_begin + chain_count) of the n_chains (a rank's share, akr_mcmc_render_shard)
    uint32_t exponential_mutation;
    float small_sigma, large_step_prob, image_mutation_prob, image_mutation_size;
};
#if !defined(__HIPCC_RTC__)  // host-callable launchers: not part of a per-scene kernel module
hipError_t launch_mcmc_bootstrap(const PtParams& p, const McmcParams& m, hipStream_t stream);
hipError_t launch_mcmc_init(const PtParams& p, const McmcParams& m, hipStream_t stream);
hipError_t launch_mcmc_advance(const PtParams& p, const McmcParams& m, uint32_t mutations_per_chain, float contribution, hipStream_t stream);
#endif

#if !defined(__HIPCC_RTC__)
// pt_lds_layout's input as a session's parameter block holds it, and the block with a layout's offsets filled in
inline PtLdsSizes pt_lds_sizes(const PtParams& p) {
    return PtLdsSizes{p.sc.bvh_stack_depth, p.sc.n_tris, p.sc.n_nodes, p.tex_slots, p.stage_total, p.sampler == 1u && p.bluenoise != nullptr};
}
inline PtParams pt_params_with_layout(const PtParams& p, const PtLdsLayout& L) {
    PtParams q = p;
    q.tile_offset = L.tile_offset; q.sc.bvh_tile_nodes = L.tile_nodes; q.park_offset = L.park_offset; q.carry_offset = L.carry_offset;
    q.bn_offset = L.bn_offset; q.sc.tex.val_offset_words = L.val_offset_words;
    return q;
}
#endif
// The simple layouts (aov, gpt, mcmc, wavefront, probes): dynamic LDS of a launch that evaluates shader graphs = its own blocks (`base_bytes`: traversal stacks, staged tables), then
// tex_slots x 256 lanes x 16 B of value slots. Returns the parameter block with the slots' offset filled in and the total size.
inline PtParams with_tex_slots(const PtParams& p, size_t base_bytes, size_t& lds_bytes) {
    PtParams q = p;
    base_bytes = (base_bytes + 15) & ~(size_t)15;
    q.sc.tex.val_offset_words = (uint32_t)(base_bytes / 4);
    lds_bytes = base_bytes + (p.sc.tex.nodes != nullptr ? (size_t)p.tex_slots * kTexValStride * sizeof(TexVal) : 0);
    return q;
}
#if !defined(__HIPCC_RTC__)
hipError_t launch_inst_share_bits(const DScene& sc, uint32_t* bits, uint32_t* mesh_tri_words, hipStream_t stream);  // pt_kernels.hip: once per kept scene (DInst::share_bits)
hipError_t launch_probe_env(const PtParams& p, uint32_t mode, uint32_t n, const float* in, float* out, hipStream_t stream);  // test hook
hipError_t launch_probe_light_sample(const PtParams& p, uint32_t n, const float* rows9, float* out13, uint32_t* light, hipStream_t stream);  // test hook
hipError_t launch_probe_light_tree_sample(const PtParams& p, uint32_t n, const float* rows9, float* out13, uint32_t* light, uint32_t* record, hipStream_t stream);  // ... the same over a light tree
// test hook: the camera ray (o.xyz, d.xyz) of n items, each a pixel (x, y) and the four numbers u_filter.xy, u_lens.xy
hipError_t launch_probe_camera_rays(const PtParams& p, uint32_t n, const uint32_t* pixels2, const float* u4, float* out6, hipStream_t stream);
// One pass launch of a pt session: lays the LDS out (pt_lds_layout) and goes to the translation unit that holds the variant's kernel
// (pt_unit_index; pt_kernels.hip: the table). spec_fn: the per-scene kernel of the session (host/specialise.cpp) instead of the precompiled one, or nullptr;
// relaxed: the kernels of the relaxed arithmetic tier (pt_kernels_relaxed.hip), which exist for variants without inst, env and lens
hipError_t launch_pt_pass(const PtParams& p, const PtVariant& v, hipStream_t stream, hipFunction_t spec_fn = nullptr, bool relaxed = false);
hipError_t launch_gpt_sample(const PtParams& p, const GptParams& g, hipStream_t stream);
hipError_t launch_gpt_update(const GptParams& g, uint32_t W, uint32_t H, float* film, hipStream_t stream);
hipError_t launch_gpt_recon_init(const GptParams& g, uint32_t W, uint32_t H, float* old, float spp, hipStream_t stream);
hipError_t launch_gpt_recon(const GptParams& g, uint32_t W, uint32_t H, const float* old, float* cur, float scaling, float spp, hipStream_t stream);
hipError_t launch_aov(const PtParams& p, uint32_t spp, uint32_t aov, uint32_t remap, hipStream_t stream);
hipError_t launch_wf_init(const PtParams& p, const WfBuffers& wf, hipStream_t stream);
hipError_t launch_wf_shade(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream);
uint32_t wf_trace_blocks_per_cu(const PtParams& p);
hipError_t launch_wf_trace(const PtParams& p, const WfBuffers& wf, uint32_t q_in, uint32_t n_blocks, hipStream_t stream);
// wf_sort.hip: key-value radix sort of a ray queue (24-bit keys)
size_t wf_sort_temp_bytes(uint32_t n);
hipError_t wf_sort_pairs(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n, hipStream_t stream);
// cost_order_kernels.hip: PtParams.item_pixels from PtParams.item_cost -- the items of p (dealt by position, p.item_pixels ignored) sorted by descending cost,
// ties by ascending pixel, kInvalid behind them. n_padded = p.n_items rounded up to 256 = entries of `table` and of each of the two key buffers.
size_t cost_order_temp_bytes(uint32_t n_padded);
hipError_t launch_cost_order(const PtParams& p, uint32_t n_padded, uint64_t* keys, uint64_t* keys_sorted, void* temp, size_t temp_bytes, uint32_t* table, hipStream_t stream);
hipError_t launch_cost_to_pixels(const PtParams& p, const uint32_t* item_cost, uint32_t* pixel_cost, hipStream_t stream);  // test hook: item costs as a map over the pixels
hipError_t launch_probe_material(const PtParams& p, uint32_t material, uint32_t n, const float* uv, uint32_t* out, hipStream_t stream);
hipError_t launch_init_pcg32(const uint64_t* seeds, void* states, uint64_t n, hipStream_t stream);
hipError_t launch_film_resolve(const float* film, uint64_t n, float splat_scale, float* rgb, hipStream_t stream);
hipError_t launch_ggx_table(const uint64_t* seeds, float* table, uint32_t samples, hipStream_t stream);
hipError_t launch_probe_math(uint32_t n, const float* x, float* s, float* c, float* l, hipStream_t stream);
hipError_t launch_probe_math2(uint32_t n, const float* xy, float* out, hipStream_t stream);
hipError_t launch_probe_bsdf(const DMaterial* m, const float* table, int mode, const float* wo, uint32_t n, const float* in, float* out,
                             hipStream_t stream);
hipError_t launch_probe_div(uint32_t n, const float* a, const float* b, float* out_fast, float* out_ieee, hipStream_t stream);
hipError_t launch_probe_pcg_end_pass(uint32_t n, const uint64_t* state, const uint64_t* inc, const uint32_t* dim, uint64_t* out_closed, uint64_t* out_loop, hipStream_t stream);
hipError_t launch_probe_intersect_pair(const PtParams& p, uint32_t n, const float* rays, const uint32_t* excl, uint32_t* out, float* out_tuv, hipStream_t stream);
hipError_t launch_probe_intersect(const PtParams& p, uint32_t n, const float* rays, uint32_t* out, float* bary, hipStream_t stream);
hipError_t launch_probe_si(const PtParams& p, uint32_t n, const uint32_t* inst_prim, const float* bary, float* out, hipStream_t stream);
#endif

}  // namespace akr
