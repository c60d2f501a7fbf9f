// scene_punct.cpp -- the punctual lights on the host (DESIGN.md sections 4.14 and 4.15): the description checked, the 64-byte record the kernels read
// (device/dscene.h DPunct; folded in double, each value rounded once) and the lights' entries in the light table, between the emissive instances and
// the environment; and the light tree over the point and spot lights (section 4.16; device/dlighttree.h walks it), which gives them one entry in place of theirs.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "scene_build.h"
#include "../device/dlighttree.h"

namespace akr {

static const char* punct_kind_name(uint32_t type) { return type == AKR_LIGHT_POINT ? "point" : (type == AKR_LIGHT_SPOT ? "spot" : "sun"); }

std::string punctual_light_name(const CompiledScene& cs) {
    if (cs.punct.empty()) return "";
    return cs.punct[0].kind == PUNCT_POINT ? "point light" : (cs.punct[0].kind == PUNCT_SPOT ? "spot light" : "sun light");
}

bool punctual_from_desc(const akr_punctual_light_desc& d, akr_punctual_light_desc& out) {
    if (d.type > AKR_LIGHT_SUN) throw std::invalid_argument("punctual light: unknown type " + std::to_string(d.type));
    const std::string who = std::string(punct_kind_name(d.type)) + " light: ";
    if (!std::isfinite(d.strength) || d.strength < 0.0f) throw std::invalid_argument(who + "strength must be finite and >= 0");
    bool any = false;
    for (int c = 0; c < 3; c++) {
        if (!std::isfinite(d.color[c]) || d.color[c] < 0.0f) throw std::invalid_argument(who + "colour must be finite and >= 0");
        any = any || d.color[c] > 0.0f;
    }
    if (d.type != AKR_LIGHT_SUN)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(d.position[k])) throw std::invalid_argument(who + "position must be finite");
    if (d.type != AKR_LIGHT_POINT) {
        double l2 = 0.0;
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(d.direction[k])) throw std::invalid_argument(who + "direction must be finite");
            l2 += (double)d.direction[k] * d.direction[k];
        }
        if (!(l2 > 0.0)) throw std::invalid_argument(who + "direction must not be zero");
    }
    if (d.type == AKR_LIGHT_SPOT) {
        // (pi/2 as the f32 nearest to it: what a caller can pass)
        if (!std::isfinite(d.cone_angle) || !(d.cone_angle > 0.0f) || d.cone_angle > 1.57079637f) throw std::invalid_argument(who + "cone_angle (the outer half-angle) must be in (0, pi/2]");
        if (!std::isfinite(d.blend) || d.blend < 0.0f || d.blend > 1.0f) throw std::invalid_argument(who + "blend must be in [0, 1]");
    }
    // the soft size (section 4.15): a radius of a point / spot light, the full angular diameter of a sun; what the kind does not read is not looked at
    if (d.type != AKR_LIGHT_SUN && (!std::isfinite(d.radius) || d.radius < 0.0f)) throw std::invalid_argument(who + "radius must be finite and >= 0");
    if (d.type == AKR_LIGHT_SUN && (!std::isfinite(d.angle) || d.angle < 0.0f || (double)d.angle >= M_PI)) throw std::invalid_argument(who + "angle (the full angular diameter) must be in [0, pi)");
    out = d;
    // what the kind does not read is stored as zero: two descriptions of the same light compare equal
    if (d.type == AKR_LIGHT_SUN) out.position[0] = out.position[1] = out.position[2] = 0.0f;
    if (d.type == AKR_LIGHT_POINT) out.direction[0] = out.direction[1] = out.direction[2] = 0.0f;
    if (d.type != AKR_LIGHT_SPOT) out.cone_angle = out.blend = 0.0f;
    if (d.type == AKR_LIGHT_SUN || d.radius == 0.0f) out.radius = 0.0f;  // (and a -0 becomes the +0 whose bits say "delta")
    if (d.type != AKR_LIGHT_SUN || d.angle == 0.0f) out.angle = 0.0f;
    return any && d.strength > 0.0f;  // a strength of 0 or an all-zero colour: no light, as for the environment
}

DPunct fold_punctual(const akr_punctual_light_desc& d, uint32_t color) {
    DPunct r;
    std::memset(&r, 0, sizeof r);
    r.kind = d.type == AKR_LIGHT_POINT ? PUNCT_POINT : (d.type == AKR_LIGHT_SPOT ? PUNCT_SPOT : PUNCT_SUN);
    if (d.type != AKR_LIGHT_SUN) r.q = mk3(d.position[0], d.position[1], d.position[2]);
    if (d.type != AKR_LIGHT_POINT) {
        const double x = d.direction[0], y = d.direction[1], z = d.direction[2];
        const double len = std::sqrt((x * x + y * y) + z * z);
        r.a = mk3((float)(x / len), (float)(y / len), (float)(z / len));
    }
    if (d.type == AKR_LIGHT_SPOT) {
        r.cos_o = (float)std::cos((double)d.cone_angle);
        r.cos_i = (float)std::cos((double)d.cone_angle * (1.0 - (double)d.blend));
        r.inv_span = r.cos_i == r.cos_o ? 0.0f : 1.0f / (r.cos_i - r.cos_o);
    }
    // the soft size: zeros (a delta light) unless the light has one. cos_max > 0 for every angle < pi, so 0 can say "no angle".
    if (d.type != AKR_LIGHT_SUN) {
        r.radius = d.radius;
    } else if (d.angle > 0.0f) {
        const double cm = std::cos(0.5 * (double)d.angle);
        r.cos_max = (float)cm;
        r.k = (float)(2.0 / (1.0 + cm));
    }
    // colour x strength, then the way of an Emission material's constant colour into the session's pipeline (dbsdf.h convert_color_inputs: here, on the host)
    r.c = color_input(mk3(d.color[0] * d.strength, d.color[1] * d.strength, d.color[2] * d.strength), false, color);
    return r;
}

// the selection weight: "radiant power" on the scale of the triangle lights' estimate -- 4 pi I for a point light, the cone's solid angle (at the mean of
// its two cosines) x I for a spot, pi R^2 E for a sun over the scene's bounding sphere (R as scene_env.cpp computes it)
static float punctual_power(const DPunct& r, double R) {
    const double m = (double)max3(r.c);
    if (r.kind == PUNCT_POINT) return (float)((4.0 * M_PI) * m);
    if (r.kind == PUNCT_SPOT) return (float)(((2.0 * M_PI) * (1.0 - 0.5 * ((double)r.cos_i + (double)r.cos_o))) * m);
    return (float)(((M_PI * R) * R) * m);
}

// The light tree over the point and spot lights (device/dlighttree.h walks it). items: per local light its record's index in
// `recs` (the order given) and its f32 selection weight. A range of n >= 2 items splits at the object median of the positions along the axis of their
// largest f32 extent (ties: the lowest axis), sorted by (q[axis], index); the left child gets (n + 1) / 2. Deterministic, single-threaded.
namespace {
struct TreeItem {
    uint32_t record;
    float power;
};
struct BuildNode {
    float lo[3], hi[3], power;
    int left = -1, right = -1;  // BuildNode indices; a leaf has neither
    uint32_t record = 0;
};
float comp(const vec3& v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
int build_range(const std::vector<DPunct>& recs, std::vector<TreeItem>& items, size_t first, size_t n, std::vector<BuildNode>& nodes) {
    const int me = (int)nodes.size();
    nodes.emplace_back();
    if (n == 1) {
        const DPunct& r = recs[items[first].record];
        BuildNode& b = nodes[me];
        for (int a = 0; a < 3; a++) {
            b.lo[a] = comp(r.q, a) - r.radius;
            b.hi[a] = comp(r.q, a) + r.radius;
        }
        b.power = items[first].power;
        b.record = items[first].record;
        return me;
    }
    int axis = 0;
    float best = -1.0f;
    for (int a = 0; a < 3; a++) {
        float mn = comp(recs[items[first].record].q, a), mx = mn;
        for (size_t k = 1; k < n; k++) {
            const float v = comp(recs[items[first + k].record].q, a);
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        const float ext = mx - mn;
        if (ext > best) {
            best = ext;
            axis = a;
        }
    }
    std::sort(items.begin() + first, items.begin() + first + n, [&](const TreeItem& x, const TreeItem& y) {
        const float qx = comp(recs[x.record].q, axis), qy = comp(recs[y.record].q, axis);
        return qx < qy || (qx == qy && x.record < y.record);
    });
    const size_t nl = (n + 1) / 2;
    const int l = build_range(recs, items, first, nl, nodes);
    const int r = build_range(recs, items, first + nl, n - nl, nodes);
    BuildNode& b = nodes[me];
    const BuildNode &L = nodes[l], &R = nodes[r];
    for (int a = 0; a < 3; a++) {
        b.lo[a] = L.lo[a] < R.lo[a] ? L.lo[a] : R.lo[a];
        b.hi[a] = L.hi[a] > R.hi[a] ? L.hi[a] : R.hi[a];
    }
    b.power = L.power + R.power;
    b.left = l;
    b.right = r;
    return me;
}
}  // namespace

std::vector<uint32_t> build_light_tree(const std::vector<DPunct>& recs, const std::vector<float>& weights) {
    std::vector<TreeItem> items;
    for (size_t k = 0; k < recs.size(); k++)
        if (recs[k].kind != PUNCT_SUN) items.push_back(TreeItem{(uint32_t)k, weights[k]});
    std::vector<uint32_t> words;
    if (items.size() < 2) return words;
    std::vector<BuildNode> nodes;
    nodes.reserve(2 * items.size());
    build_range(recs, items, 0, items.size(), nodes);
    // breadth-first from a queue, root = node 0; the children of an inner node taken off the queue get the next two indices
    std::vector<int> order{0};
    std::vector<uint32_t> child_of;
    for (size_t head = 0; head < order.size(); head++) {
        const BuildNode& b = nodes[order[head]];
        if (b.left < 0) {
            child_of.push_back(kLightTreeLeafBit | b.record);
            continue;
        }
        child_of.push_back((uint32_t)order.size());
        order.push_back(b.left);
        order.push_back(b.right);
    }
    words.resize(8 * order.size());
    for (size_t k = 0; k < order.size(); k++) {
        const BuildNode& b = nodes[order[k]];
        const float f[7] = {b.lo[0], b.lo[1], b.lo[2], b.power, b.hi[0], b.hi[1], b.hi[2]};
        std::memcpy(&words[8 * k], f, sizeof f);
        words[8 * k + 7] = child_of[k];
    }
    return words;
}

std::vector<DPunct> punctual_device_records(const std::vector<DPunct>& recs, const std::vector<uint32_t>& tree) {
    std::vector<DPunct> all = recs;
    if (!tree.empty()) {
        all.resize(recs.size() + (tree.size() * 4 + sizeof(DPunct) - 1) / sizeof(DPunct));
        std::memset((void*)(all.data() + recs.size()), 0, (all.size() - recs.size()) * sizeof(DPunct));
        std::memcpy((void*)(all.data() + recs.size()), tree.data(), tree.size() * 4);
    }
    return all;
}

void compile_punctual(const FlatScene& flat, CompiledScene& out) {
    if (flat.punct.empty() && out.punct.empty()) return;  // (a scene without one keeps its tables exactly as compile_scene made them)
    size_t n_local = 0;
    for (const akr_punctual_light_desc& d : flat.punct) n_local += d.type != AKR_LIGHT_SUN ? 1u : 0u;
    const bool tree = flat.light_tree != 0 && n_local >= 2;  // (section 4.16: otherwise every table is what the scene without the mode has)
    size_t had = 0;  // the entries the lights have in the table now: behind the emissive instances', before the environment's
    for (uint32_t i : out.light_inst) had += (i == kPunctInst || i == kPunctTreeInst) ? 1u : 0u;
    if (!flat.punct.empty()) {
        const std::string who = std::string(punct_kind_name(flat.punct[0].type)) + " light";
        if (out.instanced.on)
            throw std::runtime_error("unsupported: the scene has a " + who + " and is kept as meshes + instances (option instancing); the kernels of kept scenes sample no punctual lights");
        if (out.bvh_nodes.empty()) {  // the exhaustive kernels read the light tables from LDS: scene_build.cpp sized the fit without these entries
            const size_t entries = tree ? flat.punct.size() - n_local + 1 : flat.punct.size();
            if (exhaustive_stage_bytes(out, out.light_inst.size() - had + entries) > kStageMaxBytes) throw std::runtime_error("unsupported: the scene's shading tables with its " + who + "s pass the exhaustive kernels' LDS budget");
        }
    }
    // the environment's entry is the last: taken off, put back behind the punctual lights
    const bool env = out.env.on;
    uint32_t env_entry[3] = {0, 0, 0};
    float env_power = 0.0f;
    auto pop = [&] {
        out.light_inst.pop_back();
        out.light_power.pop_back();
        out.light_tri_offset.pop_back();
        out.light_n_tris.pop_back();
    };
    if (env) {
        env_entry[0] = out.light_inst.back(); env_entry[1] = out.light_tri_offset.back(); env_entry[2] = out.light_n_tris.back();
        env_power = out.light_power.back();
        pop();
    }
    for (size_t k = 0; k < had; k++) pop();
    out.punct.clear();
    out.punct_tree.clear();
    double r2 = 0.0;
    for (int a = 0; a < 3; a++) {
        const double ext = (double)out.scene_hi[a] - (double)out.scene_lo[a];
        r2 += ext * ext;
    }
    double R = 0.5 * std::sqrt(r2);
    if (!(R > 0.0) || !std::isfinite(R)) R = 1.0;
    auto push = [&](uint32_t inst, float power) {
        out.light_inst.push_back(inst);
        out.light_power.push_back(power);
        out.light_tri_offset.push_back((uint32_t)out.area_entries.size());
        out.light_n_tris.push_back(0);
    };
    std::vector<float> weights;
    for (const akr_punctual_light_desc& d : flat.punct) {
        const DPunct r = fold_punctual(d, 0);
        out.punct.push_back(r);
        weights.push_back(punctual_power(r, R));
        if (!tree || r.kind == PUNCT_SUN) push(kPunctInst, weights.back());
    }
    if (tree) {  // one entry for all point and spot lights, behind the suns: the sum of their weights in double, rounded once
        double sum = 0.0;
        for (size_t k = 0; k < out.punct.size(); k++)
            if (out.punct[k].kind != PUNCT_SUN) sum += (double)weights[k];
        push(kPunctTreeInst, (float)sum);
        out.punct_tree = build_light_tree(out.punct, weights);
    }
    if (env) {
        out.light_inst.push_back(env_entry[0]);
        out.light_power.push_back(env_power);
        out.light_tri_offset.push_back(env_entry[1]);
        out.light_n_tris.push_back(env_entry[2]);
    }
    rebuild_light_alias(out);
}

}  // namespace akr
