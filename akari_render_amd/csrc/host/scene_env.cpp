// scene_env.cpp -- the environment light on the host: the description checked, the texels the kernels look up, the 2D piecewise-constant
// distribution they sample (device/denv.h) and the environment's entry in the light table.
//
// Distribution: one alias table over the rows (the marginal) and one per row over its columns (the conditional), from the texel weight
// max(r, g, b) of the 3x3 neighbourhood's maximum (u wraps, v clamps; the texel alone under nearest lookup) times sin(theta) at the texel
// centre -- so the pdf is nonzero wherever a bilinear lookup can return radiance. Selection weight in the light table: 4 pi R^2 Lbar, R half
// the diagonal of the scene's world bounds and Lbar the solid-angle-weighted mean of max(r, g, b) over the sphere by the same texel
// quadrature: "radiance x emitting area", the scale of the triangle lights' power estimate (load.rs:312-343).
#include <cmath>
#include <stdexcept>
#include <string>

#include "scene_build.h"

namespace akr {

HostEnvironment environment_from_desc(const akr_environment_desc& d) {
    if (!std::isfinite(d.strength) || d.strength < 0.0f) throw std::invalid_argument("environment: strength must be finite and >= 0");
    if ((d.width == 0) != (d.height == 0)) throw std::invalid_argument("environment: zero-size image (width and height must both be 0 for a constant colour, or both > 0)");
    if (d.filter != AKR_TEX_FILTER_NEAREST && d.filter != AKR_TEX_FILTER_LINEAR) throw std::invalid_argument("environment: unknown filter");
    if ((uint64_t)d.width * d.height > (1ull << 28)) throw std::invalid_argument("environment: image too large");
    {   // a rotation: R R^T = I and det R = +1, within 1e-4
        const float* r = d.rotation;
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(r[k])) throw std::invalid_argument("environment: the transform is not finite");
        double worst = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double dot = 0.0;
                for (int k = 0; k < 3; k++) dot += (double)r[3 * i + k] * r[3 * j + k];
                worst = std::max(worst, std::fabs(dot - (i == j ? 1.0 : 0.0)));
            }
        const double det = (double)r[0] * ((double)r[4] * r[8] - (double)r[5] * r[7]) - (double)r[1] * ((double)r[3] * r[8] - (double)r[5] * r[6]) +
                           (double)r[2] * ((double)r[3] * r[7] - (double)r[4] * r[6]);
        if (worst > 1e-4 || std::fabs(det - 1.0) > 1e-4)
            throw std::invalid_argument("environment: the transform must be a rotation (no scale, shear or mirror; tolerance 1e-4)");
    }
    HostEnvironment e;
    e.width = d.width;
    e.height = d.height;
    e.filter = d.filter;
    e.strength = d.strength;
    for (int k = 0; k < 9; k++) e.rotation[k] = d.rotation[k];
    bool any = false;
    if (d.width) {
        if (!d.texels) throw std::invalid_argument("environment: texels is NULL");
        e.texels.assign(d.texels, d.texels + 4ull * d.width * d.height);
        for (size_t t = 0; t < (size_t)d.width * d.height; t++)
            for (int c = 0; c < 3; c++) {
                const float v = e.texels[4 * t + c];
                if (!std::isfinite(v) || v < 0.0f) throw std::invalid_argument("environment: texels must be finite and >= 0");
                any = any || v > 0.0f;
            }
    } else {
        for (int c = 0; c < 3; c++) {
            if (!std::isfinite(d.color[c]) || d.color[c] < 0.0f) throw std::invalid_argument("environment: colour must be finite and >= 0");
            e.color[c] = d.color[c];
            any = any || d.color[c] > 0.0f;
        }
    }
    e.set = any && d.strength > 0.0f;  // a strength of 0 or an all-black image: no environment
    if (!e.set) return HostEnvironment{};
    return e;
}

void rebuild_light_alias(CompiledScene& out) {
    out.n_lights = (uint32_t)out.light_inst.size();
    out.light_entries.clear();
    out.light_pdf.clear();
    if (out.n_lights > 0) build_alias_table(out.light_power, out.light_entries, out.light_pdf);
}

void compile_environment(const FlatScene& flat, CompiledScene& out) {
    if (!flat.env.set && !out.env.on) return;  // (a scene without one keeps its tables exactly as compile_scene made them)
    if (flat.env.set && out.bvh_nodes.empty() && !out.instanced.on) {
        // the exhaustive kernels read the light tables from LDS: scene_build.cpp sized the fit without this entry
        if (exhaustive_stage_bytes(out, out.light_inst.size() + (out.env.on ? 0 : 1)) > kStageMaxBytes) throw std::runtime_error("unsupported: the scene's shading tables with an environment light pass the exhaustive kernels' LDS budget");
    }
    if (out.env.on) {  // the previous environment: the last light
        out.light_inst.pop_back();
        out.light_power.pop_back();
        out.light_tri_offset.pop_back();
        out.light_n_tris.pop_back();
        out.env = CompiledScene::Environment{};
    }
    if (!flat.env.set) {
        rebuild_light_alias(out);
        return;
    }
    const HostEnvironment& e = flat.env;
    CompiledScene::Environment env;
    const bool constant = e.width == 0;
    env.w = constant ? kEnvConstW : e.width;
    env.h = constant ? kEnvConstH : e.height;
    env.filter = constant ? (uint32_t)AKR_TEX_FILTER_NEAREST : e.filter;
    const uint32_t W = env.w, H = env.h;
    const size_t n = (size_t)W * H;
    env.texels.resize(4 * n);
    std::vector<float> m(n);  // max(r, g, b) per texel, strength applied
    for (size_t t = 0; t < n; t++) {
        for (int c = 0; c < 3; c++) env.texels[4 * t + c] = (constant ? e.color[c] : e.texels[4 * t + c]) * e.strength;
        env.texels[4 * t + 3] = 1.0f;
        m[t] = std::max(env.texels[4 * t], std::max(env.texels[4 * t + 1], env.texels[4 * t + 2]));
    }
    std::vector<float> weight(n), row_sum(H);
    double lbar_num = 0.0, lbar_den = 0.0;
    for (uint32_t y = 0; y < H; y++) {
        const double st = std::sin(M_PI * ((double)y + 0.5) / (double)H);
        double sum = 0.0;
        for (uint32_t x = 0; x < W; x++) {
            float mx = m[(size_t)y * W + x];
            if (env.filter == AKR_TEX_FILTER_LINEAR)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int yy = std::min(std::max((int)y + dy, 0), (int)H - 1);
                        const int xx = (int)((x + W + dx) % W);
                        mx = std::max(mx, m[(size_t)yy * W + xx]);
                    }
            const float w = (float)(mx * st);
            weight[(size_t)y * W + x] = w;
            sum += w;
            lbar_num += (double)m[(size_t)y * W + x] * st;
            lbar_den += st;
        }
        row_sum[y] = (float)sum;
    }
    double total = 0.0;
    for (float s : row_sum) total += s;
    if (!(total > 0.0)) {  // all black after all (cannot happen for a HostEnvironment that is set; kept for safety)
        rebuild_light_alias(out);
        return;
    }
    build_alias_table(row_sum, env.marginal_entries, env.marginal_pdf);
    env.conditional_entries.reserve(n);
    env.conditional_pdf.reserve(n);
    for (uint32_t y = 0; y < H; y++) {
        std::vector<float> row(weight.begin() + (size_t)y * W, weight.begin() + (size_t)(y + 1) * W);
        if (!(row_sum[y] > 0.0f)) row.assign(W, 1.0f);  // a row the marginal never picks: any valid table
        std::vector<AliasEntry> ent;
        std::vector<float> pdf;
        build_alias_table(row, ent, pdf);
        env.conditional_entries.insert(env.conditional_entries.end(), ent.begin(), ent.end());
        env.conditional_pdf.insert(env.conditional_pdf.end(), pdf.begin(), pdf.end());
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) env.rot_t[3 * i + j] = e.rotation[3 * j + i];
    double r2 = 0.0;
    for (int a = 0; a < 3; a++) {
        const double ext = (double)out.scene_hi[a] - (double)out.scene_lo[a];
        r2 += ext * ext;
    }
    double R = 0.5 * std::sqrt(r2);
    if (!(R > 0.0) || !std::isfinite(R)) R = 1.0;  // (a scene without geometry: the environment is the only light, its weight is moot)
    env.power = (float)(4.0 * M_PI * R * R * (lbar_num / lbar_den));
    env.on = true;
    out.env = std::move(env);
    out.light_inst.push_back(0xffffffffu);
    out.light_power.push_back(out.env.power);
    out.light_tri_offset.push_back((uint32_t)out.area_entries.size());
    out.light_n_tris.push_back(0);
    rebuild_light_alias(out);
}

}  // namespace akr
