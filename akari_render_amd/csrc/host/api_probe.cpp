// api_probe.cpp -- host-side known-answer hooks and device probes for the tests: the TEST HOOKS of libakari_hip.so, declared in
// include/akari_hip_test.h and compiled in only with -DAKR_TEST_HOOKS=1 (the in-tree test build; build.py). Shared internals: api_internal.h
#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
#include "api_internal.h"
#include "../../../include/akari_hip_test.h"
#include "../device/dinst.h"
#include "../device/disect.h"
#include "../device/dpath.h"

extern "C" {

// ------------------------------------------------------------------------------------------------ host KAT hooks
AKR_TEST_API int32_t akr_host_stdrng_u64(uint64_t seed, uint32_t n, uint64_t* out) {
    if (!out) return fail(AKR_ERR_INVALID_ARGUMENT, "out is NULL");
    StdRng rng(seed);
    for (uint32_t i = 0; i < n; i++) out[i] = rng.next_u64();
    return AKR_OK;
}
AKR_TEST_API int32_t akr_host_chacha_block(const uint32_t* key8, uint64_t counter, uint64_t stream, int32_t rounds, uint32_t* out16) {
    if (!key8 || !out16) return fail(AKR_ERR_INVALID_ARGUMENT, "NULL argument");
    StdRng::chacha_block(key8, counter, stream, rounds, out16);
    return AKR_OK;
}
AKR_TEST_API int32_t akr_host_pcg32_states(uint64_t seed, uint64_t n, uint64_t* out2n) {
    if (!out2n) return fail(AKR_ERR_INVALID_ARGUMENT, "out is NULL");
    StdRng rng(seed);
    for (uint64_t i = 0; i < n; i++) {
        Pcg32 p = pcg_new_seq_offset(i, rng.next_u64());
        out2n[2 * i] = p.state;
        out2n[2 * i + 1] = p.inc;
    }
    return AKR_OK;
}
AKR_TEST_API int32_t akr_host_pcg_start(uint64_t* state, uint64_t inc) {
    if (!state) return fail(AKR_ERR_INVALID_ARGUMENT, "state is NULL");
    Pcg32 p{*state, inc};
    pcg_start(p, pcg_start_constants());
    *state = p.state;
    return AKR_OK;
}
// device/drng.h pcg_end_pass on the host: the closed form the kernels use for the Drop of the independent sampler = advance(-dim)
AKR_TEST_API int32_t akr_host_pcg_end_pass(uint64_t* state, uint64_t inc, uint32_t dim) {
    if (!state) return fail(AKR_ERR_INVALID_ARGUMENT, "state is NULL");
    Pcg32 p{*state, inc};
    pcg_end_pass(p, dim);
    *state = p.state;
    return AKR_OK;
}
// device/drng.h on the host: reverse_bits32(sobol_dim1(i)) by the defining loop and by the five-step butterfly the kernels use
AKR_TEST_API int32_t akr_host_sobol_dim1(uint32_t n, const uint32_t* index, uint32_t* by_loop, uint32_t* by_butterfly) {
    if (!index || !by_loop || !by_butterfly) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_sobol_dim1: NULL argument");
    for (uint32_t k = 0; k < n; k++) {
        by_loop[k] = reverse_bits32(sobol_dim1(index[k]));
        by_butterfly[k] = sobol_dim1_reversed(index[k]);
    }
    return AKR_OK;
}
// device/drng.h fastmod_u32 on the host: a[k] % d[k] through the precomputed constant
AKR_TEST_API int32_t akr_host_fastmod(uint32_t n, const uint32_t* a, const uint32_t* d, uint32_t* out) {
    if (!a || !d || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_fastmod: NULL argument");
    for (uint32_t k = 0; k < n; k++) {
        if (d[k] == 0) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_fastmod: divisor 0");
        out[k] = fastmod_u32(a[k], fastmod_magic(d[k]), d[k]);
    }
    return AKR_OK;
}
// device/dinst.h on the host: the conservative reject of a candidate (tri_may_hit) next to the exact test it stands in front of
// (woop_precompute + tri_test), per item: ray = o.xyz d.xyz tmin tlimit, tri = A B C (world space, f32). exact: bit 0 accept, t in out_t.
AKR_TEST_API int32_t akr_host_tri_pretest(uint32_t n, const float* rays8, const float* tris9, float plane_shift, uint32_t* may, uint32_t* exact, float* out_t) {
    if (!rays8 || !tris9 || !may || !exact) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_tri_pretest: NULL argument");
    for (uint32_t k = 0; k < n; k++) {
        const float* r = rays8 + 8ull * k;
        const float* t = tris9 + 9ull * k;
        const vec3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]), A = mk3(t[0], t[1], t[2]), B = mk3(t[3], t[4], t[5]), C = mk3(t[6], t[7], t[8]);
        may[k] = tri_may_hit(o, d, A, B, C, r[6], r[7], plane_shift) ? 1u : 0u;
        float w[12], tt, u, v;
        woop_precompute(A, B, C, w);
        exact[k] = tri_test(o, d, make_float4(w[0], w[1], w[2], w[3]), make_float4(w[4], w[5], w[6], w[7]), make_float4(w[8], w[9], w[10], w[11]), r[6], r[7], tt, u, v) ? 1u : 0u;
        if (out_t) out_t[k] = tt;
    }
    return AKR_OK;
}
AKR_TEST_API int32_t akr_host_alias_table(const float* weights, uint32_t n, uint32_t* j, float* t, float* pdf) {
    if (!weights || !j || !t || !pdf || n == 0) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_alias_table: bad argument");
    return guarded([&] {
        std::vector<float> w(weights, weights + n), p;
        std::vector<AliasEntry> e;
        build_alias_table(w, e, p);
        for (uint32_t i = 0; i < n; i++) { j[i] = e[i].j; t[i] = e[i].t; pdf[i] = p[i]; }
    });
}

// ------------------------------------------------------------------------------------------------ probes
AKR_TEST_API int32_t akr_probe_math(akr_context* ctx, uint32_t n, const float* x, float* s, float* c, float* l) {
    if (!ctx || !x || !s || !c || !l) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_math: NULL argument");
    return guarded([&] {
        ctx->bind();
        DevBuf dx, ds, dc, dl;
        std::vector<float> xv(x, x + n);
        dx.upload(xv);
        ds.alloc(n * 4); dc.alloc(n * 4); dl.alloc(n * 4);
        if (n) HIP_CHECK(launch_probe_math(n, dx.as<float>(), ds.as<float>(), dc.as<float>(), dl.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(s, ds.p, n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(c, dc.p, n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(l, dl.p, n * 4, hipMemcpyDeviceToHost));
        }
    });
}
AKR_TEST_API int32_t akr_probe_math2(akr_context* ctx, uint32_t n, const float* xy, float* out6) {
    if (!ctx || !xy || !out6) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_math2: NULL argument");
    return guarded([&] {
        ctx->bind();
        DevBuf dxy, dout;
        dxy.upload(std::vector<float>(xy, xy + 2ull * n));
        dout.alloc(6ull * n * 4);
        if (n) HIP_CHECK(launch_probe_math2(n, dxy.as<float>(), dout.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) HIP_CHECK(hipMemcpy(out6, dout.p, 6ull * n * 4, hipMemcpyDeviceToHost));
    });
}
AKR_TEST_API int32_t akr_probe_div(akr_context* ctx, uint32_t n, const float* a, const float* b, float* out_fast, float* out_ieee) {
    if (!ctx || !a || !b || !out_fast || !out_ieee) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_div: NULL argument");
    return guarded([&] {
        ctx->bind();
        DevBuf da, db, df, di;
        da.upload(std::vector<float>(a, a + n));
        db.upload(std::vector<float>(b, b + n));
        df.alloc((size_t)n * 4); di.alloc((size_t)n * 4);
        if (n) HIP_CHECK(launch_probe_div(n, da.as<float>(), db.as<float>(), df.as<float>(), di.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(out_fast, df.p, (size_t)n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(out_ieee, di.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
    });
}
AKR_TEST_API int32_t akr_probe_pcg_end_pass(akr_context* ctx, uint32_t n, const uint64_t* state, const uint64_t* inc, const uint32_t* dim, uint64_t* out_closed, uint64_t* out_loop) {
    if (!ctx || !state || !inc || !dim || !out_closed || !out_loop) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_pcg_end_pass: NULL argument");
    return guarded([&] {
        ctx->bind();
        DevBuf ds, di, dd, dc, dl;
        ds.upload(std::vector<uint64_t>(state, state + n));
        di.upload(std::vector<uint64_t>(inc, inc + n));
        dd.upload(std::vector<uint32_t>(dim, dim + n));
        dc.alloc((size_t)n * 8); dl.alloc((size_t)n * 8);
        if (n) HIP_CHECK(launch_probe_pcg_end_pass(n, ds.as<uint64_t>(), di.as<uint64_t>(), dd.as<uint32_t>(), dc.as<uint64_t>(), dl.as<uint64_t>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(out_closed, dc.p, (size_t)n * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(out_loop, dl.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        }
    });
}
AKR_TEST_API int32_t akr_probe_bsdf(akr_context* ctx, const akr_material_desc* m, const float* table, int32_t mode, const float* wo, uint32_t n,
                               const float* in, float* out) {
    if (!ctx || !m || !wo || !in || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_bsdf: NULL argument");
    return guarded([&] {
        ctx->bind();
        std::vector<DMaterial> dm(1, fold_material(*m));
        DevBuf dmat, dtab, din, dout;
        dmat.upload(dm);
        std::vector<float> tab(4096, 0.0f);
        if (table) tab.assign(table, table + 4096);
        dtab.upload(tab);
        std::vector<float> inv(in, in + 3ull * n);
        din.upload(inv);
        size_t out_n = (mode == 0 ? 4ull : 8ull) * n;
        dout.alloc(out_n * 4);
        if (n) HIP_CHECK(launch_probe_bsdf(dmat.as<DMaterial>(), dtab.as<float>(), mode, wo, n, din.as<float>(), dout.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) HIP_CHECK(hipMemcpy(out, dout.p, out_n * 4, hipMemcpyDeviceToHost));
    });
}
static PtParams probe_params(akr_scene* s) {
    PtParams p;
    std::memset(&p, 0, sizeof p);
    p.sc = s->dscene;
    p.tex_slots = s->cs.has_textures ? s->cs.tex_slots : 0;
    return p;
}
AKR_TEST_API int32_t akr_probe_intersect(akr_context* ctx, akr_scene* scene, uint32_t n, const float* rays, uint32_t* hit_inst_prim, float* bary) {
    if (!ctx || !scene || !rays || !hit_inst_prim || !bary) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_intersect: NULL argument");
    return guarded([&] {
        ctx->bind();
        DevBuf dr, dout, db;
        std::vector<float> rv(rays, rays + 8ull * n);
        dr.upload(rv);
        dout.alloc(3ull * n * 4);
        db.alloc(2ull * n * 4);
        if (n) HIP_CHECK(launch_probe_intersect(probe_params(scene), n, dr.as<float>(), dout.as<uint32_t>(), db.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(hit_inst_prim, dout.p, 3ull * n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(bary, db.p, 2ull * n * 4, hipMemcpyDeviceToHost));
        }
    });
}
AKR_TEST_API int32_t akr_probe_intersect_pair(akr_context* ctx, akr_scene* scene, uint32_t n, const float* rays16, const uint32_t* excl3, uint32_t* out4, float* tuv3) {
    if (!ctx || !scene || !rays16 || !excl3 || !out4 || !tuv3) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_intersect_pair: NULL argument");
    if (scene->ctx != ctx) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_intersect_pair: scene belongs to another context");
    if (scene->dscene.bvh_nodes || scene->dscene.in2.on || scene->dscene.n_tris > 64)
        return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_intersect_pair: the pair walk serves scenes of at most 64 triangles");
    return guarded([&] {
        ctx->bind();
        DevBuf dr, de, dout, dt;
        dr.upload(std::vector<float>(rays16, rays16 + 16ull * n));
        de.upload(std::vector<uint32_t>(excl3, excl3 + 3ull * n));
        dout.alloc(4ull * n * 4);
        dt.alloc(3ull * n * 4);
        if (n) HIP_CHECK(launch_probe_intersect_pair(probe_params(scene), n, dr.as<float>(), de.as<uint32_t>(), dout.as<uint32_t>(), dt.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(out4, dout.p, 4ull * n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(tuv3, dt.p, 3ull * n * 4, hipMemcpyDeviceToHost));
        }
    });
}
// the environment light's sampler (device/denv.h): n points u -> wi, pdf, valid; n directions -> pdf, radiance (default colour pipeline)
static int32_t probe_env(akr_context* ctx, akr_scene* scene, uint32_t mode, uint32_t n, const float* in, float* out, const char* name) {
    if (!ctx || !scene || !in || !out) return fail(AKR_ERR_INVALID_ARGUMENT, std::string(name) + ": NULL argument");
    if (scene->ctx != ctx || !scene->cs.env.on) return fail(AKR_ERR_INVALID_ARGUMENT, std::string(name) + ": the scene has no environment light on this context");
    return guarded([&] {
        ctx->bind();
        const size_t n_in = (mode == 0 ? 2ull : 3ull) * n, n_out = (mode == 0 ? 5ull : 4ull) * n;
        DevBuf din, dout;
        din.upload(std::vector<float>(in, in + n_in));
        dout.alloc(n_out * 4);
        if (n) HIP_CHECK(launch_probe_env(probe_params(scene), mode, n, din.as<float>(), dout.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) HIP_CHECK(hipMemcpy(out, dout.p, n_out * 4, hipMemcpyDeviceToHost));
    });
}
AKR_TEST_API int32_t akr_probe_env_sample(akr_context* ctx, akr_scene* scene, uint32_t n, const float* u2, float* out5) {
    return probe_env(ctx, scene, 0, n, u2, out5, "akr_probe_env_sample");
}
AKR_TEST_API int32_t akr_probe_env_pdf(akr_context* ctx, akr_scene* scene, uint32_t n, const float* dirs3, float* out4) {
    return probe_env(ctx, scene, 1, n, dirs3, out4, "akr_probe_env_pdf");
}
// next-event estimation with punctual lights (device/dpunct.h): the selection and the lights' branch of sample_direct, row by row.
// The seven-column hooks are the nine-column ones with u_sample = (0.5, 0.5).
static std::vector<float> rows9_of_rows7(uint32_t n, const float* rows7) {
    std::vector<float> r(9ull * n);
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 7; k++) r[9ull * i + k] = rows7[7ull * i + k];
        r[9ull * i + 7] = r[9ull * i + 8] = 0.5f;
    }
    return r;
}
AKR_TEST_API int32_t akr_host_light_sample_soft(const akr_scene* scene, uint32_t n, const float* rows9, float* out13, uint32_t* light) {
    if (!scene || !rows9 || !out13 || !light) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_light_sample_soft: NULL argument");
    return guarded([&] {
        std::vector<AliasPacked> la, aa;
        std::vector<LightRec> lr;
        packed_light_tables(scene->cs, la, aa, lr);
        for (uint32_t i = 0; i < n; i++) punct_probe_row(la.data(), lr.data(), scene->cs.punct.data(), scene->cs.n_lights, rows9 + 9ull * i, out13 + 13ull * i, light + i);
    });
}
AKR_TEST_API int32_t akr_host_light_sample(const akr_scene* scene, uint32_t n, const float* rows7, float* out13, uint32_t* light) {
    if (!scene || !rows7 || !out13 || !light) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_light_sample: NULL argument");
    return akr_host_light_sample_soft(scene, n, rows9_of_rows7(n, rows7).data(), out13, light);
}
AKR_TEST_API int32_t akr_probe_light_sample_soft(akr_context* ctx, akr_scene* scene, uint32_t n, const float* rows9, float* out13, uint32_t* light) {
    if (!ctx || !scene || !rows9 || !out13 || !light) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_light_sample_soft: NULL argument");
    if (scene->ctx != ctx) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_light_sample_soft: the scene was not created on this context");
    return guarded([&] {
        ctx->bind();
        DevBuf din, dout, dl;
        din.upload(std::vector<float>(rows9, rows9 + 9ull * n));
        dout.alloc(13ull * n * 4);
        dl.alloc(4ull * n);
        if (n) HIP_CHECK(launch_probe_light_sample(probe_params(scene), n, din.as<float>(), dout.as<float>(), dl.as<uint32_t>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(out13, dout.p, 13ull * n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(light, dl.p, 4ull * n, hipMemcpyDeviceToHost));
        }
    });
}
AKR_TEST_API int32_t akr_probe_light_sample(akr_context* ctx, akr_scene* scene, uint32_t n, const float* rows7, float* out13, uint32_t* light) {
    if (!ctx || !scene || !rows7 || !out13 || !light) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_light_sample: NULL argument");
    return akr_probe_light_sample_soft(ctx, scene, n, rows9_of_rows7(n, rows7).data(), out13, light);
}
// the same rows over a scene that may have a light tree (device/dlighttree.h)
AKR_TEST_API int32_t akr_host_light_tree_sample(const akr_scene* scene, uint32_t n, const float* rows9, float* out13, uint32_t* light, uint32_t* record) {
    if (!scene || !rows9 || !out13 || !light || !record) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_light_tree_sample: NULL argument");
    return guarded([&] {
        std::vector<AliasPacked> la, aa;
        std::vector<LightRec> lr;
        packed_light_tables(scene->cs, la, aa, lr);
        const std::vector<DPunct> recs = punctual_device_records(scene->cs.punct, scene->cs.punct_tree);
        const uint32_t tree = scene->cs.punct_tree.empty() ? 0u : (uint32_t)scene->cs.punct.size();
        for (uint32_t i = 0; i < n; i++) light_tree_probe_row(la.data(), lr.data(), recs.data(), tree, scene->cs.n_lights, rows9 + 9ull * i, out13 + 13ull * i, light + i, record + i);
    });
}
AKR_TEST_API int32_t akr_probe_light_tree_sample(akr_context* ctx, akr_scene* scene, uint32_t n, const float* rows9, float* out13, uint32_t* light, uint32_t* record) {
    if (!ctx || !scene || !rows9 || !out13 || !light || !record) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_light_tree_sample: NULL argument");
    if (scene->ctx != ctx) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_light_tree_sample: the scene was not created on this context");
    return guarded([&] {
        ctx->bind();
        DevBuf din, dout, dl, dr;
        din.upload(std::vector<float>(rows9, rows9 + 9ull * n));
        dout.alloc(13ull * n * 4);
        dl.alloc(4ull * n);
        dr.alloc(4ull * n);
        if (n) HIP_CHECK(launch_probe_light_tree_sample(probe_params(scene), n, din.as<float>(), dout.as<float>(), dl.as<uint32_t>(), dr.as<uint32_t>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) {
            HIP_CHECK(hipMemcpy(out13, dout.p, 13ull * n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(light, dl.p, 4ull * n, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(record, dr.p, 4ull * n, hipMemcpyDeviceToHost));
        }
    });
}
// the camera's ray generation (device/dpath.h): the parameter block's camera part, filled by the sessions' own function
static PtParams probe_camera_params(const akr_scene* s, uint32_t filter_type, float filter_radius) {
    PtParams p;
    std::memset(&p, 0, sizeof p);
    camera_params(p, s, filter_type, filter_radius);
    return p;
}
AKR_TEST_API int32_t akr_host_lens_ray(const akr_scene* scene, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t* pixels2, const float* u4, float* out6) {
    if (!scene || !pixels2 || !u4 || !out6) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_lens_ray: NULL argument");
    if (filter_type > AKR_FILTER_GAUSSIAN) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_lens_ray: unknown filter_type");
    const PtParams p = probe_camera_params(scene, filter_type, filter_radius);
    for (uint32_t i = 0; i < n; i++) {
        const float* u = u4 + 4ull * i;
        vec3 o, d;
        if (camera_runs_lens_kernels(p.lens_radius, p.projection)) generate_ray_lens_from(p, pixels2[2ull * i], pixels2[2ull * i + 1], mk2(u[0], u[1]), mk2(u[2], u[3]), o, d);
        else generate_ray_from(p, pixels2[2ull * i], pixels2[2ull * i + 1], mk2(u[0], u[1]), o, d);
        float* r = out6 + 6ull * i;
        r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
    }
    return AKR_OK;
}
// What akr_pt_begin decides for (scene, config) under the options `opt`, without a session or a device: the session's route (pt_route; its refusal is
// thrown), of it the variant and the staged tables, the per-scene kernel's wrapper text, and the LDS layout a launch of the whole frame would
// get (launch_pt_pass: pt_lds_layout). feat: the route of akr_pt_begin_features; -> the variant and the layout
static std::pair<PtVariant, PtLdsLayout> fill_launch_plan(akr_scene* scene, const akr_pt_config* cfg, const TuningOptions& opt, bool feat, akr_pt_launch_plan* out) {
        const CompiledScene& cs = scene->cs;
        const TileGrid grid = tile_grid(cfg->tile_w, cfg->tile_h, scene->flat.camera.width, scene->flat.camera.height, cfg->shard_rank, cfg->shard_count);
        const PtRoute route = pt_route(scene, *cfg, opt, grid, feat, /*cost_order=*/1);
        if (!route.refusal.empty()) throw Unsupported(route.refusal);
        const PtPlan& pl = route.plan;
        const PtVariant& v = pl.v;
        const PtLdsSizes sizes{scene_stack_depth(cs), cs.n_tris, scene_n_nodes(cs), pl.tex_slots, pl.stage_total, cfg->sampler_type == AKR_SAMPLER_PMJ02BN};
        const PtLdsLayout L = pt_lds_layout(v, sizes);
        std::memset(out, 0, sizeof *out);
        const bool flags[10] = {v.bvh, v.fd, v.tex, v.pmj, v.stage, v.defer, v.simple, v.inst, v.env, v.lens};
        for (int i = 0; i < 10; i++) out->variant[i] = flags[i] ? 1u : 0u;
        out->simple_scene = pl.simple_scene; out->defer_metal = pl.defer_metal; out->defer_flags = pl.defer_flags;
        std::memcpy(out->stage_bytes, pl.stage_bytes, sizeof out->stage_bytes);
        out->stage_total = pl.stage_total;
        out->tile_offset = L.tile_offset; out->bvh_tile_nodes = L.tile_nodes; out->park_offset = L.park_offset; out->carry_offset = L.carry_offset;
        out->bn_offset = L.bn_offset; out->val_offset_words = L.val_offset_words;
        out->lds_bytes = (uint32_t)L.total_bytes;
        out->blocks = (grid.n_items + 255u) / 256u;
        out->specialised = route.spec ? 1u : 0u;
        out->punct = v.punct ? 1u : 0u;
        if (route.spec) std::snprintf(out->wrapper, sizeof out->wrapper, "%s", spec_wrapper_source(v, route.spec_waves).c_str());
        return {v, L};
}
// the options a plan hook decides from: the defaults, and those the test gives (not the process's). spec_waves != 0: a per-scene kernel of that many waves
static TuningOptions plan_options(int32_t defer_metal, int32_t simple_kernels, int32_t defer_on, int32_t spec_waves) {
    TuningOptions t;
    t.defer_metal = defer_metal;
    t.simple_kernels = simple_kernels;
    t.defer_on = defer_on;
    t.specialise = spec_waves != 0 ? 1 : 0;
    t.specialise_waves = spec_waves;
    return t;
}
AKR_TEST_API int32_t akr_host_pt_launch_plan(akr_scene* scene, const akr_pt_config* cfg, int32_t defer_metal, int32_t simple_kernels, int32_t defer_on, int32_t spec_waves,
                                             akr_pt_launch_plan* out) {
    if (!scene || !cfg || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_pt_launch_plan: NULL argument");
    return guarded([&] { fill_launch_plan(scene, cfg, plan_options(defer_metal, simple_kernels, defer_on, spec_waves), false, out); });
}
// akr_host_pt_launch_plan for a session that may collect the denoiser's guides, under options wavefront and arith as given: the route's refusals, those
// of akr_pt_begin_features that need no device among them, then the plan and what a test needs to know of the layout's sizes
AKR_TEST_API int32_t akr_host_pt_features_plan(akr_scene* scene, const akr_pt_config* cfg, int32_t defer_metal, int32_t simple_kernels, int32_t defer_on, int32_t spec_waves, int32_t feat,
                                               int32_t wavefront, int32_t arith, akr_pt_features_plan* out) {
    if (!scene || !cfg || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_pt_features_plan: NULL argument");
    return guarded([&] {
        TuningOptions t = plan_options(defer_metal, simple_kernels, defer_on, spec_waves);
        t.wavefront = wavefront;
        t.arith = arith;
        std::memset(out, 0, sizeof *out);
        const auto vl = fill_launch_plan(scene, cfg, t, feat != 0, &out->plan);
        out->feat = vl.first.feat ? 1u : 0u;
        out->kernel_compiled = pt_variant_compiled(vl.first) ? 1u : 0u;
        out->park_slots = (vl.second.carry_offset - vl.second.park_offset) / 256u;
        out->required_bytes = (uint32_t)vl.second.required_bytes;
        out->lds_budget = (uint32_t)pt_lds_budget(vl.first.tex);
        out->park_slots_feat = kParkSlotsFeat;
    });
}
AKR_TEST_API int32_t akr_host_option_info(uint32_t index, akr_option_info* out) {
    OptionInfo o;
    if (!out || !tuning_info(index, &o)) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_option_info: out is NULL or index is past the table's last row");
    *out = {o.name, o.env, o.def, o.ranged, o.lo, o.hi};
    return AKR_OK;
}
AKR_TEST_API int32_t akr_probe_pt_cost_order_mode(int32_t mode, int32_t* previous) {
    if (mode < 0 || mode > 2) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_pt_cost_order_mode: mode must be 0, 1 or 2");
    const int before = cost_order_mode_set(mode);
    if (previous) *previous = before;
    return AKR_OK;
}
AKR_TEST_API int32_t akr_probe_pt_cost_order(akr_pt_session* se, uint32_t* state, uint32_t* cost, uint32_t* table, uint32_t capacity, uint32_t* n_table, float* sort_ms) {
    if (!se || !state || !n_table) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_pt_cost_order: NULL argument");
    return guarded([&] {
        se->ctx->bind();
        HIP_CHECK(hipStreamSynchronize(se->ctx->stream));
        *state = (uint32_t)se->cost.state;
        *n_table = (uint32_t)(se->cost.item_pixels.bytes / sizeof(uint32_t));
        if (cost) {
            if (!se->cost.item_cost.p || se->active_set) throw std::invalid_argument("akr_probe_pt_cost_order: the session has no cost map, or renders an active-tile list");
            DevBuf map;  // the items' costs, pixel by pixel (the session's own items: dealt by position, whatever the table says)
            map.alloc(se->film->n_floats() / 7 * sizeof(uint32_t));
            HIP_CHECK(hipMemsetAsync(map.p, 0, map.bytes, se->ctx->stream));
            HIP_CHECK(launch_cost_to_pixels(se->params, se->cost.item_cost.as<uint32_t>(), map.as<uint32_t>(), se->ctx->stream));
            HIP_CHECK(hipStreamSynchronize(se->ctx->stream));
            HIP_CHECK(hipMemcpy(cost, map.p, map.bytes, hipMemcpyDeviceToHost));
        }
        if (table && *n_table) {
            if (capacity < *n_table) throw std::invalid_argument("akr_probe_pt_cost_order: the table has " + std::to_string(*n_table) + " entries");
            HIP_CHECK(hipMemcpy(table, se->cost.item_pixels.p, se->cost.item_pixels.bytes, hipMemcpyDeviceToHost));
        }
        if (sort_ms) {
            *sort_ms = 0.0f;
            if (se->cost.ev1) HIP_CHECK(hipEventElapsedTime(sort_ms, se->cost.ev0, se->cost.ev1));
        }
    });
}
AKR_TEST_API int32_t akr_probe_camera_rays(akr_context* ctx, akr_scene* scene, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t* pixels2,
                                      const float* u4, float* out6) {
    if (!ctx || !scene || !pixels2 || !u4 || !out6) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_camera_rays: NULL argument");
    if (filter_type > AKR_FILTER_GAUSSIAN) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_camera_rays: unknown filter_type");
    return guarded([&] {
        ctx->bind();
        DevBuf dpx, du, dout;
        dpx.upload(std::vector<uint32_t>(pixels2, pixels2 + 2ull * n));
        du.upload(std::vector<float>(u4, u4 + 4ull * n));
        dout.alloc(6ull * n * 4);
        if (n) HIP_CHECK(launch_probe_camera_rays(probe_camera_params(scene, filter_type, filter_radius), n, dpx.as<uint32_t>(), du.as<float>(), dout.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) HIP_CHECK(hipMemcpy(out6, dout.p, 6ull * n * 4, hipMemcpyDeviceToHost));
    });
}
AKR_TEST_API int32_t akr_probe_surface_interaction(akr_context* ctx, akr_scene* scene, uint32_t n, const uint32_t* inst_prim, const float* bary,
                                              float* out) {
    if (!ctx || !scene || !inst_prim || !bary || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_surface_interaction: NULL argument");
    return guarded([&] {
        ctx->bind();
        for (uint32_t i = 0; i < n; i++) {
            uint32_t inst = inst_prim[2 * i], prim = inst_prim[2 * i + 1];
            if (inst >= scene->flat.instances.size() || prim >= scene->flat.meshes[scene->flat.instances[inst].mesh].n_triangles())
                throw std::invalid_argument("akr_probe_surface_interaction: (inst, prim) out of range");
        }
        DevBuf dip, db, dout;
        std::vector<uint32_t> ipv(inst_prim, inst_prim + 2ull * n);
        std::vector<float> bv(bary, bary + 2ull * n);
        dip.upload(ipv);
        db.upload(bv);
        dout.alloc(19ull * n * 4);
        if (n) HIP_CHECK(launch_probe_si(probe_params(scene), n, dip.as<uint32_t>(), db.as<float>(), dout.as<float>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) HIP_CHECK(hipMemcpy(out, dout.p, 19ull * n * 4, hipMemcpyDeviceToHost));
    });
}

AKR_TEST_API int32_t akr_host_pmj02bn_tables(uint32_t* sets, uint16_t* bluenoise) {
    return guarded([&] {
        if (sets) {
            std::vector<uint32_t> v;
            make_pmj02_sets(v);
            std::memcpy(sets, v.data(), v.size() * 4);
        }
        if (bluenoise) {
            std::vector<uint16_t> v;
            load_bluenoise(v);
            std::memcpy(bluenoise, v.data(), v.size() * 2);
        }
    });
}
// PNG reader of the scene loader, exposed for tests: rgba == NULL returns the size only.
AKR_TEST_API int32_t akr_host_decode_png(const uint8_t* data, uint64_t len, uint32_t* width, uint32_t* height, uint8_t* rgba, uint64_t capacity) {
    if (!data || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_decode_png: NULL argument");
    return guarded([&] {
        std::vector<uint8_t> px;
        decode_png(data, (size_t)len, *width, *height, px);
        if (rgba) {
            if (capacity < px.size()) throw std::invalid_argument("akr_host_decode_png: output buffer too small");
            std::memcpy(rgba, px.data(), px.size());
        }
    });
}
AKR_TEST_API int32_t akr_host_decode_jpeg(const uint8_t* data, uint64_t len, uint32_t* width, uint32_t* height, uint8_t* rgba, uint64_t capacity) {
    if (!data || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_decode_jpeg: NULL argument");
    return guarded([&] {
        std::vector<uint8_t> px;
        decode_jpeg(data, (size_t)len, *width, *height, px);
        if (rgba) {
            if (capacity < px.size()) throw std::invalid_argument("akr_host_decode_jpeg: output buffer too small");
            std::memcpy(rgba, px.data(), px.size());
        }
    });
}
AKR_TEST_API int32_t akr_host_decode_tiff(const uint8_t* data, uint64_t len, uint32_t* width, uint32_t* height, uint8_t* rgba, uint64_t capacity) {
    if (!data || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_decode_tiff: NULL argument");
    return guarded([&] {
        std::vector<uint8_t> px;
        decode_tiff(data, (size_t)len, *width, *height, px);
        if (rgba) {
            if (capacity < px.size()) throw std::invalid_argument("akr_host_decode_tiff: output buffer too small");
            std::memcpy(rgba, px.data(), px.size());
        }
    });
}
AKR_TEST_API int32_t akr_host_decode_dds(const uint8_t* data, uint64_t len, uint32_t* width, uint32_t* height, uint8_t* rgba, uint64_t capacity) {
    if (!data || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_decode_dds: NULL argument");
    return guarded([&] {
        std::vector<uint8_t> px;
        decode_dds(data, (size_t)len, *width, *height, px);
        if (rgba) {
            if (capacity < px.size()) throw std::invalid_argument("akr_host_decode_dds: output buffer too small");
            std::memcpy(rgba, px.data(), px.size());
        }
    });
}
AKR_TEST_API int32_t akr_host_decode_exr(const uint8_t* data, uint64_t len, uint32_t* width, uint32_t* height, float* rgba, uint64_t capacity_floats) {
    if (!data || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_decode_exr: NULL argument");
    return guarded([&] {
        std::vector<float> px;
        decode_exr(data, (size_t)len, *width, *height, px);
        if (rgba) {
            if (capacity_floats < px.size()) throw std::invalid_argument("akr_host_decode_exr: output buffer too small");
            std::memcpy(rgba, px.data(), px.size() * sizeof(float));
        }
    });
}
// Evaluated inputs of a material at uv points: on the device (ctx != NULL; needs a scene with textures) or with the
// same code on the host (ctx == NULL).
// The same on the host for an arbitrary colour pipeline: the material tables are compiled for `color` (what akr_pt_begin does
// for a session with akr_pt_config.color != 0) and evaluated with the code the kernels run.
AKR_TEST_API int32_t akr_probe_material_inputs_host(akr_scene* scene, uint32_t material, uint32_t color, uint32_t n, const float* uv, float* out26) {
    if (!scene || !uv || !out26) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_material_inputs_host: NULL argument");
    if (material >= scene->flat.materials.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_material_inputs_host: material out of range");
    return guarded([&] {
        CompiledScene tmp;
        tmp.images = scene->cs.images;
        std::vector<akr_material_desc> descs;
        compile_materials(scene->flat, color, tmp, descs);
        const TexScene ts{tmp.tex_nodes.data(), scene->cs.images.data(), scene->cs.texels.data(), tmp.mat_inputs.data(), color, 0};
        const DMaterial& m = tmp.materials[material];
        for (uint32_t i = 0; i < n; i++) {
            MatInputs in;
            std::memcpy(&in, &descs[material], sizeof in);
            if (m.flags & MF_TEXTURED) {
                eval_material_graph(ts, m.tex_first_node, m.tex_n_nodes & kTexCountMask, mk2(uv[2 * i], uv[2 * i + 1]), in);
            }
            std::memcpy(out26 + 26ull * i, &in, sizeof in);
        }
    });
}

// The interpreter's view of a material at n uv points, on the host, default colour pipeline: material_at (the folded record, 64
// words), material_alpha_at and material_emission_inputs_at (device/dtex.h). What a per-scene kernel's generated code must
// reproduce bit for bit (tests/test_specialise.py compiles that text for the host and compares).
AKR_TEST_API int32_t akr_probe_material_folded_host(akr_scene* scene, uint32_t material, uint32_t n, const float* uv, uint32_t* out64, float* alpha, float* emission3) {
    if (!scene || !uv || !out64) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_material_folded_host: NULL argument");
    if (material >= scene->cs.materials.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_material_folded_host: material out of range");
    return guarded([&] {
        const CompiledScene& cs = scene->cs;
        const TexScene ts{cs.tex_nodes.data(), cs.images.data(), cs.texels.data(), cs.mat_inputs.data(), 0, 0};
        const DMaterial& folded = cs.materials[material];
        for (uint32_t i = 0; i < n; i++) {
            const vec2 p = mk2(uv[2 * i], uv[2 * i + 1]);
            DMaterial m = folded;
            material_at(ts, material, p, m);
            std::memcpy(out64 + 64ull * i, &m, sizeof m);
            const bool tex = (folded.flags & MF_TEXTURED) != 0;
            if (alpha) alpha[i] = tex ? material_alpha_at(ts, folded, material, p) : folded.base_alpha;
            if (emission3) {
                const vec3 e = tex ? material_emission_inputs_at(ts, folded, material, p) : folded.emission;
                emission3[3 * i] = e.x; emission3[3 * i + 1] = e.y; emission3[3 * i + 2] = e.z;
            }
        }
    });
}

AKR_TEST_API int32_t akr_probe_material_inputs(akr_context* ctx, akr_scene* scene, uint32_t material, uint32_t n, const float* uv, float* out26) {
    if (!scene || !uv || !out26) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_material_inputs: NULL argument");
    if (material >= scene->flat.materials.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_material_inputs: material out of range");
    return guarded([&] {
        const CompiledScene& cs = scene->cs;
        if (!ctx) {
            const TexScene ts{cs.tex_nodes.data(), cs.images.data(), cs.texels.data(), cs.mat_inputs.data(), 0, 0};
            const DMaterial& m = cs.materials[material];
            for (uint32_t i = 0; i < n; i++) {
                MatInputs in;
                if (cs.has_textures) in = cs.mat_inputs[material];
                else std::memcpy(&in, &scene->flat.materials[material], sizeof in);
                if (m.flags & MF_TEXTURED) {
                    eval_material_graph(ts, m.tex_first_node, m.tex_n_nodes & kTexCountMask, mk2(uv[2 * i], uv[2 * i + 1]), in);
                }
                std::memcpy(out26 + 26ull * i, &in, sizeof in);
            }
            return;
        }
        if (!cs.has_textures) throw std::invalid_argument("akr_probe_material_inputs: the scene has no textured material");
        if (scene->ctx != ctx) throw std::invalid_argument("akr_probe_material_inputs: scene belongs to another context");
        ctx->bind();
        DevBuf duv, dout;
        std::vector<float> uvv(uv, uv + 2ull * n);
        duv.upload(uvv);
        dout.alloc(26ull * n * 4);
        if (n) HIP_CHECK(launch_probe_material(probe_params(scene), material, n, duv.as<float>(), dout.as<uint32_t>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n) HIP_CHECK(hipMemcpy(out26, dout.p, 26ull * n * 4, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
#endif  // AKR_TEST_HOOKS
