/* akari_hip_test.h -- TEST HOOKS of libakari_hip.so. Not part of the drop-in boundary.
 *
 * include/akari_hip.h is what a host application binds. The entry points below exist so that the test suite can
 * compare single pieces of the library with the oracle -- the host's random number generators and table builders, the image decoders,
 * single device functions (elementary functions, BSDF, intersection, surface interaction, shader-graph evaluation) -- through the
 * same C ABI the product is called through. They are compiled into the library, and exported, only when it is built with
 * -DAKR_TEST_HOOKS=1: the in-tree build that `python -m akari_render_amd.build` makes for the tests sets it; a build with
 * AKR_SHIP=1 in the environment leaves them out (tests/test_abi.py checks both symbol sets against the library it loads).
 */
#ifndef AKARI_HIP_TEST_H
#define AKARI_HIP_TEST_H

#include "akari_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AKR_TEST_API AKR_API

/* Host-side pieces exposed for known-answer tests (no GPU needed):
 *   akr_host_stdrng_u64      rand 0.8 StdRng::seed_from_u64(seed) then n x gen::<u64>() (sampler/mod.rs:150-151)
 *   akr_host_chacha_block    one ChaCha block with `rounds` rounds (RFC 7539 / zero-key vectors pin the core)
 *   akr_host_pcg32_states    init_pcg32_buffer_with_seed on the host: 2 x u64 (state, inc) per entry
 *   akr_host_pcg_start       the closed form the kernels use for sampler.start() = advance(16384)
 *   akr_host_pcg_end_pass    the closed form the kernels use for the Drop of the independent sampler = advance(-dim)
 *   akr_host_alias_table     AliasTable::new (util/distribution.rs:35-78) */
AKR_TEST_API int32_t akr_host_stdrng_u64(uint64_t seed, uint32_t n, uint64_t *out);

AKR_TEST_API int32_t akr_host_chacha_block(const uint32_t *key8, uint64_t counter, uint64_t stream, int32_t rounds, uint32_t *out16);

AKR_TEST_API int32_t akr_host_pcg32_states(uint64_t seed, uint64_t n, uint64_t *out2n);

AKR_TEST_API int32_t akr_host_pcg_start(uint64_t *state, uint64_t inc);

AKR_TEST_API int32_t akr_host_pcg_end_pass(uint64_t *state, uint64_t inc, uint32_t dim);

AKR_TEST_API int32_t akr_host_sobol_dim1(uint32_t n, const uint32_t *index, uint32_t *by_loop, uint32_t *by_butterfly);

/* The sobol sampler's second dimension, bit-reversed: by the defining loop and by the butterfly the kernels use (csrc/device/drng.h). */
/* a[k] % d[k] the way the index-based samplers compute it (csrc/device/drng.h fastmod_u32: precomputed constant, no division). */
AKR_TEST_API int32_t akr_host_fastmod(uint32_t n, const uint32_t *a, const uint32_t *d, uint32_t *out);

/* Scenes kept as meshes + instances: the conservative reject of a candidate triangle (csrc/device/dinst.h tri_may_hit) next to the exact
 * test it stands in front of, on the host. rays8 = o.xyz d.xyz tmin tlimit, tris9 = world-space A B C; may / exact = 0 or 1 per item. */
AKR_TEST_API int32_t akr_host_tri_pretest(uint32_t n, const float *rays8, const float *tris9, float plane_shift, uint32_t *may, uint32_t *exact,
                                     float *out_t /* or NULL */);

AKR_TEST_API int32_t akr_host_alias_table(const float *weights, uint32_t n, uint32_t *j, float *t, float *pdf);

/* ---------------------------------------------------------------------------------------------------
 * Device-function probes (used by the parity tests to compare single device functions with the oracle;
 * they launch tiny kernels on the context's stream and block).
 * ------------------------------------------------------------------------------------------------- */
/* sin/cos/log of the kernels' elementary functions for n inputs. */
AKR_TEST_API int32_t akr_probe_math(akr_context *ctx, uint32_t n, const float *x, float *sin_out, float *cos_out, float *log_out);

/* The other elementary functions of the arithmetic contract (csrc/device/dmath.h, denv.h, dtex.h) for n pairs xy = (x, y):
 * out6 = exp_f(x), pow_f(x, y), atan2_f(y, x), sqrt_f(x), rcp_f(x), srgb_to_linear1(x). Contract tier. */
AKR_TEST_API int32_t akr_probe_math2(akr_context *ctx, uint32_t n, const float *xy, float *out6);

/* a / b for n pairs: by the pair walk's division without range scaling (csrc/device/dmath.h div_f_unscaled) and by the contract's a / b. */
AKR_TEST_API int32_t akr_probe_div(akr_context *ctx, uint32_t n, const float *a, const float *b, float *out_fast, float *out_ieee);

/* advance(-dim) of n generators (state, inc): by the closed form the kernels use at the end of a pass of the independent sampler
 * (csrc/device/drng.h pcg_end_pass) and by the loop that defines it (pcg_advance), both on the device. */
AKR_TEST_API int32_t akr_probe_pcg_end_pass(akr_context *ctx, uint32_t n, const uint64_t *state, const uint64_t *inc, const uint32_t *dim, uint64_t *out_closed,
                                       uint64_t *out_loop);

/* BSDF of material `m` on a flat surface (normal +z, world == local; cf. akari_test.rs:16-439):
 * mode 0: in = wi (3 floats / item)  -> out = f.rgb, pdf (4 floats / item)
 * mode 1: in = u  (3 floats / item)  -> out = wi.xyz, f.rgb, pdf, valid (8 floats / item) */
AKR_TEST_API int32_t akr_probe_bsdf(akr_context *ctx, const akr_material_desc *m, const float *ggx_table4096, int32_t mode,
                               const float *wo, uint32_t n, const float *in, float *out);

/* Closest hit of n rays (o.xyz, d.xyz, tmin, tmax = 8 floats / ray) -> hit(0/1), inst, prim as u32 and u, v. */
AKR_TEST_API int32_t akr_probe_intersect(akr_context *ctx, akr_scene *scene, uint32_t n, const float *rays, uint32_t *hit_inst_prim,
                                    float *bary);

/* The pair walk of scenes of at most 64 triangles (csrc/device/disect.h trace_pair_exhaustive) as the pt kernel calls it, n lanes:
 * rays16 = o.xyz d.xyz tmax - | so.xyz sd.xyz stmax - (closest-hit ray | shadow ray; tmax < 0: the lane has no such ray),
 * excl3 = excluded global triangle ids ex0 | sex0 sex1 (0xffffffff: none) -> out4 = found, gid, occluded, whether the lane's wave
 * repeated the walk with the contract's division; tuv3 = t, u, v of the closest hit. */
AKR_TEST_API int32_t akr_probe_intersect_pair(akr_context *ctx, akr_scene *scene, uint32_t n, const float *rays16, const uint32_t *excl3, uint32_t *out4,
                                         float *tuv3);

AKR_TEST_API int32_t akr_probe_surface_interaction(akr_context *ctx, akr_scene *scene, uint32_t n, const uint32_t *inst_prim,
                                              const float *bary, float *out);

/* The environment light's sampler on the device (csrc/device/denv.h), for a scene with one:
 *   akr_probe_env_sample  u2 (2 floats / item) -> wi.xyz, pdf, valid (5 floats / item): env_sample
 *   akr_probe_env_pdf     directions (3 floats / item) -> pdf, radiance.rgb (4 floats / item): env_pdf, env_eval */
AKR_TEST_API int32_t akr_probe_env_sample(akr_context *ctx, akr_scene *scene, uint32_t n, const float *u2, float *out5);

AKR_TEST_API int32_t akr_probe_env_pdf(akr_context *ctx, akr_scene *scene, uint32_t n, const float *dirs3, float *out4);

/* Next-event estimation of a scene with punctual lights (csrc/device/dpunct.h; default colour pipeline) for n rows
 * rows7 = p.xyz, n.xyz (the surface point and its geometric normal), u_select: the light the alias table picks and, if it is a punctual one, its sample.
 * out13 = li.rgb, wi.xyz, pdf, ro.xyz, tmax, valid, delta (the last two 0 or 1); light = the index chosen. A choice of an emissive instance or
 * of the environment comes back with pdf = its selection probability and everything else 0.
 *   akr_host_light_sample    the shared text on the host (no GPU; works on a host-only scene)
 *   akr_probe_light_sample   the same through a kernel of one thread per row */
AKR_TEST_API int32_t akr_host_light_sample(const akr_scene *scene, uint32_t n, const float *rows7, float *out13, uint32_t *light);

AKR_TEST_API int32_t akr_probe_light_sample(akr_context *ctx, akr_scene *scene, uint32_t n, const float *rows7, float *out13, uint32_t *light);

/* The same with the two numbers a light with a size draws its point from: rows9 = p.xyz, n.xyz, u_select, u_sample.xy; out13 and
 * light as above. A delta light ignores u_sample; the two hooks above are these with u_sample = (0.5, 0.5). */
AKR_TEST_API int32_t akr_host_light_sample_soft(const akr_scene *scene, uint32_t n, const float *rows9, float *out13, uint32_t *light);

AKR_TEST_API int32_t akr_probe_light_sample_soft(akr_context *ctx, akr_scene *scene, uint32_t n, const float *rows9, float *out13, uint32_t *light);

/* The same over a scene that may have a light tree (csrc/device/dlighttree.h light_tree_probe_row): rows9, out13 and light as above. A row
 * whose entry of the light list is the tree's walks the tree with the number the selection left: out13[6] is then the FULL pdf (the entry's times every
 * level's) and record[i] the index of the record the walk ended at, whose sample the other columns hold; record[i] = 0xFFFFFFFF where the entry was not
 * the tree (the row is then akr_*_light_sample_soft's). The four hooks above keep their outputs on a scene without a tree and sample nothing at the
 * tree's entry of a scene with one. */
AKR_TEST_API int32_t akr_host_light_tree_sample(const akr_scene *scene, uint32_t n, const float *rows9, float *out13, uint32_t *light, uint32_t *record);

AKR_TEST_API int32_t akr_probe_light_tree_sample(akr_context *ctx, akr_scene *scene, uint32_t n, const float *rows9, float *out13, uint32_t *light, uint32_t *record);

/* The camera ray of the scene's camera and lens (csrc/device/dpath.h generate_ray_from / generate_ray_lens_from) for n items:
 * pixels2 = (x, y) as u32, u4 = u_filter.xy, u_lens.xy (u_lens is ignored without a lens), out6 = o.xyz, d.xyz in world space.
 *   akr_host_lens_ray       the shared text on the host (no GPU; works on a host-only scene)
 *   akr_probe_camera_rays   the same on the device */
AKR_TEST_API int32_t akr_host_lens_ray(const akr_scene *scene, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t *pixels2, const float *u4,
                                  float *out6);

AKR_TEST_API int32_t akr_probe_camera_rays(akr_context *ctx, akr_scene *scene, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t *pixels2,
                                      const float *u4, float *out6);

/* Which kernel a pt session of (scene, cfg) would launch and how that launch's LDS is laid out, decided on the host (no GPU; works on a
 * host-only scene): what akr_pt_begin decides, without the session. The options are the process-wide ones a session snapshots when it
 * begins (defer_metal -1 = the library decides, simple_kernels, defer_on); spec_waves = 0: no per-scene kernel, else the per-scene kernel
 * of that many waves per SIMD is taken to have compiled (where the session would ask for one: texture-fed materials, no force_diffuse).
 *   variant[10]     the instantiation: bvh, fd, tex, pmj, stage, defer, simple, inst, env, lens; punct (the struct's last field): the PUNCT kernels
 *   simple_scene .. stage_total, tile_offset .. val_offset_words   the fields of the kernel parameter block of the same names
 *   lds_bytes, blocks   dynamic LDS and workgroups of a launch
 *   specialised     1 = a per-scene kernel; wrapper is then the text that instantiates it (part of the kernel cache's key), else "" */
typedef struct akr_pt_launch_plan {
    uint32_t variant[10];
    uint32_t simple_scene, defer_metal, defer_flags;
    uint32_t stage_bytes[13], stage_total;
    uint32_t tile_offset, bvh_tile_nodes, park_offset, carry_offset, bn_offset, val_offset_words;
    uint32_t lds_bytes, blocks;
    uint32_t specialised;
    char wrapper[600];
    uint32_t punct;
} akr_pt_launch_plan;
AKR_TEST_API int32_t akr_host_pt_launch_plan(akr_scene *scene, const akr_pt_config *cfg, int32_t defer_metal, int32_t simple_kernels, int32_t defer_on,
                                        int32_t spec_waves, akr_pt_launch_plan *out);
/* The same for a session that may collect the denoiser's guides (feat = 1: what akr_pt_begin_features decides; feat = 0: exactly the plan above).
 * wavefront, arith: the values of the options of those names to decide for (not the process's). feat = 1 where akr_pt_begin_features refuses --
 * a kept scene, wavefront = 1, arith = 1 -- fails with AKR_ERR_UNSUPPORTED and that call's message. A feature session gets no per-scene kernel.
 *   plan            as above (variant[] has no entry for feat: it is `feat` here)
 *   kernel_compiled 1 = the variant exists as a precompiled kernel (kernels.h pt_variant_compiled)
 *   park_slots      LDS columns per lane of parked path state in the layout (0: the kernel parks nothing); park_slots_feat: kParkSlotsFeat
 *   required_bytes  the layout's LDS without the blocks that only take what is left; lds_budget: the workgroup's share (pt_lds_budget) */
typedef struct akr_pt_features_plan {
    akr_pt_launch_plan plan;
    uint32_t feat, kernel_compiled, park_slots, park_slots_feat, required_bytes, lds_budget;
} akr_pt_features_plan;
AKR_TEST_API int32_t akr_host_pt_features_plan(akr_scene *scene, const akr_pt_config *cfg, int32_t defer_metal, int32_t simple_kernels, int32_t defer_on,
                                               int32_t spec_waves, int32_t feat, int32_t wavefront, int32_t arith, akr_pt_features_plan *out);

/* Whether pt sessions begun from now on order their work items by measured pixel cost: 0 = never, 1 = where the library's rule says it
 * pays (its behaviour without this hook: the exhaustive intersector without textures and without collected guides), 2 = every megakernel session.
 * Process-wide; *previous (may be NULL) = the mode before the call. Films, sampler states and counters are the same bit for bit in every mode. */
AKR_TEST_API int32_t akr_probe_pt_cost_order_mode(int32_t mode, int32_t *previous);
/* A pt session's work items ordered by measured pixel cost, once everything on its stream has run:
 *   state    0 = the items are dealt by position, 1 = the launches record the cost, 2 = the table is in use
 *   cost     W * H words, or NULL: closest-hit rays of every pixel in the launch that recorded, 0 for pixels the session does not render (the kernel
 *            records by work item; the hook maps items to pixels). Refused for a session that never recorded or renders an active-tile list
 *   table    `capacity` words, or NULL: the item -> pixel table; *n_table = its entries (0 before it exists), a multiple of 256, 0xFFFFFFFF = no pixel
 *   sort_ms  or NULL: what building the table took on the device, by HIP events (0 before it exists) */
AKR_TEST_API int32_t akr_probe_pt_cost_order(akr_pt_session *se, uint32_t *state, uint32_t *cost, uint32_t *table, uint32_t capacity, uint32_t *n_table, float *sort_ms);

/* Row `index` of the table of options behind akr_option_set / akr_option_get (host/options.cpp), in the table's order; AKR_ERR_INVALID_ARGUMENT
 * past its last row. name, env: static strings (env = "" for an option without an environment variable); default_value: what the option is when
 * the environment says nothing; ranged = 1: akr_option_set refuses values outside [lo, hi]; 0: it takes any int32 (lo, hi = INT32_MIN, INT32_MAX). */
typedef struct akr_option_info {
    const char *name, *env;
    int32_t default_value, ranged, lo, hi;
} akr_option_info;
AKR_TEST_API int32_t akr_host_option_info(uint32_t index, akr_option_info *out);

/* akr_denoise on the host (no GPU): the text of csrc/device/ddenoise.h compiled for the host, over host arrays. Each film is an accumulator
 * in the reference layout [rgb 3N | splat 3N | weight N] with its splat scale; albedo_film / normal_film may be NULL. out_rgb = 3 N floats,
 * what akr_film_resolve returns for akr_denoise's output film. Same refusals as akr_denoise. */
AKR_TEST_API int32_t akr_host_denoise(const akr_denoise_config *cfg, uint32_t width, uint32_t height, const float *color_film, float color_splat_scale,
                                 const float *albedo_film, float albedo_splat_scale, const float *normal_film, float normal_splat_scale, float *out_rgb);

/* akr_denoise under one level kernel (0 = gathering, 1 = LDS-tiled; -1 = the library's choice per step, what akr_denoise runs) with its parts timed by HIP events on the context's stream:
 * times11 = milliseconds of prepare, level 0 .. 7 (0 beyond cfg->iterations), finish, the whole call (tools/denoise_bench.py). */
AKR_TEST_API int32_t akr_probe_denoise_times(akr_context *ctx, const akr_denoise_config *cfg, akr_film *color, akr_film *albedo, akr_film *normal, akr_film *out,
                                        int32_t kernel, float *times11);

/* akr_denoise_variance on the host and timed: the twins of the two hooks above. half_film = the colour film after a subset of its samples
 * (its splat plane is not read); times11[0] = prepare + prefilter. */
AKR_TEST_API int32_t akr_host_denoise_variance(const akr_denoise_config *cfg, uint32_t width, uint32_t height, const float *color_film, float color_splat_scale,
                                          const float *half_film, const float *albedo_film, float albedo_splat_scale, const float *normal_film,
                                          float normal_splat_scale, float *out_rgb);
AKR_TEST_API int32_t akr_probe_denoise_variance_times(akr_context *ctx, const akr_denoise_config *cfg, akr_film *color, akr_film *half, akr_film *albedo,
                                                 akr_film *normal, akr_film *out, int32_t kernel, float *times11);

/* Adaptive sampling on the host (no GPU): the text of csrc/device/dadapt.h compiled for the host, over host film arrays [rgb 3N | splat 3N | weight N].
 * akr_host_tile_error = akr_film_tile_error; akr_host_half_bracket runs k_half_open (close = 0: half <- half - film) or k_half_close
 * (close = 1: half <- half + film) over the rgb and weight planes of the listed tiles' pixels, in place in half_film. Same refusals. */
AKR_TEST_API int32_t akr_host_tile_error(uint32_t width, uint32_t height, const float *film, const float *half_film, uint32_t tile_w, uint32_t tile_h,
                                    const uint32_t *tiles, uint32_t n, float *err_out);
AKR_TEST_API int32_t akr_host_half_bracket(uint32_t width, uint32_t height, const float *film, float *half_film, uint32_t tile_w, uint32_t tile_h,
                                      const uint32_t *tiles, uint32_t n, int32_t close);
/* The three kernels over the listed tiles, timed by HIP events on the context's stream: times3 = milliseconds of k_tile_error, k_half_open,
 * k_half_close (tools/adaptive_bench.py). half is left as it was up to the rounding of (half - film) + film. */
AKR_TEST_API int32_t akr_probe_adapt_times(akr_context *ctx, akr_film *film, akr_film *half, uint32_t tile_w, uint32_t tile_h, const uint32_t *tiles, uint32_t n,
                                      float *times3);

/* akr_display_transform on the host (no GPU): the text of csrc/device/ddisplay.h compiled for the host, over a host array. film = an accumulator in the
 * reference layout [rgb 3N | splat 3N | weight N] with its splat scale. out_rgb = 3 N floats, what akr_film_resolve returns for akr_display_transform's
 * output film; *exposure_used (may be NULL) = k. Same refusals as akr_display_transform. */
AKR_TEST_API int32_t akr_host_display_transform(const akr_display_config *cfg, uint32_t width, uint32_t height, const float *film, float splat_scale, float *out_rgb,
                                           float *exposure_used);
/* akr_film_luminance_histogram on the host: counts256 and *skipped of a host film. */
AKR_TEST_API int32_t akr_host_luminance_histogram(uint32_t width, uint32_t height, const float *film, float splat_scale, uint32_t *counts256, uint32_t *skipped);
/* akr_display_transform under one blur (0 = gathering passes, 1 = LDS; -1 = the library's choice) with its parts timed by HIP events on the context's stream:
 * times8 = milliseconds of the histogram kernel, the bloom source, all downsamples, all blurs, all upsamples, the apply pass, the whole call (the histogram's read-back included),
 * the blur of level 1 alone (tools/display_bench.py). */
AKR_TEST_API int32_t akr_probe_display_times(akr_context *ctx, const akr_display_config *cfg, akr_film *film, akr_film *out, int32_t kernel, float *times8);

/* SurfaceInteraction of (inst, prim, u, v): out 19 floats / item = p, ng, n, t, s, uv, area, material. */
/* The tables of the pmj02bn sampler as the library uses them: sets = u32[5 * 65536 * 2], bluenoise = u16[48 * 128 * 128]. */
AKR_TEST_API int32_t akr_host_pmj02bn_tables(uint32_t *sets, uint16_t *bluenoise);

/* The PNG reader of akr_scene_load (8/16-bit, all colour types, tRNS, Adam7 interlacing), image crate `to_rgba8` rules
 * (load.rs:583-604). Rows in file order. rgba == NULL: only the size is returned. */
AKR_TEST_API int32_t akr_host_decode_png(const uint8_t *data, uint64_t len, uint32_t *width, uint32_t *height, uint8_t *rgba, uint64_t capacity);

/* The JPEG reader of akr_scene_load (baseline + progressive Huffman, 8 bit, grey / YCbCr / RGB, any integer sampling
 * ratios, restart intervals). Same calling convention as akr_host_decode_png. */
AKR_TEST_API int32_t akr_host_decode_jpeg(const uint8_t *data, uint64_t len, uint32_t *width, uint32_t *height, uint8_t *rgba, uint64_t capacity);

/* The TIFF reader of akr_scene_load (classic TIFF, first image; strips or tiles; chunky 8 / 16-bit or float samples; grey,
 * grey + alpha, RGB, RGBA; none / LZW / deflate / PackBits; horizontal predictor) and the DDS reader (DXT1 / DXT3 / DXT5, top
 * mip level) -- the remaining two encoded formats of load.rs:585-592. Same calling convention as akr_host_decode_png. */
AKR_TEST_API int32_t akr_host_decode_tiff(const uint8_t *data, uint64_t len, uint32_t *width, uint32_t *height, uint8_t *rgba, uint64_t capacity);

AKR_TEST_API int32_t akr_host_decode_dds(const uint8_t *data, uint64_t len, uint32_t *width, uint32_t *height, uint8_t *rgba, uint64_t capacity);

/* The OpenEXR reader of akr_scene_load (single-part scanline; none / RLE / ZIPS / ZIP; half / float / uint channels R G B A
 * or Y), RGBA f32 out, rows in file order. rgba == NULL: only the size is returned. */
AKR_TEST_API int32_t akr_host_decode_exr(const uint8_t *data, uint64_t len, uint32_t *width, uint32_t *height, float *rgba, uint64_t capacity_floats);

/* The same on the host under the colour pipeline `color` (akr_color_pipeline_bits): the tables a session with that
 * akr_pt_config.color uses, evaluated by the code the kernels run. */
AKR_TEST_API int32_t akr_probe_material_inputs_host(akr_scene *scene, uint32_t material, uint32_t color, uint32_t n, const float *uv, float *out26);

/* The interpreter's result for `material` at n uv points on the host (default colour pipeline): the folded record (64 words each),
 * optionally the alpha of the base-colour node and emission_color * emission_strength -- the values per-scene code must reproduce. */
AKR_TEST_API int32_t akr_probe_material_folded_host(akr_scene *scene, uint32_t material, uint32_t n, const float *uv, uint32_t *out64, float *alpha, float *emission3);

/* Evaluated inputs of `material` (26 words each = akr_material_desc) at n uv points: shader-graph evaluation + texture
 * sampling on the device, or -- ctx == NULL -- the same code on the host. */
AKR_TEST_API int32_t akr_probe_material_inputs(akr_context *ctx, akr_scene *scene, uint32_t material, uint32_t n, const float *uv, float *out26);

#ifdef __cplusplus
}
#endif

#endif /* AKARI_HIP_TEST_H */
