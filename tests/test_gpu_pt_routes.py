"""What kind of session akr_pt_begin / akr_pt_begin_features make of (scene, config, options) -- which schedule, which arithmetic tier, a per-scene
kernel or not, the status text, or the refusal -- held to tests/golden/pt_session_routes.json: what the library answered, on the MI355X, before those
decisions were gathered into pt_route (host/pt_plan.cpp). A row begins one session of a 32 x 32 frame at 4 spp under its options,
reads akr_pt_kernel_info (or the error code and message) and ends the session: no pass is launched. `record()` below wrote the table; it is not a test."""
import json
import os

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import launch_plan_matrix as M
from tests import punct_parity_cases as P
from tests.helpers import instanced_scene, make_config, textured_room

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pt_session_routes.json")
FLAT = dict(force_bvh=0, instancing=0, light_tree=0)
KEPT = dict(force_bvh=0, instancing=1, light_tree=0)
POINT = abi.PunctualLightData(abi.LIGHT_POINT, position=(0.1, 0.2, 0.3), color=(3.0, 2.5, 2.0), strength=3.0)
OPTIONS = ("wavefront", "arith", "specialise", "wf_sort", "sched_trial")  # a row's process options; force_diffuse is of its config, guides of the call
VALUES = dict(wavefront=(-1, 0, 1), arith=(0, 1), specialise=(0, 1), wf_sort=(0, 1), sched_trial=(0, 1), force_diffuse=(0, 1), guides=(0, 1))


def _with(sd, **fields):
    for k, v in fields.items():
        setattr(sd, k, v)
    return sd


# name -> (maker, the options the scene is created under)
SCENES = {
    "cbox": (M.cbox, FLAT),
    "cbox_tree": (M.cbox, dict(FLAT, force_bvh=1)),
    "tex": (lambda: textured_room(32, 32), FLAT),
    "kept2": (lambda: instanced_scene(n_inst=2, n=4, width=32, height=32), KEPT),
    "kept2_tex": (lambda: instanced_scene(n_inst=2, n=4, width=32, height=32, textured=True), KEPT),
    "cbox_env": (lambda: _with(M.cbox(), environment=M.ENV), FLAT),
    "cbox_lens": (lambda: _with(M.camera_inside(M.cbox()), lens=M.LENS), FLAT),
    "cbox_point": (lambda: _with(M.cbox(), lights=[POINT]), FLAT),
    "cbox_tree3": (lambda: _with(M.cbox(), lights=P.grid_lights(3)), dict(FLAT, light_tree=1)),
    # (not one of the eight kinds of scene a route distinguishes, but the only way to the status of a textured scene with punctual lights)
    "tex_point": (lambda: P.tex_scene(32, 32, P.ROOM_LIGHTS), FLAT),
}
# (wavefront, arith, specialise, wf_sort, sched_trial, force_diffuse, guides): every scene meets every tuple, so every value of every option. Of the
# four with specialise = 1 only the last leaves a textured scene its per-scene kernel: two rows of the table compile one (tex, kept2_tex).
TUPLES = [
    (-1, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0),
    (-1, 1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 1, 0, 0), (1, 1, 0, 1, 0, 0, 0),
    (-1, 0, 0, 1, 0, 0, 0), (1, 0, 0, 1, 1, 0, 0), (-1, 0, 0, 0, 1, 0, 0), (-1, 0, 0, 0, 0, 1, 0),
    (-1, 0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 1, 1), (1, 0, 0, 0, 0, 0, 1), (-1, 1, 0, 0, 0, 0, 1),
    (-1, 0, 1, 0, 0, 1, 0), (0, 0, 1, 0, 1, 0, 1), (1, 1, 1, 1, 1, 1, 0), (-1, 0, 1, 0, 0, 0, 0),
]
# two faults in one call: which one is reported (`fault` is the second, made by the call itself)
DOUBLE_FAULTS = [
    dict(scene="cbox_point", wavefront=1, fault="spp_per_pass_0"),
    dict(scene="cbox_env", arith=1, fault="film_size"),
    dict(scene="kept2", arith=1, guides=1, fault=""),
    dict(scene="cbox", wavefront=1, guides=1, fault="albedo_is_film"),
]


def requests():
    """the rows to ask, without their answers"""
    names = OPTIONS + ("force_diffuse", "guides")
    rows = [dict(zip(names, t), scene=s, fault="", double_fault=0) for s in SCENES for t in TUPLES]
    rows += [{**dict(zip(names, TUPLES[0])), **d, "double_fault": 1} for d in DOUBLE_FAULTS]
    return rows


def answer(ctx, scene, row):
    """{"code", "message"} of a refused begin, or {"status", "kernel_flags", "specialised", "min_waves", "per_scene"} of the session"""
    cfg = make_config(spp=4, spp_per_pass=0 if row["fault"] == "spp_per_pass_0" else 4, max_depth=6, force_diffuse=row["force_diffuse"])
    size = 16 if row["fault"] == "film_size" else 32
    film = capi.Film(ctx, size, size)
    albedo = normal = None
    if row["guides"]:
        albedo, normal = film if row["fault"] == "albedo_is_film" else capi.Film(ctx, 32, 32), capi.Film(ctx, 32, 32)
    with capi.options(**{k: row[k] for k in OPTIONS}):
        try:
            se = capi.PtSession(ctx, scene, cfg, film, albedo, normal)
        except capi.AkariError as e:
            return dict(code=e.code, message=capi.last_error())
        info = se.kernel_info()
        se.end()
    # (min_waves is reported by the sessions that asked for a per-scene kernel, whether or not it compiled)
    return dict(status=info["status"], kernel_flags=info["kernel_flags"], specialised=info["specialised"], min_waves=info["min_waves"], per_scene=int(info["min_waves"] != 0))


def answers(ctx, rows):
    out, scenes = [], {}
    for row in rows:
        if row["scene"] not in scenes:
            make, opts = SCENES[row["scene"]]
            sd = make()
            if sd.ggx_table is None:
                sd.ggx_table = np.fromfile(os.path.join(os.path.dirname(GOLDEN), "ggx_dielectric_s.f32"), dtype=np.float32)
            with capi.options(**opts):
                scenes[row["scene"]] = capi.Scene(ctx, sd)
        out.append(answer(ctx, scenes[row["scene"]], row))
    for s in scenes.values():
        s.close()
    return out


def record(path=GOLDEN):
    """writes the table: run on the library the table is to pin"""
    rows = requests()
    got = answers(capi.Context(0), rows)
    with open(path, "w") as f:
        json.dump(dict(rows=[dict(ask=r, got=g) for r, g in zip(rows, got)]), f, indent=0, sort_keys=True)
        f.write("\n")
    return len(rows)


@pytest.fixture(scope="module")
def table():
    return json.load(open(GOLDEN))["rows"]


def test_every_route_is_the_recorded_one(ctx, table):
    got = answers(ctx, [r["ask"] for r in table])
    bad = []
    for r, g in zip(table, got):
        want = dict(r["got"])
        if want.get("per_scene") and g.get("per_scene"):  # that text says whether the disk cache was hit
            want.pop("status"), g.pop("status")
        if g != want:
            bad.append(f"{r['ask']}:\n    got      {g}\n    recorded {want}")
    assert not bad, f"{len(bad)} of {len(table)} rows differ:\n" + "\n".join(bad[:20])


# a status begins with / a refusal contains
ARMS = {
    "relaxed": "relaxed arithmetic tier: precompiled kernels",
    "wavefront": "wavefront schedule",
    "guides, option ignored": "guides are collected by the interpreter kernels: no per-scene kernel",
    "guides": "guides are collected by the precompiled kernels",
    "no textures": "the scene has no texture-fed material",
    "punctual": "punctual lights are sampled by the interpreter kernels: no per-scene kernel",
    "specialise = 0": "option specialise = 0",
    "force_diffuse": "force_diffuse kernels evaluate no surface graphs",
}
REFUSALS = {
    "punctual, wavefront": "and the wavefront schedule is forced (option wavefront = 1); only the megakernel samples punctual lights",
    "punctual, relaxed": "has no kernels that sample punctual lights",
    "guides, kept": "akr_pt_begin_features: the scene is kept as meshes + instances",
    "guides, wavefront": "akr_pt_begin_features: the wavefront schedule is forced",
    "guides, relaxed": "akr_pt_begin_features: the relaxed arithmetic tier",
    "guides, punctual": "the kernels that sample punctual lights collect no guides",
    "relaxed, environment": "does not render scenes with an environment light",
    "relaxed, lens": "does not render through a lens",
}


def test_the_table_covers_what_it_is_there_for(table):
    """from the table alone: its size, every option value on every scene, the nine arms of the status, both cost-order states a session can be in
    before its first pass, the eight refusals, the four double faults, and no more than two compiles"""
    assert len(table) <= 200
    plain = [r for r in table if not r["ask"]["double_fault"]]
    for s in SCENES:
        for k, vals in VALUES.items():
            assert {r["ask"][k] for r in plain if r["ask"]["scene"] == s} == set(vals), (s, k)
    assert all(r["ask"]["specialise"] in (0, 1) for r in table)
    status = [r["got"]["status"] for r in table if "status" in r["got"] and not r["got"]["per_scene"]]
    for arm, text in ARMS.items():
        assert any(s.startswith(text) for s in status), arm
    compiled = [r for r in table if r["got"].get("per_scene")]
    assert 1 <= len(compiled) <= 2 and all(r["got"]["specialised"] == 1 and r["got"]["min_waves"] == 3 for r in compiled)  # the ninth arm
    assert any(s.endswith("; cost order: recording") for s in status) and any("cost order" not in s for s in status)
    assert not any("cost order: in use" in s for s in status)  # (that needs a pass)
    refused = [r["got"] for r in table if "code" in r["got"]]
    for name, text in REFUSALS.items():
        assert any(g["code"] == capi.ERR_UNSUPPORTED and text in g["message"] for g in refused), name
    double = [r for r in table if r["ask"]["double_fault"]]
    assert [{k: r["ask"][k] for k in d} for r, d in zip(double, DOUBLE_FAULTS)] == DOUBLE_FAULTS and all("code" in r["got"] for r in double)
