"""Procedural shader nodes on the host: CONST4, MATH and NOISE against the numpy restatement of tests/procedural_model.py,
bit for bit; properties that restate nothing; constant folding; the any-hit test's opacity proof; refusals; the scene-file reader."""
import base64
import json

import numpy as np
import pytest

from akari_render_amd import abi, capi
from tests import procedural_cases as PC
from tests import procedural_model as M
from tests.helpers import box_scene, make_config, n_bit_diff, textured_room

F = np.float32
N = abi.NodeData


@pytest.fixture(scope="module")
def probe(hip_lib):
    sd, index, cases = PC.probe_scene()
    scene = capi.Scene(None, sd)
    return scene, index, cases, PC.probe_points(), PC.host_pow(scene, index["pow"])


def _mismatch(got, want):
    bad = ~M.bits_equal(got, want)
    return int(np.count_nonzero(bad)), (got[bad][:4], want[bad][:4])


# ---------------------------------------------------------------------------------------------- model against host
@pytest.mark.parametrize("case", PC.math_cases(), ids=lambda c: "%s-b%d-%s" % (M.MATH_NAMES[c[0]], c[1], c[2]))
def test_math_node_host_equals_model(probe, case):
    scene, index, _, uv, pow_fn = probe
    name = "math-%s-b%d-%s" % (M.MATH_NAMES[case[0]], case[1], case[2])
    got = capi.probe_material_inputs_host(scene, index[name], uv)[:, 1:5]  # base colour and its alpha: x y z w of the node
    n_bad, first = _mismatch(got, PC.math_expected(case, uv, pow_fn))
    assert n_bad == 0, first


def test_math_cases_cover_both_alphas(probe):
    """w = 0 and w = 1 both reach the output, and the scalar cases have w = 0: the cases above check the w rule on both."""
    _, _, _, uv, _ = probe
    ws = {(c[1], c[2]): float(PC.math_expected((0,) + c[1:], uv, None)[0, 3]) for c in PC.math_cases()}
    assert ws[(0, "V,C1")] == 0.0 and ws[(1, "V,C1")] == 1.0 and ws[(0, "C1,V")] == 1.0 and ws[(1, "C1,V")] == 0.0 and ws[(3, "C1,V")] == 0.0


@pytest.mark.parametrize("case", PC.NOISE_CASES, ids=lambda c: "d%d-%s-s%g" % (c[0], "vec" if c[1] else "uv", c[2]))
def test_noise_node_host_equals_model(probe, case):
    scene, index, _, uv, _ = probe
    name = "noise-d%d-%s-s%g" % (case[0], "vec" if case[1] else "uv", case[2])
    got = capi.probe_material_inputs_host(scene, index[name], uv)[:, 1:5]
    want = PC.noise_expected(case, uv)
    n_bad, first = _mismatch(got, want)
    assert n_bad == 0, first
    assert np.count_nonzero(want[:, 0]) > 128 and np.abs(want[:200, 0]).max() > 0.25  # (the comparison is not one of zeros)


def test_fbm_of_four_octaves_is_accepted_and_equals_model(probe):
    scene, index, _, uv, _ = probe
    got = capi.probe_material_inputs_host(scene, index["fbm"], uv)[:, 6]
    assert np.all(M.bits_equal(got, PC.fbm_expected(uv)))


# ---------------------------------------------------------------------------------------------- properties that restate nothing
def _noise_scene(dim):
    sd = box_scene()
    sd.materials[0].graph = abi.GraphData([N(abi.NODE_CONST, (), (1.0, 0, 0)), abi.noise(0, abi.NODE_NONE, dim)], {"base_color": 1})
    return capi.Scene(None, sd)


@pytest.mark.parametrize("dim", [1, 2])
def test_noise_is_zero_on_the_lattice(hip_lib, dim):
    uv = np.array([[i, j] for j in range(-7, 9) for i in range(-7, 9)], dtype=F)
    n = capi.probe_material_inputs_host(_noise_scene(dim), 0, uv)[:, 1]
    assert np.all((n.view(np.uint32) & 0x7FFFFFFF) == 0)  # +0 or -0


@pytest.mark.parametrize("dim,axis", [(1, 0), (2, 0), (2, 1)])
def test_noise_is_continuous_across_lattice_lines(hip_lib, dim, axis):
    """One ulp below and one ulp above a lattice line the values come from two cells (other hashes for the far corners, the shared corners at the
    other end of the lerp): they agree to within the slope bound of the model times the distance."""
    rng = np.random.default_rng(5 + dim + axis)
    ks = np.repeat(np.arange(-8, 8, dtype=F), 8)
    lo, hi = np.nextafter(ks, F(-np.inf)), np.nextafter(ks, F(np.inf))
    other = rng.uniform(-8, 8, size=ks.shape).astype(F)
    pts = lambda c: np.stack([c, other] if axis == 0 else [other, c], axis=1)  # noqa: E731
    scene = _noise_scene(dim)
    a = capi.probe_material_inputs_host(scene, 0, pts(lo))[:, 1].astype(np.float64)
    b = capi.probe_material_inputs_host(scene, 0, pts(hi))[:, 1].astype(np.float64)
    L, slack = M.slope_bound(dim)
    bound = L * (hi.astype(np.float64) - lo.astype(np.float64)) + slack
    assert np.all(np.abs(a - b) <= bound), float(np.max(np.abs(a - b) - bound))
    if dim == 2:
        assert np.abs(a).max() > 0.5  # (on a lattice line of the plane the function is not zero: values of two cells were compared)


@pytest.mark.parametrize("op", [abi.MATH_MIN, abi.MATH_MAX])
def test_min_max_of_a_value_with_itself(probe, op):
    _, _, _, uv, _ = probe
    sd = box_scene()
    nodes = PC._operand_nodes()
    sd.materials[0].graph = abi.GraphData(nodes + [abi.math(op, 3, 3, 0)], {"base_color": 8})
    sd.materials.append(abi.MaterialData(graph=abi.GraphData(list(nodes), {"base_color": 3})))
    scene = capi.Scene(None, sd)
    assert n_bit_diff(capi.probe_material_inputs_host(scene, 0, uv)[:, 1:5], capi.probe_material_inputs_host(scene, 1, uv)[:, 1:5]) == 0


# ---------------------------------------------------------------------------------------------- folding
def test_constant_math_chains_fold(hip_lib):
    """A math chain over constants leaves no graph: the material, its folded record and the launch plan are those of the folded constants."""
    chain = abi.GraphData([
        N(abi.NODE_CONST, (), (0.2, 0.4, 0.6)), abi.const4(0.5, 0.25, 2.0, 1.0), abi.math(abi.MATH_MUL, 1, 0, 0),      # 2 = (0.1, 0.1, 1.2, 1)
        N(abi.NODE_CONST, (), (0.125, 0, 0)), abi.math(abi.MATH_ADD, 2, 3, 2), abi.math(abi.MATH_MIN, 4, 1, 0),        # 4 = + 0.125, 5 = min with node 1
        N(abi.NODE_CONST, (), (0.3, 0, 0)), N(abi.NODE_CONST, (), (2.0, 0, 0)), abi.math(abi.MATH_DIV, 6, 7, 3), abi.math(abi.MATH_SUB, 8, 3, 3),  # 9 = 0.3 / 2 - 0.125
    ], {"base_color": 5, "roughness": 9})
    k = lambda *v: np.array([v + (0.0,) * (4 - len(v))], dtype=F)  # noqa: E731
    c4 = np.array([[0.5, 0.25, 2.0, 1.0]], dtype=F)
    col = M.math_node(5, M.math_node(0, M.math_node(2, c4, k(0.2, 0.4, 0.6), 0), k(0.125), 2), c4, 0)[0]
    rough = M.math_node(1, M.math_node(3, k(0.3), k(2.0), 3), k(0.125), 3)[0, 0]
    assert col[3] == 1.0
    direct = abi.GraphData([abi.const4(*(float(x) for x in col)), N(abi.NODE_CONST, (), (float(rough), 0, 0))], {"base_color": 0, "roughness": 1})
    scenes = []
    for g in (chain, direct):
        sd = box_scene()
        sd.materials[0].graph = g
        scenes.append(capi.Scene(None, sd))
    cfg = make_config(spp=4)
    plans = [s.launch_plan(cfg) for s in scenes]
    assert plans[0]["variant"]["tex"] == 0 and plans[0] == plans[1]
    uv = np.zeros((1, 2), dtype=F)
    a, b = (capi.probe_material_inputs_host(s, 0, uv) for s in scenes)
    assert n_bit_diff(a, b) == 0 and n_bit_diff(a[0, 1:5], col) == 0 and a[0, 6] == rough
    ma, mb = (s.array(capi.ARRAY_MATERIALS, np.uint32) for s in scenes)
    assert np.array_equal(ma, mb)


# ---------------------------------------------------------------------------------------------- opacity
def _flags(sd):
    mats = capi.Scene(None, sd).array(capi.ARRAY_MATERIALS, np.uint32).reshape(-1, 64)
    return [(int(f) >> 8) & 3 for f in mats[:, 1]]  # bit 0: MF_TEXTURED, bit 1: MF_ALPHA_TEXTURED (as tests/test_textures.py reads them)


def test_math_and_noise_in_the_opacity_proof(hip_lib):
    def wall(graph, cutout=False):
        sd = textured_room(alpha_cutout=cutout)
        sd.materials[1].graph = graph
        return _flags(sd)[1]

    tint = N(abi.NODE_RGB, (), (0.9, 0.5, 0.4))
    image = [N(abi.NODE_IMAGE, (0, abi.NODE_NONE, 1)), tint]
    assert wall(abi.GraphData(image + [abi.math(abi.MATH_MUL, 0, 1, 0)], {"base_color": 2})) == 1               # opaque image x rgb: provably opaque
    assert wall(abi.GraphData(image + [abi.math(abi.MATH_MUL, 0, 1, 0)], {"base_color": 2}), cutout=True) == 3  # transparent texels: not
    assert wall(abi.GraphData(image + [abi.math(abi.MATH_MUL, 1, 0, 0)], {"base_color": 2}), cutout=True) == 1  # w comes from the rgb operand
    checker = [tint, N(abi.NODE_RGB, (), (0.1, 0.2, 0.3)), N(abi.NODE_CONST, (), (3.0, 0, 0)), N(abi.NODE_CHECKERBOARD, (abi.NODE_NONE, 2, 0, 1))]
    assert wall(abi.GraphData(checker + [abi.math(abi.MATH_MUL, 3, 0, 0)], {"base_color": 4})) == 1             # mul(rgb, rgb), varying
    scalar = [N(abi.NODE_CONST, (), (2.0, 0, 0)), abi.noise(0)]
    assert wall(abi.GraphData(scalar, {"base_color": 1})) == 3                                                  # noise has w = 0
    assert wall(abi.GraphData(scalar + [tint, abi.math(abi.MATH_MUL, 1, 2, 1)], {"base_color": 3})) == 1        # scalar x rgb: the rgb's w
    assert wall(abi.GraphData(scalar + [abi.const4(0.5, 0.5, 0.5, 0.75), abi.math(abi.MATH_MUL, 1, 2, 1)], {"base_color": 3})) == 3
    assert wall(abi.GraphData(scalar + [abi.const4(0.5, 0.5, 0.5, 1.0), abi.math(abi.MATH_MUL, 1, 2, 1)], {"base_color": 3})) == 1


# ---------------------------------------------------------------------------------------------- refusals
def _refused(graph):
    sd = box_scene()
    sd.materials[0].graph = graph
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, sd)
    return e.value.code, str(e.value)


def test_refusals(hip_lib):
    one = N(abi.NODE_CONST, (), (1.0, 0, 0))
    code, msg = _refused(abi.GraphData([one, abi.noise(0, abi.NODE_NONE, 3)], {"base_color": 1}))
    assert code == capi.ERR_UNSUPPORTED and "dimension 3" in msg
    code, msg = _refused(abi.GraphData([one, abi.noise(0, abi.NODE_NONE, 0)], {"base_color": 1}))
    assert code == capi.ERR_INVALID_ARGUMENT and "dimension" in msg
    code, msg = _refused(abi.GraphData([one, N(abi.NODE_TEXCOORDS), abi.math(7, 0, 1)], {"base_color": 2}))
    assert code == capi.ERR_INVALID_ARGUMENT and "unknown math op" in msg
    code, msg = _refused(abi.GraphData([one, N(abi.NODE_TEXCOORDS), abi.math(abi.MATH_ADD, 0, 1, 4)], {"base_color": 2}))
    assert code == capi.ERR_INVALID_ARGUMENT and "broadcast" in msg
    code, msg = _refused(abi.GraphData([one, abi.math(abi.MATH_ADD, 0, abi.NODE_NONE)], {"base_color": 1}))
    assert code == capi.ERR_INVALID_ARGUMENT and "math needs" in msg
    code, msg = _refused(abi.GraphData([N(abi.NODE_TEXCOORDS), abi.noise(abi.NODE_NONE, 0)], {"base_color": 1}))
    assert code == capi.ERR_INVALID_ARGUMENT and "noise needs scale" in msg
    code, msg = _refused(abi.GraphData([N(abi.NODE_TEXCOORDS), abi.math(abi.MATH_ADD, 0, 2), one], {"base_color": 1}))
    assert code == capi.ERR_INVALID_ARGUMENT and "earlier nodes" in msg
    code, msg = _refused(abi.GraphData([one, abi.noise(2), one], {"base_color": 1}))
    assert code == capi.ERR_INVALID_ARGUMENT and "earlier nodes" in msg
    # nine values alive at once: si.uv and eight sums of it are all still to be read when the ninth is computed
    nodes = [N(abi.NODE_TEXCOORDS)] + [abi.math(abi.MATH_ADD, 0, 0) for _ in range(9)]
    acc = 1
    for i in range(2, 10):
        nodes.append(abi.math(abi.MATH_ADD, acc, i))
        acc = len(nodes) - 1
    code, msg = _refused(abi.GraphData(nodes, {"base_color": acc}))
    assert code == capi.ERR_INVALID_ARGUMENT and "unsupported" in msg and "values alive" in msg  # (the refusal every graph gets, as it was)


# ---------------------------------------------------------------------------------------------- reader
def _scene_file(tmp_path, extra_nodes, **inputs):
    """One quad with uvs in the scene-graph format, its principled material's `inputs` fed by `extra_nodes`."""
    verts = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=F)
    idx = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    uvs = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], dtype=F)
    blob = verts.tobytes() + idx.tobytes() + uvs.tobytes() + np.zeros(1, np.uint32).tobytes()
    o1, o2, o3 = verts.nbytes, verts.nbytes + idx.nbytes, verts.nbytes + idx.nbytes + uvs.nbytes
    view = lambda o, ln: {"buffer": {"id": "b"}, "offset": o, "length": ln}  # noqa: E731
    f = lambda v: {"type": "float", "value": v}  # noqa: E731
    rgb = lambda name, v: {"rgb_" + name: {"type": "rgb", "value": v, "colorspace": "srgb"}, "c_" + name: {"type": "spectral_uplift", "rgb": {"id": "rgb_" + name}}}  # noqa: E731
    nodes = {"f0": f(0.0), "f1": f(1.0), "f_half": f(0.5), "f_ior": f(1.45), "n0": {"type": "float3", "value": [0, 0, 0]}}
    for name, v in (("base", [0.8, 0.7, 0.6]), ("white", [1, 1, 1]), ("black", [0, 0, 0])):
        nodes.update(rgb(name, v))
    nodes.update(extra_nodes)
    bsdf = {"base_color": "c_base", "metallic": "f0", "roughness": "f_half", "ior": "f_ior", "alpha": "f1", "normal": "n0",
            "subsurface_weight": "f0", "subsurface_radius": "n0", "subsurface_scale": "f0", "subsurface_ior": "f_ior",
            "subsurface_anisotropy": "f0", "specular_ior_level": "f_half", "specular_tint": "c_white", "anisotropic": "f0",
            "anisotropic_rotation": "f0", "tangent": "n0", "transmission_weight": "f0", "sheen_weight": "f0", "sheen_tint": "c_white",
            "coat_weight": "f0", "coat_roughness": "f0", "coat_ior": "f_ior", "coat_tint": "c_white", "coat_normal": "n0",
            "emission_color": "c_black", "emission_strength": "f0"}
    bsdf.update(inputs)
    nodes["bsdf"] = dict({"type": "principled"}, **{k: {"id": v} for k, v in bsdf.items()})
    nodes["out"] = {"type": "output", "node": {"id": "bsdf"}}
    trs = lambda t: {"type": "trs", "data": {"translation": t, "rotation": [0, 0, 0], "scale": [1, 1, 1], "coordinate_system": "Akari"}}  # noqa: E731
    scene = {
        "camera": {"type": "perspective", "data": {"transform": trs([0, 1, 3]), "fov": 50.0, "focal_distance": 1.0, "fstop": 2.8, "sensor_width": 40, "sensor_height": 30}},
        "instances": {"a": {"geometry": {"id": "g"}, "transform": trs([0, 0, 0]), "materials": [{"id": "m"}]}},
        "geometries": {"g": {"type": "mesh", "vertices": {"id": "v_pos"}, "indices": {"id": "v_idx"}, "uvs": {"id": "v_uv"}, "materials": {"id": "v_slot"}}},
        "materials": {"m": {"shader": {"kind": "surface", "nodes": nodes, "output": {"id": "out"}}}},
        "lights": {}, "images": {},
        "buffers": {"b": {"type": "base64", "data": base64.b64encode(blob).decode(), "length": len(blob)}},
        "buffer_views": {"v_pos": view(0, o1), "v_idx": view(o1, idx.nbytes), "v_uv": view(o2, uvs.nbytes), "v_slot": view(o3, 4)},
    }
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(scene))
    return str(path)


def test_reader_reads_float4_math_and_noise(hip_lib, tmp_path):
    """The file's graph uses every math op; its probed inputs equal those of the same graph given through the ABI with the broadcast bits the
    static types imply: scalar x scalar (3), vector x scalar (2), scalar x vector (1), vector x vector (0)."""
    ref = lambda i: {"id": i}  # noqa: E731
    m = lambda op, a, b: {"type": "math", "op": op, "first": ref(a), "second": ref(b)}  # noqa: E731
    file_nodes = {
        "tc": {"type": "texcoords"}, "uv": {"type": "extract", "node": ref("tc"), "field": "UV"},
        "s3": {"type": "float", "value": 3.0}, "half": {"type": "float", "value": 0.5}, "lo": {"type": "float", "value": 0.1}, "hi": {"type": "float", "value": 0.9},
        "k4": {"type": "float4", "value": [0.75, 0.5, 0.25, 1.0]}, "k3": {"type": "float3", "value": [0.2, 0.3, 0.4]}, "two": {"type": "float", "value": 2.0},
        "n2": {"type": "noise", "dim": 2, "scale": ref("s3")}, "n1": {"type": "noise", "dim": 1, "scale": ref("s3"), "vector": ref("uv")},
        "t0": m("mul", "n2", "half"), "t1": m("add", "t0", "half"), "t2": m("max", "t1", "lo"), "t3": m("min", "t2", "hi"),   # scalars: 3
        "p": m("pow", "t3", "two"),                                                                                               # 3
        "c0": m("mul", "k4", "p"),                                                                                                # vector x scalar: 2
        "c1": m("sub", "c0", "k3"),                                                                                               # vector x vector: 0
        "c2": m("div", "half", "c1"),                                                                                             # scalar x vector: 1
        "red": {"type": "extract", "node": ref("tc"), "field": "Red"}, "r0": m("add", "red", "n1"), "r1": m("mul", "uv", "r0"),  # 3, then vector x scalar: 2
    }
    path = _scene_file(tmp_path, file_nodes, base_color="c2", roughness="t3", metallic="r0", emission_color="r1")
    loaded = capi.Scene(None, path)
    g = abi.GraphData([
        N(abi.NODE_CONST, (), (3.0, 0, 0)), abi.noise(0, abi.NODE_NONE, 2), N(abi.NODE_CONST, (), (0.5, 0, 0)),                         # 0 s3, 1 n2, 2 half
        abi.math(abi.MATH_MUL, 1, 2, 3), abi.math(abi.MATH_ADD, 3, 2, 3),                                                               # 3 t0, 4 t1
        N(abi.NODE_CONST, (), (0.1, 0, 0)), abi.math(abi.MATH_MAX, 4, 5, 3), N(abi.NODE_CONST, (), (0.9, 0, 0)), abi.math(abi.MATH_MIN, 6, 7, 3),  # 5 lo, 6 t2, 7 hi, 8 t3
        N(abi.NODE_CONST, (), (2.0, 0, 0)), abi.math(abi.MATH_POW, 8, 9, 3),                                                            # 9 two, 10 p
        abi.const4(0.75, 0.5, 0.25, 1.0), abi.math(abi.MATH_MUL, 11, 10, 2),                                                            # 11 k4, 12 c0
        N(abi.NODE_CONST, (), (0.2, 0.3, 0.4)), abi.math(abi.MATH_SUB, 12, 13, 0), abi.math(abi.MATH_DIV, 2, 14, 1),                    # 13 k3, 14 c1, 15 c2
        N(abi.NODE_TEXCOORDS), N(abi.NODE_EXTRACT, (16, abi.FIELD_RED)), N(abi.NODE_EXTRACT, (16, abi.FIELD_UV)), abi.noise(0, 18, 1),  # 16 tc, 17 red, 18 uv, 19 n1
        abi.math(abi.MATH_ADD, 17, 19, 3), abi.math(abi.MATH_MUL, 18, 20, 2),                                                           # 20 r0, 21 r1
    ], {"base_color": 15, "roughness": 8, "metallic": 20, "emission_color": 21})
    sd = loaded.to_scene_data()
    got_ops = sorted((n.op, n.args[2], n.args[3]) for n in sd.materials[0].graph.nodes if n.op == abi.NODE_MATH)
    assert got_ops == sorted((n.op, n.args[2], n.args[3]) for n in g.nodes if n.op == abi.NODE_MATH)  # every op, the derived broadcast bits
    sd.materials[0].graph = g
    by_abi = capi.Scene(None, sd)
    uv = PC.probe_points()
    a, b = capi.probe_material_inputs_host(loaded, 0, uv), capi.probe_material_inputs_host(by_abi, 0, uv)
    assert np.all(M.bits_equal(a, b))
    assert len(np.unique(a[:, 1])) > 100 and len(np.unique(a[:, 19])) > 100  # (varying values, not a folded constant)


def test_reader_still_refuses_closure_nodes_and_noise_of_dimension_3(hip_lib, tmp_path):
    ref = lambda i: {"id": i}  # noqa: E731
    path = _scene_file(tmp_path, {"s": {"type": "float", "value": 2.0}, "n": {"type": "noise", "dim": 3, "scale": ref("s")}}, roughness="n")
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, path)
    assert e.value.code == capi.ERR_UNSUPPORTED and "dimension 3" in str(e.value)
    path = _scene_file(tmp_path, {"a": {"type": "float", "value": 2.0}, "x": {"type": "math", "op": "mod", "first": ref("a"), "second": ref("a")}}, roughness="x")
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, path)
    assert e.value.code == capi.ERR_UNSUPPORTED and "'mod'" in str(e.value)
    scene = json.loads(open(_scene_file(tmp_path, {})).read())
    nodes = scene["materials"]["m"]["shader"]["nodes"]
    nodes["bsdf2"] = dict(nodes["bsdf"])
    nodes["mixed"] = {"type": "mix", "first": ref("bsdf"), "second": ref("bsdf2"), "factor": ref("f_half")}
    nodes["out"]["node"] = ref("mixed")
    bad = tmp_path / "mix.json"
    bad.write_text(json.dumps(scene))
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, str(bad))
    assert e.value.code == capi.ERR_UNSUPPORTED and "mix" in str(e.value)


def test_reader_decides_a_nodes_static_type_once(hip_lib, tmp_path):
    """x_i = add(x_{i-1}, x_{i-1}), 48 deep: 2^48 visits if the static type were derived afresh for every operand. A math node that is its own
    operand is refused, not followed."""
    ref = lambda i: {"id": i}  # noqa: E731
    nodes = {"s": {"type": "float", "value": 3.0}, "x0": {"type": "noise", "dim": 1, "scale": ref("s")}, "q": {"type": "float", "value": 0.5}}
    for i in range(1, 49):
        nodes["y%d" % i] = {"type": "math", "op": "add", "first": ref("x%d" % (i - 1)), "second": ref("x%d" % (i - 1))}
        nodes["x%d" % i] = {"type": "math", "op": "mul", "first": ref("y%d" % i), "second": ref("q")}
    loaded = capi.Scene(None, _scene_file(tmp_path, nodes, roughness="x48"))
    graph = loaded.to_scene_data().materials[0].graph
    assert all(n.args[3] == 3 for n in graph.nodes if n.op == abi.NODE_MATH) and sum(n.op == abi.NODE_MATH for n in graph.nodes) == 96
    uv = PC.probe_points()
    want = M.noise_node(uv, 3.0, 1)[:, 0]  # (x + x) * 0.5 is exact
    assert np.all(M.bits_equal(capi.probe_material_inputs_host(loaded, 0, uv)[:, 6], want))
    loop = {"a": {"type": "float", "value": 1.0}, "x": {"type": "math", "op": "add", "first": ref("x"), "second": ref("a")}}
    with pytest.raises(capi.AkariError) as e:
        capi.Scene(None, _scene_file(tmp_path, loop, roughness="x"))
    assert "its own operand" in str(e.value)
