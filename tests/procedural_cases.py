"""Scenes, graphs and probe points of tests/test_procedural.py and tests/test_gpu_procedural.py, with what
tests/procedural_model.py says each graph evaluates to. Not a test module."""
import numpy as np

from akari_render_amd import abi, capi
from tests import procedural_model as M
from tests.helpers import textured_room

F = np.float32
N = abi.NodeData

# the operands of the math cases: two varying vectors (w = 0) built from si.uv by a point mapping, one constant with w = 1
V_LOC, V_SC = (0.25, -0.5, 0.75), (1.5, -2.0, 1.0)
V2_LOC, V2_SC = (-0.3, 0.6, 0.5), (0.5, 0.75, 1.0)
C1 = (0.5, 2.0, -1.5, 1.0)
PAIRS = ("V,C1", "C1,V", "V,V2")
NOISE_CASES = [(dim, vec, scale) for dim in (1, 2) for vec in (False, True) for scale in (1.0, 2.5)]


def probe_points():
    """256 uv points: random ones of [-4, 4]^2, the integer lattice of [-2, 2]^2, points one ulp below and above an integer on either axis,
    1e6, and the four sign combinations of zero."""
    rng = np.random.default_rng(418)
    rnd = rng.uniform(-4.0, 4.0, size=(207, 2)).astype(F)
    grid = np.array([[i, j] for j in range(-2, 3) for i in range(-2, 3)], dtype=F)
    ulp = []
    for k in (-1.0, 0.0, 1.0, 2.0):
        lo, hi = np.nextafter(F(k), F(-np.inf)), np.nextafter(F(k), F(np.inf))
        ulp += [[lo, 0.37], [hi, 0.37], [-1.62, lo], [-1.62, hi]]
    big = [[1e6, 0.5], [0.5, 1e6], [1e6, 1e6], [-1e6, 0.3]]
    zero = [[0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]]
    uv = np.concatenate([rnd, grid, np.array(ulp, dtype=F), np.array(big, dtype=F), np.array(zero, dtype=F)]).astype(F)
    assert uv.shape == (256, 2)
    return uv


def _operand_nodes():
    """nodes 0..7: 0 si.uv, 3 V, 6 V2, 7 C1"""
    return [N(abi.NODE_TEXCOORDS), N(abi.NODE_CONST, (), V_LOC), N(abi.NODE_CONST, (), V_SC), N(abi.NODE_MAPPING, (0, 1, 2, abi.MAPPING_POINT)),
            N(abi.NODE_CONST, (), V2_LOC), N(abi.NODE_CONST, (), V2_SC), N(abi.NODE_MAPPING, (0, 4, 5, abi.MAPPING_POINT)), abi.const4(*C1)]


def operand_values(uv):
    t = M.texcoords(uv)
    c1 = np.tile(np.array(C1, dtype=F), (uv.shape[0], 1))
    return {"V": M.mapping_point(t, V_LOC, V_SC), "V2": M.mapping_point(t, V2_LOC, V2_SC), "C1": c1}


def math_cases():
    return [(op, bc, pair) for op in range(7) for bc in range(4) for pair in PAIRS]


def math_graph(op, bc, pair):
    idx = {"V": 3, "V2": 6, "C1": 7}
    a, b = pair.split(",")
    return abi.GraphData(_operand_nodes() + [abi.math(op, idx[a], idx[b], bc)], {"base_color": 8})


def math_expected(case, uv, pow_fn):
    op, bc, pair = case
    vals = operand_values(uv)
    a, b = pair.split(",")
    return M.math_node(op, vals[a], vals[b], bc, pow_fn)


def noise_graph(dim, vec, scale):
    nodes = _operand_nodes() + [N(abi.NODE_CONST, (), (scale, 9.0, 9.0)), abi.noise(8, 3 if vec else abi.NODE_NONE, dim)]
    return abi.GraphData(nodes, {"base_color": 9})


def noise_expected(case, uv):
    dim, vec, scale = case
    st = operand_values(uv)["V"][:, :2] if vec else np.asarray(uv, dtype=F)
    return M.noise_node(st, scale, dim)


def pow_graph():
    """metallic <- pow(u, v) of two scalars: where the model takes POW from (procedural_model.math_apply)."""
    return abi.GraphData([N(abi.NODE_TEXCOORDS), N(abi.NODE_EXTRACT, (0, abi.FIELD_RED)), N(abi.NODE_EXTRACT, (0, abi.FIELD_GREEN)),
                          abi.math(abi.MATH_POW, 1, 2, 3)], {"metallic": 3})


def fbm_graph(octaves=4):
    """roughness <- 0.5 + 0.5 * sum_i 2^-i noise(2^i uv): fBm from noise and math nodes (scalars throughout)."""
    nodes, acc = [], None
    for i in range(octaves):
        b = len(nodes)
        nodes += [N(abi.NODE_CONST, (), (2.0 ** i, 0, 0)), abi.noise(b, abi.NODE_NONE, 2), N(abi.NODE_CONST, (), (0.5 ** i, 0, 0)), abi.math(abi.MATH_MUL, b + 1, b + 2, 3)]
        if acc is None:
            acc = b + 3
        else:
            nodes.append(abi.math(abi.MATH_ADD, acc, b + 3, 3))
            acc = len(nodes) - 1
    b = len(nodes)
    nodes += [N(abi.NODE_CONST, (), (0.5, 0, 0)), abi.math(abi.MATH_MUL, acc, b, 3), abi.math(abi.MATH_ADD, b + 1, b, 3)]
    return abi.GraphData(nodes, {"roughness": len(nodes) - 1})


def fbm_expected(uv, octaves=4):
    acc = None
    for i in range(octaves):
        n = M.noise_node(uv, 2.0 ** i, 2)
        amp = np.zeros_like(n)
        amp[:, 0] = F(0.5 ** i)
        t = M.math_node(2, n, amp, 3)
        acc = t if acc is None else M.math_node(0, acc, t, 3)
    half = np.zeros_like(acc)
    half[:, 0] = F(0.5)
    return M.math_node(0, M.math_node(2, acc, half, 3), half, 3)[:, 0]


def probe_scene():
    """The textured room with one more material per case. -> (scene data, {name: material index}, cases by name)."""
    sd = textured_room()
    index, cases = {}, {}

    def add(name, graph, case=None):
        index[name] = len(sd.materials)
        cases[name] = case
        sd.materials.append(abi.MaterialData(roughness=0.9, ior=1.0, specular_ior_level=0.0, graph=graph))

    add("pow", pow_graph())
    for c in math_cases():
        add("math-%s-b%d-%s" % (M.MATH_NAMES[c[0]], c[1], c[2]), math_graph(*c), c)
    for c in NOISE_CASES:
        add("noise-d%d-%s-s%g" % (c[0], "vec" if c[1] else "uv", c[2]), noise_graph(*c), c)
    add("fbm", fbm_graph())
    return sd, index, cases


def host_pow(scene, pow_material):
    """pow_f(a, b) of the library's host build, through the scalar POW node (any shape in, the same shape out)."""
    def fn(a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F))
        uv = np.stack([a.ravel(), b.ravel()], axis=1)
        return capi.probe_material_inputs(None, scene, pow_material, uv)[:, 5].reshape(a.shape)
    return fn


# ---------------------------------------------------------------------------------------------- the scene the routes render
COL1, COL2 = (0.85, 0.35, 0.2), (0.1, 0.3, 0.75)


def routes_room(width=32, height=24, n_floor=1):
    """The textured room with procedural inputs: the back wall's base colour is c1 + (c2 - c1) * clamp(0.5 * noise + 0.5) built from math nodes,
    the floor's roughness is min / max-clamped 1D noise, and the ceiling light's strength is noise-driven."""
    sd = textured_room(width, height, n_floor=n_floor)
    sd.materials[1].graph = base_color_graph()
    sd.materials[1].base_color = (0.5, 0.5, 0.5)
    fl = sd.materials[0].graph
    b = len(fl.nodes)
    fl.nodes += [N(abi.NODE_CONST, (), (5.0, 0, 0)), abi.noise(b, abi.NODE_NONE, 1), N(abi.NODE_CONST, (), (0.35, 0, 0)), abi.math(abi.MATH_ADD, b + 1, b + 2, 3),
                 N(abi.NODE_CONST, (), (0.15, 0, 0)), N(abi.NODE_CONST, (), (0.8, 0, 0)), abi.math(abi.MATH_MAX, b + 3, b + 4, 3), abi.math(abi.MATH_MIN, b + 6, b + 5, 3)]
    fl.inputs["roughness"] = b + 7
    li = sd.materials[6].graph
    b = len(li.nodes)
    li.nodes += [N(abi.NODE_CONST, (), (3.0, 0, 0)), abi.noise(b, abi.NODE_NONE, 2), N(abi.NODE_CONST, (), (2.0, 0, 0)), abi.math(abi.MATH_ADD, b + 1, b + 2, 3)]
    li.inputs["emission_strength"] = b + 3
    # one more mesh with two instances, so that option instancing = 1 keeps the scene as meshes + instances: two tiles in front of the back
    # wall with the wall's material
    tile = abi.MeshData(vertices=np.array([[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.2, 0.2, 0], [-0.2, 0.2, 0]], dtype=F), indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32),
                        uvs=np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], dtype=F))
    sd.meshes.append(tile)
    for t in ([-0.45, -0.3, -0.6], [0.4, 0.25, -0.75]):
        m = np.eye(4, dtype=F)
        m[:3, 3] = t
        sd.instances.append(abi.InstanceData(len(sd.meshes) - 1, [1], m.T.reshape(16).copy()))
    return sd


def base_color_graph():
    nodes = [N(abi.NODE_RGB, (), COL1), N(abi.NODE_RGB, (), COL2), abi.math(abi.MATH_SUB, 1, 0, 0),              # 0 c1, 1 c2, 2 c2 - c1
             N(abi.NODE_CONST, (), (6.0, 0, 0)), abi.noise(3, abi.NODE_NONE, 2),                                # 3 scale, 4 noise
             N(abi.NODE_CONST, (), (0.5, 0, 0)), abi.math(abi.MATH_MUL, 4, 5, 3), abi.math(abi.MATH_ADD, 6, 5, 3),  # 5 half, 6, 7 0.5 n + 0.5
             N(abi.NODE_CONST, (), (0.0, 0, 0)), N(abi.NODE_CONST, (), (1.0, 0, 0)),
             abi.math(abi.MATH_MAX, 7, 8, 3), abi.math(abi.MATH_MIN, 10, 9, 3),                                 # 10, 11 clamp to [0, 1]
             abi.math(abi.MATH_MUL, 2, 11, 2), abi.math(abi.MATH_ADD, 0, 12, 0)]                                # 12 (c2 - c1) t, 13 c1 + ...
    return abi.GraphData(nodes, {"base_color": 13})


def base_color_expected(uv, c1, c2):
    """c1, c2: the two Rgb nodes' values in the pipeline's space, (4,) each (w = 1)."""
    n = uv.shape[0]
    a, b = np.tile(np.asarray(c1, dtype=F), (n, 1)), np.tile(np.asarray(c2, dtype=F), (n, 1))

    def k(v):
        out = np.zeros((n, 4), dtype=F)
        out[:, 0] = F(v)
        return out

    d = M.math_node(1, b, a, 0)
    t = M.math_node(0, M.math_node(2, M.noise_node(uv, 6.0, 2), k(0.5), 3), k(0.5), 3)
    t = M.math_node(5, M.math_node(6, t, k(0.0), 3), k(1.0), 3)
    return M.math_node(0, a, M.math_node(2, d, t, 2), 0)
