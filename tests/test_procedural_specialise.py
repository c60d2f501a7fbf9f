"""Per-scene code for the procedural nodes (csrc/host/specialise.cpp), CPU side: the text generated for graphs with CONST4, MATH and
NOISE nodes, compiled for the host with the library's headers and flags, computes what the interpreter computes, bit for bit; a math node's
op and broadcast bits and a noise node's dimension are part of a material's shader kind, a float4's w is not."""
import ctypes as C
import subprocess

import numpy as np

from akari_render_amd import abi, build as B, capi
from tests import procedural_cases as PC

N = abi.NodeData

HOST_SRC = r'''
#define AKR_SPEC_GRAPHS 1
#include "device/dtex.h"
using namespace akr;
extern "C" __attribute__((visibility("default"))) void spec_host_eval(const void* nodes, const void* images, const void* texels, const void* mat_inputs, const void* materials,
                               uint32_t material, uint32_t n, const float* uv, uint32_t* out64, float* alpha, float* emission3) {
    const TexScene ts{(const DNode*)nodes, (const DImage*)images, (const uint32_t*)texels, (const MatInputs*)mat_inputs, 0, 0};
    const DMaterial& folded = ((const DMaterial*)materials)[material];
    for (uint32_t i = 0; i < n; i++) {
        const vec2 p = mk2(uv[2 * i], uv[2 * i + 1]);
        DMaterial m = folded;
        material_at(ts, material, p, m);
        __builtin_memcpy(out64 + 64ull * i, &m, sizeof m);
        const bool tex = (folded.flags & MF_TEXTURED) != 0;
        alpha[i] = tex ? material_alpha_at(ts, folded, material, p) : folded.base_alpha;
        const vec3 e = tex ? material_emission_inputs_at(ts, folded, material, p) : folded.emission;
        emission3[3 * i] = e.x; emission3[3 * i + 1] = e.y; emission3[3 * i + 2] = e.z;
    }
}
'''


def _host_module(tmp_path, header):
    (tmp_path / "akr_scene_spec.h").write_text(header)
    (tmp_path / "host.hip").write_text(HOST_SRC)
    so = tmp_path / "libspec_host.so"
    cmd = (["/opt/rocm/bin/hipcc"] + [f for f in B.FLAGS if not f.startswith("--offload-arch")]
           + ["--cuda-host-only", "-shared", str(tmp_path / "host.hip"), "-I", B.CSRC, "-I", str(tmp_path), "-o", str(so)])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    L = C.CDLL(str(so))
    L.spec_host_eval.restype = None
    return L


def _same_as_interpreter(L, sc, uv):
    nodes, images = sc.array(capi.ARRAY_TEX_NODES, np.uint8), sc.array(capi.ARRAY_TEX_IMAGES, np.uint8)
    texels, inputs = sc.array(capi.ARRAY_TEX_TEXELS, np.uint32), sc.array(capi.ARRAY_MAT_INPUTS, np.uint8)
    mats = sc.array(capi.ARRAY_MATERIALS, np.uint32).reshape(-1, 64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for mi in range(mats.shape[0]):
        want, want_a, want_e = sc.material_folded_host(mi, uv)
        got, got_a, got_e = np.zeros_like(want), np.zeros_like(want_a), np.zeros_like(want_e)
        L.spec_host_eval(vp(nodes), vp(images), vp(texels), vp(inputs), vp(mats), C.c_uint32(mi), C.c_uint32(uv.shape[0]), vp(uv), vp(got), vp(got_a), vp(got_e))
        assert np.array_equal(want, got), f"material {mi}: folded record differs in words {np.argwhere(want != got)[:8].tolist()}"
        assert np.array_equal(want_a.view(np.uint32), got_a.view(np.uint32)), f"material {mi}: alpha differs"
        assert np.array_equal(want_e.view(np.uint32), got_e.view(np.uint32)), f"material {mi}: emission differs"


def test_generated_code_is_the_interpreter_on_procedural_graphs(hip_lib, tmp_path):
    """The room the routes render, and next to it materials of one shape that differ in a math op, in broadcast bits, in a noise dimension (a kind
    each) and in a float4's w alone (one kind, w read from the node record)."""
    sd = PC.routes_room()

    def variant(op=abi.MATH_MUL, bc=1, dim=2, w=1.0):
        g = abi.GraphData([N(abi.NODE_CONST, (), (4.0, 0, 0)), abi.noise(0, abi.NODE_NONE, dim), abi.const4(0.6, 0.5, 0.4, w), abi.math(op, 1, 2, bc)], {"base_color": 3})
        sd.materials.append(abi.MaterialData(roughness=0.9, ior=1.0, specular_ior_level=0.0, graph=g))

    first = len(sd.materials)
    variant(), variant(w=0.5), variant(op=abi.MATH_ADD), variant(bc=0), variant(dim=1)
    sc = capi.Scene(None, sd)
    src = sc.spec_source()
    assert "node_noise(uv, v" in src and "node_math(" in src and "node_const4(" in src
    assert src.count("node_const4(") > src.count("nd[2].arg[0])") >= 1  # the shared kind reads w from the record, the others have it as a literal
    # materials first and first + 1 share a kind; the other three have one each
    titles = [ln for ln in src.split("spec_alpha")[0].splitlines() if ln.startswith("    case ")]
    owners = {m: t for t in titles for m in t.split("materials")[1].split()}
    assert owners[str(first)] == owners[str(first + 1)]
    assert len({owners[str(first + k)] for k in range(5)}) == 4
    _same_as_interpreter(_host_module(tmp_path, src), sc, np.ascontiguousarray(PC.probe_points()[::4]))
