"""Builds libakari_hip.so in-tree with hipcc for gfx950 (no JIT cache: the .so travels with the repo)."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libakari_hip.so")

# The precompiled pt kernels: pt_unit_kernels.hip compiled once per unit (kind, ENV, LENS), with -DAKR_PT_UNIT=<index>. The kinds, their order
# and the index are those of csrc/kernels.h (PtKind, pt_unit_index): the two lists go together. The router (pt_kernels.hip) names kPtUnits
# entry points, so a unit missing here is an undefined symbol of the library, and one too many does not compile.
PT_KINDS = ["plain", "inst", "feat", "punct", "punct_tree"]
PT_UNITS = {"pt_unit_" + kind + ("_env" if env else "") + ("_lens" if lens else ""): 4 * k + 2 * env + lens
            for k, kind in enumerate(PT_KINDS) for env in (0, 1) for lens in (0, 1)}

# A source is a file under csrc/, or the name of a pt unit (e.g. "pt_unit_punct_tree_env_lens"): what `only` of build_variant and
# tools/kernel_resources.py take too. Its object is named after it.
SOURCES = [
    "pt_kernels.hip", "pt_kernels_relaxed.hip", *PT_UNITS, "probe_kernels.hip",
    "wf_env_kernels.hip",  # the instantiations of scenes with an environment light
    "wf_lens_kernels.hip", "aov_lens_kernels.hip",  # ... of cameras with a thin lens
    "wf_kernels.hip", "wf_sort.hip",
    "cost_order_kernels.hip",  # a pt session's item -> pixel table, sorted by measured pixel cost
    "aov_kernels.hip", "gpt_kernels.hip", "mcmc_kernels.hip", "denoise_kernels.hip", "adapt_kernels.hip", "display_kernels.hip",
    "host/options.cpp", "host/api_common.cpp", "host/api_scene.cpp", "host/api_pt.cpp", "host/pt_plan.cpp", "host/wf_schedule.cpp", "host/api_aux.cpp", "host/api_task.cpp", "host/api_probe.cpp", "host/api_denoise.cpp", "host/api_adapt.cpp", "host/api_display.cpp",
    "host/scene_build.cpp", "host/scene_inst.cpp", "host/scene_env.cpp", "host/scene_punct.cpp",
    "host/scene_json.cpp",
    "host/bvh.cpp",
    "host/image_io.cpp",
    "host/image_formats.cpp",
    "host/pmj_tables.cpp",
    "host/comm.cpp",
    "host/specialise.cpp",
]
# The in-tree library is the TEST build: it carries the test hooks of include/akari_hip_test.h (host known-answer functions, device probes).
# AKR_SHIP=1 in the environment builds the library a host application ships: the boundary of include/akari_hip.h and nothing else.
TEST_HOOKS = os.environ.get("AKR_SHIP", "0") != "1"


def _headers():
    """Every header the sources can include: all of csrc/ and the public header (a forgotten entry in a hand-kept list
    means a stale library that still loads)."""
    out = []
    for d, _, files in os.walk(CSRC):
        out += [os.path.relpath(os.path.join(d, f), CSRC) for f in files if f.endswith(".h")]
    return sorted(out) + ["../../include/akari_hip.h", "../../include/akari_hip_test.h"]


# -ffp-contract=off + correctly rounded div/sqrt: the arithmetic contract of DESIGN.md ("AKR-F32")
FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
    "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
    # packed-f32 SLP vectorisation costs s_mov shuffles of the SGPR triangle records (-5 % on the bench)
    "-fno-slp-vectorize",
    "-Wall", "-Wno-unused-function", "-x", "hip",
] + (["-DAKR_TEST_HOOKS=1"] if TEST_HOOKS else [])


# The relaxed arithmetic tier (option `arith`; device/dmath.h AKR_ARITH_RELAXED): its one translation unit drops the three flags that
# make up the contract (the later flag wins) -- contraction allowed, v_rcp_f32 / v_sqrt_f32 instead of the correctly rounded
# sequences, denormals flushed (the precondition for the compiler to use them without range scaling).
RELAXED_FLAGS = ["-ffp-contract=fast", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fgpu-flush-denormals-to-zero"]
SOURCE_FLAGS = {"pt_kernels_relaxed.hip": RELAXED_FLAGS, **{u: ["-DAKR_PT_UNIT=%d" % i] for u, i in PT_UNITS.items()}}


def source_file(src: str) -> str:
    """The file under csrc/ that source `src` is compiled from."""
    return "pt_unit_kernels.hip" if src in PT_UNITS else src


# What a per-scene kernel is compiled from at run time (host/specialise.cpp, hiprtc): the device headers and kernels.h, embedded
# in the library as text, with the flags that define the arithmetic (the same as the library's own).
RTC_FLAG_SKIP = ("--offload-arch", "-fPIC", "-fvisibility", "-W", "-x", "hip", "-DAKR_TEST_HOOKS")
GEN = os.path.join(HERE, "build", "gen")


def _rtc_flags(extra):
    out = []
    for f in FLAGS + list(extra):
        if f.startswith(RTC_FLAG_SKIP) or f == "hip":
            continue
        out.append(f)
    return out


def write_embedded_sources(extra=(), gen_dir=None) -> str:
    """<gen_dir>/embedded_src.inc (default build/gen): {name, text} of every header a per-scene kernel includes + a hash of texts
    and flags. A variant build writes its own, with its own flags: the per-scene kernels of a variant must be the variant's."""
    import hashlib
    gen_dir = gen_dir or GEN

    names = ["kernels.h"] + sorted("device/" + f for f in os.listdir(os.path.join(CSRC, "device")) if f.endswith(".h"))
    h = hashlib.sha256()
    parts = ["// generated by akari_render_amd/build.py -- do not edit\n", "static const akr::EmbeddedSource kEmbeddedSources[] = {\n"]
    for n in names:
        text = open(os.path.join(CSRC, n)).read()
        assert ')AKRSRC"' not in text
        h.update(n.encode() + b"\0" + text.encode() + b"\0")
        # (a raw string literal may not exceed the compiler's limit in one piece: split at line boundaries, adjacent literals concatenate)
        chunks, cur = [], ""
        for line in text.splitlines(keepends=True):
            if len(cur) + len(line) > 12000:
                chunks.append(cur)
                cur = ""
            cur += line
        chunks.append(cur)
        parts.append('    {"%s",\n' % n + "\n".join('R"AKRSRC(' + c + ')AKRSRC"' for c in chunks) + "},\n")
    parts.append("};\n")
    flags = _rtc_flags(extra)
    h.update(" ".join(flags).encode())
    parts.append('static const char kEmbeddedHash[] = "%s";\n' % h.hexdigest()[:32])
    parts.append("static const char* const kEmbeddedFlags[] = {" + ", ".join('"%s"' % f for f in flags) + "};\n")
    os.makedirs(gen_dir, exist_ok=True)
    path = os.path.join(gen_dir, "embedded_src.inc")
    new = "".join(parts)
    if not os.path.exists(path) or open(path).read() != new:
        open(path, "w").write(new)
    return path


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    for f in [source_file(s) for s in SOURCES] + _headers() + ["../build.py"]:
        p = os.path.normpath(os.path.join(CSRC, f))
        if os.path.exists(p) and os.path.getmtime(p) > t:
            return True
    return False


CLI = os.path.join(HERE, "akari-cli")


def build_cli(verbose: bool = False) -> str:
    """akari-cli: the reference's command line (crates/akari_api/src/bin/akari_cli.rs) over libakari_hip.so."""
    src = os.path.join(CSRC, "host", "cli_main.cpp")
    if os.path.exists(CLI) and os.path.getmtime(CLI) > max(os.path.getmtime(src), os.path.getmtime(LIB)):
        return CLI
    cmd = ["g++", "-O2", "-std=c++17", src, "-I", os.path.join(HERE, "..", "include"), "-L", HERE, "-lakari_hip",
           "-Wl,-rpath,$ORIGIN", "-o", CLI]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError("g++ failed:\n" + res.stdout)
    return CLI


OBJ = os.path.join(HERE, "build", "obj")  # git-ignored; objects are rebuilt per source file, in parallel


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        build_cli(verbose)
        return LIB
    from concurrent.futures import ThreadPoolExecutor

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("AKR_EXTRA_HIPCC_FLAGS", "").split()
    os.makedirs(OBJ, exist_ok=True)
    write_embedded_sources(extra)
    tag = os.path.join(OBJ, "flags.txt")  # objects built with other flags are stale
    flags_now = " ".join(FLAGS + extra)
    if force or not os.path.exists(tag) or open(tag).read() != flags_now:
        for f in os.listdir(OBJ):
            os.remove(os.path.join(OBJ, f))
    newest_header = max([os.path.getmtime(os.path.normpath(os.path.join(CSRC, h))) for h in _headers()] + [os.path.getmtime(os.path.abspath(__file__))])

    def compile_one(src: str):
        obj = os.path.join(OBJ, src.replace("/", "_") + ".o")
        path = os.path.join(CSRC, source_file(src))
        if os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(path), newest_header):
            return obj, 0, ""
        cmd = [hipcc] + FLAGS + extra + SOURCE_FLAGS.get(src, []) + ["-c", path, "-I", CSRC, "-I", GEN, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return obj, res.returncode, res.stdout

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4)) as ex:
        results = list(ex.map(compile_one, SOURCES))
    log = "".join(out for _, _, out in results)
    if any(rc != 0 for _, rc, _ in results):
        raise RuntimeError("hipcc failed:\n" + log)
    open(tag, "w").write(flags_now)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + [o for o, _, _ in results] + ["-ldl", "-o", LIB]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc (link) failed:\n" + log + res.stdout)
    if verbose and (log + res.stdout).strip():
        print(log + res.stdout, file=sys.stderr)
    build_cli(verbose)
    return LIB


def build_variant(name: str, extra_flags, verbose: bool = False, only=None) -> str:
    """An A/B build of the library with extra compiler flags (e.g. -DAKR_PT_STRAGGLERS=4) next to the product:
    akari_render_amd/variants/libakari_hip_<name>.so, selected at run time with AKR_HIP_LIB=<path> (measurement only).
    only = the sources the flags concern (e.g. ["pt_unit_plain"]): the others are linked from the product's objects."""
    from concurrent.futures import ThreadPoolExecutor

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(HERE, "build", "obj_" + name)
    out_dir = os.path.join(HERE, "variants")
    os.makedirs(obj, exist_ok=True)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, f"libakari_hip_{name}.so")
    if only:
        build(verbose=verbose)  # the product's objects must be current

    # the variant's own embedded sources (its flags shape the LDS layout of its per-scene kernels too): host/specialise.cpp is always
    # rebuilt against them, whatever `only` says
    gen = os.path.join(obj, "gen")
    write_embedded_sources(extra_flags, gen)
    if only and "host/specialise.cpp" not in only:
        only = list(only) + ["host/specialise.cpp"]

    def compile_one(src: str):
        if only and src not in only:
            return os.path.join(OBJ, src.replace("/", "_") + ".o"), 0, ""
        o = os.path.join(obj, src.replace("/", "_") + ".o")
        # (the variant's flags last: they can take back one of a source's own, e.g. -ffp-contract=off for pt_kernels_relaxed.hip)
        res = subprocess.run([hipcc] + FLAGS + SOURCE_FLAGS.get(src, []) + list(extra_flags) + ["-c", os.path.join(CSRC, source_file(src)), "-I", CSRC, "-I", gen, "-o", o],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return o, res.returncode, res.stdout

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4)) as ex:
        results = list(ex.map(compile_one, SOURCES))
    if any(rc != 0 for _, rc, _ in results):
        raise RuntimeError("hipcc failed:\n" + "".join(o for _, _, o in results))
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + [o for o, _, _ in results] + ["-ldl", "-o", out],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc (link) failed:\n" + res.stdout)
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--variant":  # --variant NAME [--only a.hip,b.cpp] FLAGS...
        rest = sys.argv[3:]
        only = None
        if rest and rest[0] == "--only":
            only, rest = rest[1].split(","), rest[2:]
        print(build_variant(sys.argv[2], rest, verbose=True, only=only))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
