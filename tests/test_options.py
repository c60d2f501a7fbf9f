"""The process-wide options (akr_option_set / akr_option_get) are one table (csrc/host/options.cpp), and the table reads the environment as
the commit before it did.

How an AKR_* variable becomes an option's value differs from variable to variable (a first-character flag, atoi != 0, raw atoi, atoi clamped
to a range, the strings of AKR_PT_MODE) and had no test. tests/golden/option_env.json holds what the parent of the commit that introduced the
table read from a dozen environments; its "recorded_with" field holds the command and "commit" the commit. Every environment is a fresh child
process (the variables are looked at once per process); no child opens a GPU.

The rest is asserted over the table itself, through the test hook akr_host_option_info: names and variables are unique, defaults are what a
process with no variable set sees, akr_option_set refuses exactly what lies outside a declared range and leaves the value alone, and the table,
the option comment of include/akari_hip.h and INTEGRATION.md name the same options."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from akari_render_amd import capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "option_env.json")
PROBES = ("1", "0", "2", "-5", "10", "100000000", "abc", "")
PT_MODES = ("wavefront", "auto", "megakernel")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

CHILD = "import json, sys; sys.path.insert(0, sys.argv[1]); from akari_render_amd import capi; print(json.dumps({n: capi.get_option(n) for n in sys.argv[2:]}))"


def header_options():
    """[(name, variable or "")] of the entries of the option comment of include/akari_hip.h: the lines that start with a quoted name."""
    text = open(os.path.join(ROOT, "include", "akari_hip.h")).read()
    comment = text[text.index("/* Process-wide tuning switches"):text.index("AKR_API int32_t akr_option_set")]
    return [(m.group(1), m.group(2) or "") for m in re.finditer(r'^ \*   "(\w+)"\s*\((?:(AKR_\w+)|no environment hook)', comment, re.M)], comment


def environments(variables):
    """label -> the option variables a child runs with: every one set to a probe string, none, AKR_PT_MODE alone."""
    envs = {"all=" + p: {v: p for v in variables} for p in PROBES}
    envs["none"] = {}
    for m in PT_MODES:
        envs["AKR_PT_MODE=" + m] = {"AKR_PT_MODE": m}
    return envs


def run_children(names, variables):
    """label -> {option: value}, one fresh Python process per environment (started together, none touches a device)."""
    base = {k: v for k, v in os.environ.items() if k not in variables}
    flags = ["-s"] if sys.flags.no_user_site else []
    procs = {label: subprocess.Popen([sys.executable] + flags + ["-c", CHILD, ROOT] + list(names), env={**base, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for label, env in environments(variables).items()}
    out = {}
    for label, p in procs.items():
        so, se = p.communicate()
        assert p.returncode == 0, (label, se[-2000:])
        out[label] = json.loads(so.strip().splitlines()[-1])
    return out


@pytest.fixture(scope="module")
def table(hip_lib):
    return capi.option_table()


@pytest.fixture(scope="module")
def children(table):
    return run_children([r["name"] for r in table], sorted(r["env"] for r in table if r["env"]))


def test_table_has_no_duplicates(table):
    names = [r["name"] for r in table]
    variables = [r["env"] for r in table if r["env"]]
    assert len(names) == 32 and len(set(names)) == len(names)
    assert len(set(variables)) == len(variables) and all(v.startswith("AKR_") for v in variables)


def test_environment_is_read_as_the_parent_read_it(table, children):
    gold = json.load(open(GOLDEN))
    assert gold["commit"] and sorted(gold["options"]) == sorted(r["name"] for r in table)
    assert sorted(gold["variables"]) == sorted(r["env"] for r in table if r["env"])
    assert sorted(gold["children"]) == sorted(children) and len(children) == len(PROBES) + 1 + len(PT_MODES)
    diff = [(label, n, children[label][n], want) for label, vals in gold["children"].items() for n, want in vals.items() if children[label][n] != want]
    print(diff)
    assert diff == []


def test_defaults_are_what_no_environment_gives(table, children):
    assert {r["name"]: r["default"] for r in table} == children["none"]


def test_option_set_checks_the_declared_ranges(table):
    def refused(name, value):
        before = capi.get_option(name)
        with pytest.raises(capi.AkariError) as e:
            capi.set_option(name, value)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, (name, value)
        assert capi.get_option(name) == before, (name, value)

    unranged = []
    for r in table:
        name, start = r["name"], capi.get_option(r["name"])
        try:
            if r["range"] is None:
                unranged.append(name)
                for v in (INT32_MIN, INT32_MAX):
                    capi.set_option(name, v)
                    assert capi.get_option(name) == v
                continue
            lo, hi = r["range"]
            assert lo <= r["default"] <= hi
            for v in (lo, hi):
                capi.set_option(name, v)
                assert capi.get_option(name) == v
            refused(name, lo - 1)
            refused(name, hi + 1)
        finally:
            capi.set_option(name, start)
    assert sorted(unranged) == ["bvh_balanced", "defer_metal", "force_bvh", "simple_kernels"]  # (as before the table; a finding, not a decision)
    refused("specialise_waves", 1)  # 0 or 2..4: the one hole in a range
    with pytest.raises(capi.AkariError) as e:
        capi.set_option("no_such_option", 1)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.AkariError):
        capi.get_option("no_such_option")


def test_the_documents_name_the_tables_options(table):
    entries, comment = header_options()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for r in table:
        for word in filter(None, (r["name"], r["env"])):
            assert re.search(r"\b%s\b" % word, comment), word + " is not in the option comment of include/akari_hip.h"
            assert re.search(r"\b%s\b" % word, integration), word + " is not in INTEGRATION.md"
    assert len(entries) == len(table)
    assert sorted(entries) == sorted((r["name"], r["env"]) for r in table)


if __name__ == "__main__":  # --record OUT.json, with AKR_HIP_LIB = a library built from the parent commit (names and variables: the header's comment)
    entries, _ = header_options()
    names, variables = [n for n, _ in entries], sorted(v for _, v in entries if v)
    out = {"recorded_with": "AKR_HIP_LIB=<libakari_hip.so built from the parent commit> python tests/test_options.py --record OUT.json --commit <that commit>",
           "commit": sys.argv[sys.argv.index("--commit") + 1], "options": names, "variables": variables, "children": run_children(names, variables)}
    json.dump(out, open(sys.argv[sys.argv.index("--record") + 1], "w"), indent=1, sort_keys=True)
