"""Records tests/golden/pt_launch_plan.json: what akr_host_pt_launch_plan answers for every row of tests/launch_plan_matrix.py.
Recorded once, at the commit before the launch decision moved into PtVariant / pt_lds_layout; tests/test_launch_plan.py holds every later
commit to it. python tests/golden/make_launch_plan_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import launch_plan_matrix as M  # noqa: E402


def pack(rows: dict) -> dict:
    """{plans: the distinct plans, rows: key -> index into plans}"""
    plans, index, keyed = [], {}, {}
    for key, plan in rows.items():
        t = json.dumps(plan)
        if t not in index:
            index[t] = len(plans)
            plans.append(plan)
        keyed[key] = index[t]
    return {"layout": ["variant x 10"] + list(M.FIELDS) + ["stage_bytes x 13", "wrapper sha256[:16]"], "plans": plans, "rows": keyed}


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "pt_launch_plan.json")
    packed = pack(M.rows())
    with open(out, "w") as f:
        f.write("{\n\"layout\": " + json.dumps(packed["layout"]) + ",\n\"plans\": [\n" + ",\n".join(json.dumps(p, separators=(",", ":")) for p in packed["plans"]) +
                "\n],\n\"rows\": " + json.dumps(packed["rows"], separators=(",", ":")) + "\n}\n")
    print(len(packed["rows"]), "rows,", len(packed["plans"]), "distinct plans ->", out)
