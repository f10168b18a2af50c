"""Records tests/golden/halo_plans.json: the halo-exchange plan (sharding.plan_halo_exchange) and the per-dispatch reach of every case of tests/halo_plan_cases.py -- every frame,
every rank, as plain values. tests/test_sharding.py and tests/test_halo_plan_host.py hold the planner (csrc/host/halo_plan.cpp) against the file, so it is re-recorded only when a
planning rule is changed on purpose; the diff of the file then shows what the change did to the plans.
usage: python tools/make_halo_plan_golden.py        (parameters: tests/halo_plan_cases.py)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import halo_plan_cases as G  # noqa: E402
from raytracingdenoiser_amd import sharding  # noqa: E402


def record(name, size, world, overrides, cs_kw):
    bounds, out = G.strip_bounds(size[1], world), []
    for inst, _, _, ptr, n in G.frames(name, size, overrides, cs_kw):
        plans = [sharding.plan_halo_exchange(inst, ptr, n, bounds, rank, size[1], G.MAX_MOTION_ROWS, G.EXCHANGE_THRESHOLD) for rank in range(world)]
        out.append({"reach": list(plans[0].reach), "ranks": [G.plan_record(p) for p in plans]})
    return out


if __name__ == "__main__":
    out = {G.key(*case[:4]): record(*case) for case in G.CASES}
    with open(G.PATH, "w") as fp:  # one case per line: compact, and a re-recording diffs case by case
        fp.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in sorted(out.items())) + "\n}\n")
    print("%s: %d cases, %d plans, %.0f KB" % (os.path.relpath(G.PATH, ROOT), len(out), sum(len(f["ranks"]) for v in out.values() for f in v), os.path.getsize(G.PATH) / 1024.0))
