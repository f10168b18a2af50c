"""Shared by tools/make_halo_plan_golden.py (the recorder), tests/test_sharding.py and tests/test_halo_plan_host.py (the replays): the cases whose halo-exchange plans
tests/golden/halo_plans.json pins -- for every case the restart frame and two steady-state frames (ping-pong), every rank, uneven strips."""
import json
import os

import parity
from raytracingdenoiser_amd import api

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halo_plans.json")
FRAMES, MAX_MOTION_ROWS, EXCHANGE_THRESHOLD = 3, 32, 24
# (name, size, world, overrides, cs_kw)
CASES = [
    ("REBLUR_DIFFUSE_SPECULAR", (2560, 1440), 8, None, None),
    ("REBLUR_DIFFUSE_SPECULAR", (2560, 1440), 4, dict(enablePerformanceMode=True, maxBlurRadius=12.0), None),
    ("REBLUR_DIFFUSE_SPECULAR", (640, 360), 8, None, None),                                   # 45-row strips: the PostBlur halo does not fit -> unsharded
    ("REBLUR_DIFFUSE_SPECULAR_OCCLUSION", (1920, 1080), 4, None, None),                        # the user's OUT planes are the history
    ("REBLUR_DIFFUSE_SH", (1920, 1080), 3, dict(hitDistanceReconstructionMode=1), None),       # the pre-pass gathers from the reconstruction's output: reach = its blur radius
    ("RELAX_DIFFUSE_SPECULAR", (1920, 1080), 3, dict(hitDistanceReconstructionMode=2), None),
    ("RELAX_DIFFUSE_SPECULAR_SH", (3840, 2160), 8, None, None),
    ("RELAX_SPECULAR", (1920, 1080), 2, dict(atrousIterationNum=8), None),
    ("RELAX_DIFFUSE", (1920, 1080), 2, dict(enableAntiFirefly=True), None),                    # Copy (texel to texel) + AntiFirefly (3x3)
    ("SIGMA_SHADOW", (1920, 1080), 4, None, None),
]


def key(name, size, world, overrides):
    return "%s %dx%dx%d" % (name, size[0], size[1], world) + ("" if not overrides else " " + json.dumps(overrides, sort_keys=True))


def strip_bounds(height, world):
    return [0] + [(r * height // world) + (7 if r % 2 else -5) for r in range(1, world)] + [height]  # uneven on purpose


def frames(name, size, overrides, cs_kw):
    """one instance driven through the FRAMES frames of a case: yields (instance, common settings, denoiser settings, dispatch pointer, count) per frame"""
    inst = api.Instance([(0, parity.DENOISERS[name][0])])
    seq = parity.generate_sequence(name, 32, 18, FRAMES)
    for f in range(FRAMES):
        settings = parity.denoiser_settings(name, seq[f], overrides)
        inst.set_denoiser_settings(0, settings)
        cs = parity.common_settings(seq[f]["camera"], seq[max(f - 1, 0)]["camera"], size[0], size[1], f, **(cs_kw or {}))
        assert inst.set_common_settings(cs) == api.Result.SUCCESS
        r, ptr, n = inst.get_compute_dispatches_raw()
        assert r == api.Result.SUCCESS
        yield inst, cs, settings, ptr, n


def plan_record(plan):
    """a sharding.HaloPlan as plain JSON values"""
    return {"fallback": bool(plan.fallback), "steps": [[[[list(k), wd] for k, wd in items], first, count] for items, first, count in plan.steps], "early": list(plan.early),
            "row_begin": list(plan.row_begin), "row_end": list(plan.row_end)}


def load():
    with open(PATH) as fp:
        return json.load(fp)
