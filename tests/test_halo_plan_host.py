"""The sharding planner is host-only code (raytracingdenoiser_amd/csrc/host/halo_plan.cpp; include/NRDHip.h: "needs no device"): tests/cpp/halo_plan_host.cpp links from
csrc/host/*.cpp alone -- no HIP runtime -- under AddressSanitizer + UndefinedBehaviorSanitizer, plans two of the recorded cases for every rank (with too small and with exactly
sized arrays, and for one rank) and prints what tests/golden/halo_plans.json holds. A stand-alone program on the CPU: nothing is loaded into python."""
import json
import os
import subprocess

import halo_plan_cases as G
import parity
from raytracingdenoiser_amd import build as native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "halo_plan_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "halo_plan_host")
CLANG = os.environ.get("NRD_EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wno-return-type-c-linkage", "-I" + os.path.join(ROOT, "include")]
CASES = [c for c in G.CASES if (c[0], c[1], c[2]) in (("REBLUR_DIFFUSE_SPECULAR", (2560, 1440), 8), ("SIGMA_SHADOW", (1920, 1080), 4)) and not c[3]]


def _build():
    host, _ = native_build._sources()
    deps = host + [SRC] + [os.path.join(d, f) for base in (os.path.join(ROOT, "include"), native_build.CSRC) for d, _, files in os.walk(base) for f in files if f.endswith(".h")]
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(p) for p in deps):
        return
    # the host sources and the program, nothing else: no -lamdhip64, no device code
    r = subprocess.run([CLANG] + FLAGS + native_build.encoding_flags() + host + [SRC, "-o", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_planner_links_without_hip_and_runs_clean_under_sanitizers(tmp_path):
    assert len(CASES) == 2
    _build()
    lines = []
    for name, size, world, overrides, cs_kw in CASES:
        lines.append("case %d %d %d %d %d %d %s" % (int(parity.DENOISERS[name][0]), size[1], G.MAX_MOTION_ROWS, G.EXCHANGE_THRESHOLD, G.FRAMES, world,
                                                    " ".join(str(b) for b in G.strip_bounds(size[1], world))))
        for _, cs, settings, _, _ in G.frames(name, size, overrides, cs_kw):
            lines.append("%s %s" % (bytes(cs).hex(), bytes(settings).hex()))
    cases_file = tmp_path / "cases.txt"
    cases_file.write_text("\n".join(lines) + "\n")
    r = subprocess.run([EXE, str(cases_file)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert not [line for line in r.stderr.splitlines() if "Sanitizer" in line or "runtime error" in line], r.stderr[-3000:]  # (-fno-sanitize-recover: a report also ends the program)
    got, recorded = json.loads(r.stdout), G.load()
    assert len(got) == len(CASES)
    for plans, (name, size, world, overrides, _) in zip(got, CASES):
        want = recorded[G.key(name, size, world, overrides)]
        assert all(not rank["fallback"] for frame in want for rank in frame["ranks"])  # (a plan that falls back is recorded without rows)
        assert len(plans) == len(want) == G.FRAMES
        for f, (frame, want_frame) in enumerate(zip(plans, want)):
            assert frame["reach"] == want_frame["reach"], (name, f)
            assert len(frame["ranks"]) == world
            for rank, (plan, want_plan) in enumerate(zip(frame["ranks"], want_frame["ranks"])):
                for field in ("fallback", "steps", "early", "row_begin", "row_end"):
                    assert plan[field] == want_plan[field], (name, f, rank, field)
