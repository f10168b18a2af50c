"""The reader of a dispatch list is host-only code (raytracingdenoiser_amd/csrc/host/dispatch_list.cpp): tests/cpp/dispatch_list_host.cpp links from csrc/host/*.cpp alone -- no HIP
runtime -- under AddressSanitizer + UndefinedBehaviorSanitizer, scans the lists of the cases below (one of them with its first family block nulled, one with it a byte short, in
a heap allocation of exactly that size) and prints the scans. What they must hold is computed HERE, from the settings this file wrote and NRD's documented inputs and outputs of
each denoiser -- the library is not asked. A stand-alone program on the CPU: nothing is loaded into python."""
import json
import os
import subprocess

from raytracingdenoiser_amd import api, scene, synth
from raytracingdenoiser_amd import build as native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dispatch_list_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "dispatch_list_host")
CLANG = os.environ.get("NRD_EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wno-return-type-c-linkage", "-I" + os.path.join(ROOT, "include")]
W, H, FRAME = 64, 48, 5
NONE, REBLUR, RELAX, SIGMA, REFERENCE = range(5)  # csrc/host/dispatch_list.h Family
RT = api.ResourceType
GUIDES = {RT.IN_MV, RT.IN_NORMAL_ROUGHNESS, RT.IN_VIEWZ}
REBLUR_DS = GUIDES | {RT.IN_DIFF_RADIANCE_HITDIST, RT.IN_SPEC_RADIANCE_HITDIST, RT.OUT_DIFF_RADIANCE_HITDIST, RT.OUT_SPEC_RADIANCE_HITDIST}
RELAX_DS_SH = GUIDES | {RT.IN_DIFF_SH0, RT.IN_DIFF_SH1, RT.IN_SPEC_SH0, RT.IN_SPEC_SH1, RT.OUT_DIFF_SH0, RT.OUT_DIFF_SH1, RT.OUT_SPEC_SH0, RT.OUT_SPEC_SH1}
SIGMA_SHADOW = GUIDES | {RT.IN_PENUMBRA, RT.OUT_SHADOW_TRANSLUCENCY}
MIXED = GUIDES | {RT.IN_DIFF_RADIANCE_HITDIST, RT.OUT_DIFF_RADIANCE_HITDIST, RT.IN_SPEC_RADIANCE_HITDIST, RT.OUT_SPEC_RADIANCE_HITDIST}
D = api.Denoiser

# (label, mutation, [(denoiser, settings)], CommonSettings overrides, first family, checkerboard cells (diff, spec), slots named, slots named outside REBLUR, IN_MV written)
# IN_MV written: REBLUR's TemporalStabilization binds IN_MV as an output in every list, as the reference's does; the kernel patches it only under specular MV modification
CASES = [
    ("reblur", 0, [(D.REBLUR_DIFFUSE_SPECULAR, api.ReblurSettings())], {}, REBLUR, (2, 2), REBLUR_DS, set(), True),
    ("reblur shifted", 0, [(D.REBLUR_DIFFUSE_SPECULAR, api.ReblurSettings())], dict(rectOrigin=(16, 8), resourceSize=(W + 16, H + 8), resourceSizePrev=(W + 16, H + 8)), REBLUR, (2, 2), REBLUR_DS, set(), True),
    ("reblur mv modification", 0, [(D.REBLUR_DIFFUSE_SPECULAR, api.ReblurSettings())], dict(isBaseColorMetalnessAvailable=True), REBLUR, (2, 2), REBLUR_DS | {RT.IN_BASECOLOR_METALNESS}, set(), True),
    ("relax checkerboard", 0, [(D.RELAX_DIFFUSE_SPECULAR_SH, api.RelaxSettings(checkerboardMode=api.CheckerboardMode.BLACK))], {}, RELAX, (0, 1), RELAX_DS_SH, RELAX_DS_SH, False),
    ("sigma", 0, [(D.SIGMA_SHADOW, api.SigmaSettings(lightDirection=(0.3, 0.8, 0.5)))], dict(viewZScale=2.0, denoisingRange=1000.0), SIGMA, (2, 2), SIGMA_SHADOW, SIGMA_SHADOW, False),
    ("reference", 0, [(D.REFERENCE, api.ReferenceSettings())], {}, REFERENCE, (2, 2), {RT.IN_SIGNAL, RT.OUT_SIGNAL}, {RT.IN_SIGNAL, RT.OUT_SIGNAL}, False),
    ("mixed", 0, [(D.REBLUR_DIFFUSE, api.ReblurSettings()), (D.RELAX_SPECULAR, api.RelaxSettings())], {}, REBLUR, (2, 2), MIXED,
     GUIDES | {RT.IN_SPEC_RADIANCE_HITDIST, RT.OUT_SPEC_RADIANCE_HITDIST}, True),
    ("empty", 1, [(D.REBLUR_DIFFUSE_SPECULAR, api.ReblurSettings())], {}, NONE, (2, 2), set(), set(), False),
    ("first block null", 2, [(D.REBLUR_DIFFUSE_SPECULAR, api.ReblurSettings())], dict(rectOrigin=(16, 8), resourceSize=(W + 16, H + 8), resourceSizePrev=(W + 16, H + 8)), REBLUR, (2, 2), REBLUR_DS, set(), True),
    ("first block short", 3, [(D.REBLUR_DIFFUSE_SPECULAR, api.ReblurSettings())], dict(rectOrigin=(16, 8), resourceSize=(W + 16, H + 8), resourceSizePrev=(W + 16, H + 8)), REBLUR, (2, 2), REBLUR_DS, set(), True),
]


def _build():
    host, _ = native_build._sources()
    deps = host + [SRC] + [os.path.join(d, f) for base in (os.path.join(ROOT, "include"), native_build.CSRC) for d, _, files in os.walk(base) for f in files if f.endswith(".h")]
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(p) for p in deps):
        return
    # the host sources and the program, nothing else: no -lamdhip64, no device code
    r = subprocess.run([CLANG] + FLAGS + native_build.encoding_flags() + host + [SRC, "-o", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _common_settings(overrides):
    kw = dict(viewZScale=1.0, denoisingRange=500.0)
    kw.update(overrides)
    return scene.common_settings(synth.Camera(W, H, FRAME), synth.Camera(W, H, FRAME - 1), W, H, FRAME, **kw)


def test_scan_of_every_family_matches_the_settings_and_runs_clean_under_sanitizers(tmp_path):
    _build()
    lines = []
    for _, mutation, denoisers, overrides, *_ in CASES:
        lines.append("case %d %d %s" % (mutation, len(denoisers), " ".join(str(int(d)) for d, _ in denoisers)))
        lines.append(" ".join([bytes(_common_settings(overrides)).hex()] + [bytes(s).hex() for _, s in denoisers]))
    cases_file = tmp_path / "cases.txt"
    cases_file.write_text("\n".join(lines) + "\n")
    r = subprocess.run([EXE, str(cases_file)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert not [line for line in r.stderr.splitlines() if "Sanitizer" in line or "runtime error" in line], r.stderr[-3000:]  # (-fno-sanitize-recover: a report also ends the program)
    scans = json.loads(r.stdout)
    assert len(scans) == len(CASES)
    for got, (label, mutation, denoisers, overrides, first, cells, named, outside_reblur, mv_written) in zip(scans, CASES):
        cs = _common_settings(overrides)
        if mutation == 1:  # an empty list: the defaults, nothing named
            assert got["num"] == 0 and got["first"] == got["first_with_origin"] == NONE and got["has"] == [0, 0, 0, 0], label
            assert got["rect"] == [0, 0] and got["origin"] == [0, 0] and got["view_z_scale"] == 1.0 and got["cells"] == [2, 2], label
            assert got["named"] == got["read"] == got["written"] == got["slots"] == got["binds_normal_roughness"] == [], label
            continue
        origin = [0, 0] if first == REFERENCE else list(cs.rectOrigin)  # REFERENCE carries no origin
        assert got["first"] == first and got["first_with_origin"] == (NONE if first == REFERENCE else first), label
        families = {REBLUR if int(d) < int(D.RELAX_DIFFUSE) else RELAX if int(d) < int(D.SIGMA_SHADOW) else SIGMA if int(d) < int(D.REFERENCE) else REFERENCE for d, _ in denoisers}
        assert got["has"] == [int(f in families) for f in (REBLUR, RELAX, SIGMA, REFERENCE)], label
        assert set(got["families"]) - {NONE} == families, label
        assert got["rect"] == list(cs.rectSize) == [W, H], label
        assert got["origin"] == origin, label
        if first != REFERENCE:  # (its blocks carry neither: the defaults 1 and 0 stand)
            assert got["view_z_scale"] == cs.viewZScale and got["denoising_range"] == cs.denoisingRange and got["frame_index"] == cs.frameIndex == FRAME, label
        else:
            assert got["view_z_scale"] == 1.0 and got["denoising_range"] == 0.0 and got["frame_index"] == 0, label
        assert got["cells"] == list(cells), label
        assert set(got["named"]) == set(got["slots"]) == {int(t) for t in named} and len(got["slots"]) == len(named), label
        assert set(got["outside_reblur"]) == {int(t) for t in outside_reblur}, label
        inputs, outputs = {int(t) for t in named if t.name.startswith("IN_")}, {int(t) for t in named if t.name.startswith("OUT_")}
        # REBLUR, RELAX and SIGMA read their OUT_ slots back (PostBlur / the a-trous ping-pong write them, TemporalStabilization / the next iteration read them); REFERENCE's
        # copy only writes OUT_SIGNAL
        assert set(got["read"]) == (inputs if first == REFERENCE else inputs | outputs), label
        assert set(got["written"]) == outputs | ({int(RT.IN_MV)} if mv_written else set()), label
        # per dispatch: the tile classification binds no IN_NORMAL_ROUGHNESS (the executor's guide-row rule relies on it), the tap passes of REBLUR and RELAX all do
        assert len(got["binds_normal_roughness"]) == len(got["shaders"]) == got["num"], label
        for shader, family, binds in zip(got["shaders"], got["families"], got["binds_normal_roughness"]):
            if "ClassifyTiles" in shader or family in (NONE, REFERENCE):
                assert binds == 0, (label, shader)
            elif family in (REBLUR, RELAX) and any(k in shader for k in ("_PrePass", "_TemporalAccumulation", "_HistoryFix", "_Blur", "_PostBlur", "_Atrous")):
                assert binds == 1, (label, shader)
        assert sum("ClassifyTiles" in shader for shader in got["shaders"]) == sum(d != D.REFERENCE for d, _ in denoisers), label
        assert 0 <= got["first_block_dispatch"] < got["num"], label
        if mutation >= 2:  # the spoiled block is skipped, the next one of the family taken: same frame, same origin (asserted above)
            assert 0 <= got["mutated_dispatch"] < got["first_block_dispatch"], label
    # the spoiled lists scan like the intact one except for the block they take
    intact, spoiled = scans[1], scans[-2:]
    for s in spoiled:
        assert {k: v for k, v in s.items() if k not in ("first_block_dispatch", "mutated_dispatch")} == {k: v for k, v in intact.items() if k not in ("first_block_dispatch", "mutated_dispatch")}
        assert s["mutated_dispatch"] == intact["first_block_dispatch"]
