"""One entry per field of the public settings structs: how the suite holds that field OFF its default on the device and in the oracle.

    case     the field runs through tests/test_settings_sweep.py at `value`, alone (with the companions it needs to be read at all), in the twins and in the bundles
    held_by  an existing test file already runs it off its default on the device (the fields that change the pass list, the inputs or the frame geometry)
    dead     no pass reads it: the sweep checks that it moves nothing

Keys are "<Struct>.<field>" or "<Struct>.<field>[i]" for the components the API documents one by one; a whole-array entry "<Struct>.<field>" covers every element of
an array that has no per-component entries (the matrices, the sizes). tests/test_settings_sweep.py walks the ctypes structs and fails on a leaf without an entry.

The off-default values are chosen to bind within the five frames of a sweep run (accumulation caps of 1..4, not 30), to stay inside the ranges NRDSettings.h documents,
and -- for sibling fields whose defaults are equal -- to differ from the sibling's value, so that a pass that reads the sibling cannot go unnoticed in the twins."""
from raytracingdenoiser_amd import api

STRUCTS = {"CommonSettings": api.CommonSettings, "ReblurSettings": api.ReblurSettings, "RelaxSettings": api.RelaxSettings, "SigmaSettings": api.SigmaSettings,
           "ReferenceSettings": api.ReferenceSettings}
# the denoiser a one-field case of a family runs on, and the struct that carries the family's settings
BASE = {"REBLUR": "REBLUR_DIFFUSE_SPECULAR", "RELAX": "RELAX_DIFFUSE_SPECULAR", "SIGMA": "SIGMA_SHADOW", "REFERENCE": "REFERENCE"}
STRUCT_OF = {"REBLUR": "ReblurSettings", "RELAX": "RelaxSettings", "SIGMA": "SigmaSettings", "REFERENCE": "ReferenceSettings"}
BUNDLES = ["REBLUR_DIFFUSE_SPECULAR", "REBLUR_DIFFUSE_SPECULAR_SH", "REBLUR_DIFFUSE_SPECULAR_OCCLUSION", "RELAX_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR_SH",
           "SIGMA_SHADOW_TRANSLUCENCY", "REFERENCE"]

ALL3 = ("REBLUR", "RELAX", "SIGMA")
RR = ("REBLUR", "RELAX")  # (SIGMA reads neither the jitter, the frame time, the disocclusion thresholds nor the materials: measured, those move none of its output values)

# companions: what a field needs beside itself to be read by any pass. cs = CommonSettings keywords, settings = denoiser settings, want = extra planes of the frame generator
MATERIALS = dict(want=("materials",))
MIX = dict(cs=dict(isDisocclusionThresholdMixAvailable=True), want=("confidence",))
# (the scene's world-space motion vectors come with motionVectorScale 0; the specular motion written back into IN_MV is divided by that scale: with 0 every modified
# texel is an infinity whatever the thresholds weigh, so these cases scale by 1)
BASECOLOR = dict(cs=dict(isBaseColorMetalnessAvailable=True, motionVectorScale=(1.0, 1.0, 1.0)), want=("basecolor",))
ANTIFIREFLY = dict(settings=dict(enableAntiFirefly=True))
STRAND = dict(cs=dict(strandMaterialID=1.0), want=("materials",))


def case(on, value, companions=None, frames=5):
    return dict(kind="case", on=tuple(on), value=value, companions=companions or {}, frames=frames)


def held_by(path):
    return dict(kind="held_by", path=path)


def dead(reason, values):
    """values: two off-default values, each of which must move nothing"""
    return dict(kind="dead", reason=reason, values=tuple(values))


TABLE = {
    # ------------------------------------------------------------------------------------------------------------------------------------ CommonSettings
    "CommonSettings.viewToClipMatrix": held_by("tests/test_motion_rows.py"),  # (every run of the moving camera; the file re-derives the re-projection from the matrices)
    "CommonSettings.viewToClipMatrixPrev": held_by("tests/test_motion_rows.py"),
    "CommonSettings.worldToViewMatrix": held_by("tests/test_motion_rows.py"),
    "CommonSettings.worldToViewMatrixPrev": held_by("tests/test_motion_rows.py"),
    # a world that itself turned between the frames, 15 degrees about y (column-major, as the other matrices): the temporal passes of REBLUR and RELAX rotate the previous
    # frame's normals with it before they compare them; no SIGMA pass reads it
    "CommonSettings.worldPrevToWorldMatrix": case(RR, (0.96592583, 0.0, -0.25881905, 0.0, 0.0, 1.0, 0.0, 0.0, 0.25881905, 0.0, 0.96592583, 0.0, 0.0, 0.0, 0.0, 1.0)),
    "CommonSettings.motionVectorScale[0]": held_by("tests/test_reblur.py"),
    "CommonSettings.motionVectorScale[1]": held_by("tests/test_reblur.py"),
    "CommonSettings.motionVectorScale[2]": held_by("tests/test_reblur.py"),
    "CommonSettings.cameraJitter[0]": case(RR, 0.3),
    "CommonSettings.cameraJitter[1]": case(RR, -0.2),
    "CommonSettings.cameraJitterPrev[0]": case(RR, -0.1),
    "CommonSettings.cameraJitterPrev[1]": case(RR, 0.25),
    "CommonSettings.resourceSize": held_by("tests/test_dynamic_resolution.py"),
    "CommonSettings.resourceSizePrev": held_by("tests/test_dynamic_resolution.py"),
    "CommonSettings.rectSize": held_by("tests/test_dynamic_resolution.py"),
    "CommonSettings.rectSizePrev": held_by("tests/test_dynamic_resolution.py"),
    "CommonSettings.viewZScale": case(ALL3, 0.5),
    "CommonSettings.timeDeltaBetweenFrames": case(RR, 40.0),
    "CommonSettings.denoisingRange": case(ALL3, 20.0),
    "CommonSettings.disocclusionThreshold": case(RR, 0.003),
    "CommonSettings.disocclusionThresholdAlternate": case(RR, 0.2, MIX),
    "CommonSettings.cameraAttachedReflectionMaterialID": case(RR, 2.0, MATERIALS),
    "CommonSettings.strandMaterialID": case(RR, 1.0, MATERIALS),
    "CommonSettings.strandThickness": case(RR, 0.05, STRAND),
    "CommonSettings.splitScreen": held_by("tests/test_reblur.py"),  # (and switched on and off in mid-sequence: tests/test_sharding.py _scenarios through tests/test_scenarios.py)
    "CommonSettings.printfAt": dead("a shader-printf position: no pass of the library prints", ((3, 5), (40, 17))),
    "CommonSettings.debug": dead("gDebug is written into the constants and read by no pass", (0.5, 1.0)),
    "CommonSettings.rectOrigin": held_by("tests/test_dynamic_resolution.py"),
    "CommonSettings.frameIndex": held_by("tests/test_reference.py"),  # (and every multi-frame parity run, through scene.common_settings: the Poisson rotators, the checkerboard phase)
    "CommonSettings.accumulationMode": held_by("tests/test_sharding.py"),  # (_scenarios, run on one device by tests/test_scenarios.py)
    "CommonSettings.isMotionVectorInWorldSpace": held_by("tests/test_reblur.py"),
    "CommonSettings.isHistoryConfidenceAvailable": held_by("tests/test_reblur.py"),
    "CommonSettings.isDisocclusionThresholdMixAvailable": held_by("tests/test_reblur.py"),
    "CommonSettings.isBaseColorMetalnessAvailable": held_by("tests/test_reblur.py"),
    "CommonSettings.enableValidation": held_by("tests/test_validation.py"),
    # ------------------------------------------------------------------------------------------------------------------------------------ ReblurSettings
    "ReblurSettings.hitDistanceParameters[0]": case(["REBLUR"], 5.0),
    "ReblurSettings.hitDistanceParameters[1]": case(["REBLUR"], 0.3),
    "ReblurSettings.hitDistanceParameters[2]": case(["REBLUR"], 10.0),
    "ReblurSettings.hitDistanceParameters[3]": case(["REBLUR"], -15.0),
    "ReblurSettings.antilagSettings[0]": case(["REBLUR"], 1.0),  # luminanceSigmaScale
    "ReblurSettings.antilagSettings[1]": case(["REBLUR"], 1.5),  # luminanceSensitivity
    "ReblurSettings.maxAccumulatedFrameNum": case(["REBLUR"], 2),
    "ReblurSettings.maxFastAccumulatedFrameNum": case(["REBLUR"], 1),
    "ReblurSettings.maxStabilizedFrameNum": case(["REBLUR"], 2),  # (0 drops the pass: tests/test_reblur.py)
    "ReblurSettings.maxStabilizedFrameNumForHitDistance": dead("gHitDistStabilizationStrength is read by no pass, here or in the reference (Reblur.cpp writes it, no shader names it)", (2, 0)),
    "ReblurSettings.historyFixFrameNum": case(["REBLUR"], 1),
    "ReblurSettings.historyFixBasePixelStride": case(["REBLUR"], 5),
    "ReblurSettings.diffusePrepassBlurRadius": case(["REBLUR"], 12.0),  # (0 drops the pass: tests/test_sharding.py _scenarios)
    "ReblurSettings.specularPrepassBlurRadius": case(["REBLUR"], 20.0),
    "ReblurSettings.minHitDistanceWeight": case(["REBLUR"], 0.3),
    "ReblurSettings.minBlurRadius": case(["REBLUR"], 3.0),
    "ReblurSettings.maxBlurRadius": case(["REBLUR"], 12.0),
    "ReblurSettings.lobeAngleFraction": case(["REBLUR"], 0.4),
    "ReblurSettings.roughnessFraction": case(["REBLUR"], 0.05),
    "ReblurSettings.responsiveAccumulationRoughnessThreshold": case(["REBLUR"], 0.5),
    "ReblurSettings.planeDistanceSensitivity": case(["REBLUR"], 0.1),
    "ReblurSettings.specularProbabilityThresholdsForMvModification[0]": case(["REBLUR"], 0.2, BASECOLOR),
    "ReblurSettings.specularProbabilityThresholdsForMvModification[1]": case(["REBLUR"], 0.6, BASECOLOR),
    "ReblurSettings.fireflySuppressorMinRelativeScale": case(["REBLUR"], 8.0, ANTIFIREFLY),
    "ReblurSettings.checkerboardMode": held_by("tests/test_reblur.py"),
    "ReblurSettings.hitDistanceReconstructionMode": held_by("tests/test_reblur.py"),
    "ReblurSettings.enableAntiFirefly": held_by("tests/test_reblur.py"),
    "ReblurSettings.enablePerformanceMode": held_by("tests/test_reblur.py"),
    "ReblurSettings.minMaterialForDiffuse": case(["REBLUR"], 1.0, MATERIALS),
    "ReblurSettings.minMaterialForSpecular": case(["REBLUR"], 2.0, MATERIALS),
    "ReblurSettings.usePrepassOnlyForSpecularMotionEstimation": case(["REBLUR"], True),
    # ------------------------------------------------------------------------------------------------------------------------------------ RelaxSettings
    "RelaxSettings.antilagSettings[0]": case(["RELAX"], 0.8),  # accelerationAmount
    "RelaxSettings.antilagSettings[1]": case(["RELAX"], 1.5),  # spatialSigmaScale
    "RelaxSettings.antilagSettings[2]": case(["RELAX"], 0.1),  # temporalSigmaScale
    "RelaxSettings.antilagSettings[3]": case(["RELAX"], 0.9),  # resetAmount
    "RelaxSettings.diffuseMaxAccumulatedFrameNum": case(["RELAX"], 2),
    "RelaxSettings.specularMaxAccumulatedFrameNum": case(["RELAX"], 3),
    "RelaxSettings.diffuseMaxFastAccumulatedFrameNum": case(["RELAX"], 1),
    "RelaxSettings.specularMaxFastAccumulatedFrameNum": case(["RELAX"], 2),
    "RelaxSettings.historyFixFrameNum": case(["RELAX"], 1),  # (0 drops the pass: tests/test_relax.py)
    "RelaxSettings.historyFixBasePixelStride": case(["RELAX"], 5),
    "RelaxSettings.historyFixEdgeStoppingNormalPower": case(["RELAX"], 2.0),
    "RelaxSettings.spatialVarianceEstimationHistoryThreshold": case(["RELAX"], 1),
    "RelaxSettings.diffusePrepassBlurRadius": case(["RELAX"], 12.0),
    "RelaxSettings.specularPrepassBlurRadius": case(["RELAX"], 20.0),
    "RelaxSettings.minHitDistanceWeight": case(["RELAX"], 0.3),
    "RelaxSettings.diffusePhiLuminance": case(["RELAX"], 0.5),
    "RelaxSettings.specularPhiLuminance": case(["RELAX"], 3.0),
    "RelaxSettings.lobeAngleFraction": case(["RELAX"], 0.2),
    "RelaxSettings.roughnessFraction": case(["RELAX"], 0.4),
    "RelaxSettings.specularVarianceBoost": case(["RELAX"], 2.0),
    "RelaxSettings.specularLobeAngleSlack": case(["RELAX"], 0.6),
    "RelaxSettings.historyClampingColorBoxSigmaScale": case(["RELAX"], 1.0),
    "RelaxSettings.atrousIterationNum": held_by("tests/test_relax.py"),
    "RelaxSettings.diffuseMinLuminanceWeight": case(["RELAX"], 0.2),
    "RelaxSettings.specularMinLuminanceWeight": case(["RELAX"], 0.4),
    "RelaxSettings.depthThreshold": case(["RELAX"], 0.02),
    "RelaxSettings.confidenceDrivenRelaxationMultiplier": held_by("tests/test_relax.py"),  # (needs the confidence inputs: a binding variant of the a-trous passes)
    "RelaxSettings.confidenceDrivenLuminanceEdgeStoppingRelaxation": held_by("tests/test_relax.py"),
    "RelaxSettings.confidenceDrivenNormalEdgeStoppingRelaxation": held_by("tests/test_relax.py"),
    "RelaxSettings.luminanceEdgeStoppingRelaxation": dead("the reference host writes roughnessEdgeStoppingRelaxation into gLuminanceEdgeStoppingRelaxation (Relax.cpp:156), and so does this one", (0.1, 0.9)),
    "RelaxSettings.normalEdgeStoppingRelaxation": case(["RELAX"], 0.8),
    "RelaxSettings.roughnessEdgeStoppingRelaxation": case(["RELAX"], 0.4),
    "RelaxSettings.checkerboardMode": held_by("tests/test_relax.py"),
    "RelaxSettings.hitDistanceReconstructionMode": held_by("tests/test_relax.py"),
    "RelaxSettings.enableAntiFirefly": held_by("tests/test_relax.py"),
    "RelaxSettings.enableRoughnessEdgeStopping": held_by("tests/test_relax.py"),
    "RelaxSettings.minMaterialForDiffuse": case(["RELAX"], 1.0, MATERIALS),
    "RelaxSettings.minMaterialForSpecular": case(["RELAX"], 2.0, MATERIALS),
    # ------------------------------------------------------------------------------------------------------------------------------------ SigmaSettings
    "SigmaSettings.lightDirection": dead("gLightDirectionView is read only by the world-space sampling branch of SIGMA_Blur.hlsli:176-196, compiled out by SIGMA_USE_SCREEN_SPACE_SAMPLING 1 "
                                         "(SIGMA_Config.hlsli:20, SIGMA_Blur.hlsli:168)", ((0.6, 0.64, -0.48), (0.0, 1.0, 0.0))),
    "SigmaSettings.planeDistanceSensitivity": case(["SIGMA"], 0.2),
    "SigmaSettings.maxStabilizedFrameNum": case(["SIGMA"], 2),  # (0 drops the pass: tests/test_sigma.py)
    # -------------------------------------------------------------------------------------------------------------------------------- ReferenceSettings
    "ReferenceSettings.maxAccumulatedFrameNum": case(["REFERENCE"], 2),
}

# siblings whose defaults are equal, both off the default at DIFFERENT values in one run: a pass that reads the wrong one of the two fails these
TWINS = {
    "reblur_lobe_roughness_fraction": ("REBLUR", ["ReblurSettings.lobeAngleFraction", "ReblurSettings.roughnessFraction"]),
    "relax_max_accumulated": ("RELAX", ["RelaxSettings.diffuseMaxAccumulatedFrameNum", "RelaxSettings.specularMaxAccumulatedFrameNum"]),
    "relax_max_fast_accumulated": ("RELAX", ["RelaxSettings.diffuseMaxFastAccumulatedFrameNum", "RelaxSettings.specularMaxFastAccumulatedFrameNum"]),
    "relax_min_luminance_weight": ("RELAX", ["RelaxSettings.diffuseMinLuminanceWeight", "RelaxSettings.specularMinLuminanceWeight"]),
    "reblur_min_material": ("REBLUR", ["ReblurSettings.minMaterialForDiffuse", "ReblurSettings.minMaterialForSpecular"]),
    "relax_min_material": ("RELAX", ["RelaxSettings.minMaterialForDiffuse", "RelaxSettings.minMaterialForSpecular"]),
    "reblur_special_materials": ("REBLUR", ["CommonSettings.strandMaterialID", "CommonSettings.cameraAttachedReflectionMaterialID"]),
    "relax_special_materials": ("RELAX", ["CommonSettings.strandMaterialID", "CommonSettings.cameraAttachedReflectionMaterialID"]),
}


def leaves(struct_name):
    """every scalar of a settings struct: "<Struct>.<field>" or "<Struct>.<field>[i]" """
    out = []
    for field, ctype in STRUCTS[struct_name]._fields_:
        n = getattr(ctype, "_length_", None)
        out += ["%s.%s" % (struct_name, field)] if n is None else ["%s.%s[%d]" % (struct_name, field, i) for i in range(n)]
    return out


def entry_of(leaf):
    """the table entry that covers a leaf: its own, or the whole-array entry of its field"""
    return TABLE.get(leaf) or TABLE.get(leaf.split("[")[0])


def family_of(name):
    return name if name == "REFERENCE" else name.split("_")[0]


def cases_of(family):
    """the keys of the case entries that run on a family"""
    return [k for k, e in TABLE.items() if e["kind"] == "case" and family in e["on"]]


def _put(target, struct, key, value):
    field, _, index = key.partition("[")
    if index:  # one component of an array field: the others keep the default (or what an earlier key of the same field set)
        cur = list(target.get(field, tuple(getattr(struct(), field))))
        cur[int(index[:-1])] = value
        value = tuple(cur)
    target[field] = value


def build(family, keys, values=None, companions=True):
    """run_parity / run_per_pass arguments of a run with the fields `keys` off their defaults: dict(settings_overrides=, cs_kw=, extra_want=).
    values: {key: value} replaces the table's value (the dead entries); companions=False leaves the companions out."""
    settings, cs, want = {}, {}, []
    for key in keys:
        e = TABLE[key]
        comp = e.get("companions") or {}
        if companions:
            cs.update(comp.get("cs") or {})
            settings.update(comp.get("settings") or {})
            want += [w for w in comp.get("want", ()) if w not in want]
    for key in keys:
        struct_name, _, rest = key.partition(".")
        value = (values or {}).get(key, TABLE[key].get("value"))
        if struct_name == "CommonSettings":
            _put(cs, api.CommonSettings, rest, value)
        else:
            assert struct_name == STRUCT_OF[family], (key, family)
            _put(settings, STRUCTS[struct_name], rest, value)
    return dict(settings_overrides=settings or None, cs_kw=cs or None, extra_want=tuple(want))


def companions_only(family, keys):
    """the same run with every field of `keys` left at its default: what a case is compared against"""
    merged = dict(settings={}, cs={}, want=[])
    for key in keys:
        comp = TABLE[key].get("companions") or {}
        merged["cs"].update(comp.get("cs") or {})
        merged["settings"].update(comp.get("settings") or {})
        merged["want"] += [w for w in comp.get("want", ()) if w not in merged["want"]]
    return dict(settings_overrides=merged["settings"] or None, cs_kw=merged["cs"] or None, extra_want=tuple(merged["want"]))


def bundle(name, mid_sequence=False):
    """every case field of the denoiser's family off its default at once. mid_sequence: only the fields that need no companion -- the companions (anti-firefly, the
    optional inputs) change the pass list or the bindings, and the mid-sequence test keeps the list the same"""
    family = family_of(name)
    keys = [k for k in cases_of(family) if not (mid_sequence and TABLE[k]["companions"])]
    return build(family, keys)
