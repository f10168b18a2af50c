"""Times the front-end pack and back-end resolve kernels (include/NRDHip.h nrdHipPackInputs / nrdHipResolveOutputs) for the REBLUR_DIFFUSE_SPECULAR plane set and holds them
against (c) the same packing done with the torch packers of raytracingdenoiser_amd/synth.py -- the only path there was before the kernels -- and (d) the copy bandwidth the
same device delivers (nrdHipMeasureCopyBandwidth). Device events around `--reps` back-to-back launches after `--warmup` launches; the bytes are counted from the plane formats.
Also records what the compiler made of the kernels (VGPRs, waves per SIMD, scratch, 16-byte loads) from a gfx950 assembly listing (tools/isa_stats.py).
--rejitter adds, in the same run, an SH plane set (REBLUR_SH for both signals in fp16 planes): (a) nrdHipResolveOutputs with resolve = SG, (b) nrdHipResolveOutputsEx with
reJitter = 1 on the same planes, both against the copy rate, (b) once more from --ab-library (a build of the re-jitter form that did not ship:
python tools/build_variant.py rejitter_plain -DNRD_REJITTER_TILE=0), and nrdHipPackInputsEx with checkerboardMode = BLACK on the plane set of `pack`.
--samples [N ...] (default 4) is a run of its own with an output file of its own (profiles/frontend_samples_bench.json): many paths per pixel, REBLUR_RADIANCE on both signals, N sample
layers each. Alternated in one process: (a) nrdHipPackInputsSamples, (b) the best composition there was before it -- torch reductions to the same two single-sample planes (mean for the
radiance and the diffuse hit distance, masked amin for the specular one) followed by nrdHipPackInputs -- and (c) the plain single-sample pack, for scale; with the algorithmic bytes of (a),
its GB/s and its fraction of the copy rate of the same run, and the static facts of the kernel (samples_isa()). The run fails if (a) is slower than (b).
--split is a run of its own that adds the `split` and `isa_split` objects to the output file: the plane set of `pack` held as a tensor host holds it (normal [H, W, 3], roughness [H, W],
two radiance [H, W, 3] and two hit_dist [H, W]); alternated in one process: widen_ms (the frontend.rgba() copies the four-channel path needs), pack_ms (nrdHipPackInputs on the widened
planes), pack_split_ms (nrdHipPackInputsSplit in place), and the same three for resolve ([H, W, 3] outputs against [H, W, 4] outputs + [..., :3].contiguous()); split_isa(): the twins' static facts.
--check-inputs is a run of its own that adds the `check_inputs` and `isa_check_inputs` objects to the output file: nrdHipCheckInputsAsync on the bound REBLUR_DIFFUSE_SPECULAR planes
of raytracingdenoiser_amd/synth.py (28 B per pixel: viewZ 4, IN_MV 8, two signals 8 + 8) against (a) the copy rate of the same run and (b) what a tensor host does today for the same
answer: torch.isfinite over the four planes, masked with the range test, .all(). The run fails if the kernel is slower than (b).
--guides is a run of its own that adds the `guides` and `isa_guides` objects to the output file: nrdHipPackGuides on RGB32_SFLOAT position and positionPrev planes (36 B per pixel
with IN_VIEWZ and IN_MV) against the copy rate of the same run, next to the four shadow-light calls of --shadow-lights on planes of the same size -- streaming kernels of the same
shape, its yardstick; the whole set three times with the rows alternating, each row's spread over the rounds next to its number.
--upsample is a run of its own that adds the `upsample` and `isa_upsample` objects to the output file: quarter-resolution denoising, REBLUR_DIFFUSE_SPECULAR radiance with
remodulation. nrdHipResolveOutputsUpsampled from 1280 x 720 planes to 2560 x 1440 against the plain resolve of the same configuration at 2560 x 1440 and the copy rate, five
alternating rounds, medians; and whole frames (pack + denoise + resolve, default settings) at full size and at quarter resolution.
--lobes is a run of its own that adds the `lobes` and `isa_lobes` objects to the output file: the probabilistic diffuse / specular split at 2560 x 1440, REBLUR_RADIANCE on both
signals, one traced plane, a lobe byte and a probability per pixel. Five alternating rounds of (a) nrdHipPackInputsLobes, (b) nrdHipPackInputs producing the same outputs from two
prepared RGBA32_SFLOAT planes, (c) the torch chain that prepares those planes, (d) nrdHipCheckHitDistCoverage with area 2 on both packed signals; the copy rate of the same run,
each row's spread over the rounds, and whether (a) is slower than (b) by more than that spread.
--direct is a run of its own that adds the `direct` and `isa_direct` objects to the output file (--isa-only: the second one alone, without a GPU): combined direct and indirect
lighting at 2560 x 1440, REBLUR_RADIANCE on both signals, RGBA32_SFLOAT planes. Five alternating rounds of (a) nrdHipPackInputsDirect, (b) what a host writes today -- the torch
composition of the README's rule (sum, two luminances, ratio, clamp, lerp, where) into two RGBA32_SFLOAT planes followed by nrdHipPackInputs -- and the two halves of (b) alone;
the fused call's bytes per pixel and its fraction of the copy rate of the same run. The run fails if (a) is slower than (b).
usage: python tools/frontend_bench.py [--width 2560 --height 1440 --reps 300 --warmup 20] [--out profiles/frontend_bench.json] [--isa-only] [--rejitter [--ab-library PATH]] [--samples [N ...]] [--split]
       [--check-inputs] [--shadow-lights] [--guides] [--upsample] [--lobes] [--direct]"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import isa_stats  # noqa: E402
from raytracingdenoiser_amd import build as B  # noqa: E402

SRC = os.path.join(B.CSRC, "hip", "kernels_frontend.hip")
# bytes per pixel of the timed plane sets, from the formats
PACK_READ = {"normal_roughness RGBA32_SFLOAT": 16, "viewZ R32_SFLOAT": 4, "motion RGBA32_SFLOAT": 16, "diffuse radiance_hitdist RGBA32_SFLOAT": 16, "specular radiance_hitdist RGBA32_SFLOAT": 16}
PACK_WRITE = {"IN_NORMAL_ROUGHNESS": 4, "IN_VIEWZ R32_SFLOAT": 4, "IN_MV RGBA16_SFLOAT": 8, "IN_DIFF_RADIANCE_HITDIST RGBA16_SFLOAT": 8, "IN_SPEC_RADIANCE_HITDIST RGBA16_SFLOAT": 8}
RESOLVE_READ = {"OUT_DIFF_RADIANCE_HITDIST RGBA16_SFLOAT": 8, "OUT_SPEC_RADIANCE_HITDIST RGBA16_SFLOAT": 8, "IN_NORMAL_ROUGHNESS": 4, "IN_VIEWZ R32_SFLOAT": 4}
RESOLVE_WRITE = {"diffuse RGBA32_SFLOAT": 16, "specular RGBA32_SFLOAT": 16}
SH_RESOLVE_READ = {"OUT_DIFF_SH0 RGBA16_SFLOAT": 8, "OUT_DIFF_SH1 RGBA16_SFLOAT": 8, "OUT_SPEC_SH0 RGBA16_SFLOAT": 8, "OUT_SPEC_SH1 RGBA16_SFLOAT": 8, "IN_NORMAL_ROUGHNESS": 4, "IN_VIEWZ R32_SFLOAT": 4}
REJITTER_READ = dict(SH_RESOLVE_READ, **{"rf0 RGBA32_SFLOAT": 16})  # (the four neighbour texels of IN_NORMAL_ROUGHNESS / IN_VIEWZ are other lanes' own texels: counted once)


def isa():
    """static facts about the two kernels from a gfx950 listing of the translation unit, compiled with the product's flags"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_frontend.s")
        flags = [f for f in B._flags(SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    out = {}
    for mangled, s in stats.items():
        name = "pack" if "PackInputsKernel" in mangled else "resolve" if "ResolveOutputsKernel" in mangled else None
        if name:
            c = s["counter"]
            out[name] = {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                         "global_load_dwordx4": c.get("global_load_dwordx4", 0), "global_load_dwordx2": c.get("global_load_dwordx2", 0), "global_store_dwordx4": c.get("global_store_dwordx4", 0),
                         "global_store_dwordx2": c.get("global_store_dwordx2", 0), "v_div_scale_f32": c.get("v_div_scale_f32", 0), "transcendental": s["trans"]}
    assert set(out) == {"pack", "resolve"}, list(stats)
    return out


def _facts(s):
    c = s["counter"]
    return {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
            "ds_read_b128": c.get("ds_read_b128", 0), "ds_write_b128": c.get("ds_write_b128", 0), "v_div_scale_f32": c.get("v_div_scale_f32", 0), "transcendental": s["trans"]}


def options_isa(extra=()):
    """static facts about the kernels behind nrdHipResolveOutputsEx / nrdHipPackInputsEx (the `isa_options` object of profiles/frontend_bench.json), as isa(): "rejitter"
    and "pack_checkerboard"; extra: further compiler flags (-DNRD_REJITTER_TILE=0: the form without the LDS tile). rejitter also holds the tile its source declares."""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_frontend.s")
        flags = [f for f in B._flags(SRC) if f not in ("-x", "hip")] + list(extra)
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    out = {}
    for mangled, s in stats.items():
        name = "rejitter" if "ReJitterKernel" in mangled else "pack_checkerboard" if "PackCheckerboardKernel" in mangled else None
        if name:
            out[name] = _facts(s)
    assert set(out) == {"rejitter", "pack_checkerboard"}, list(stats)
    tile = re.search(r"constexpr int kReJitterTileW = (\d+), kReJitterTileH = (\d+);", open(SRC).read())
    out["rejitter"]["declared_tile_bytes"] = (int(tile.group(1)) + 2) * (int(tile.group(2)) + 2) * 16
    return out


def _loop_loads(body):
    """{instruction: count} of the vector-memory loads inside the loops of one kernel of a listing: the instructions between a label and a later branch back to it"""
    lines = body.split("\n")
    label_at = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    inside = set()
    for i, l in enumerate(lines):
        m = re.match(r"\ts_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and label_at.get(m.group(1), i) < i:
            inside.update(range(label_at[m.group(1)], i))
    out = {}
    for i in sorted(inside):
        ins = lines[i].strip().split()[0] if lines[i].startswith("\t") and lines[i].strip() else ""
        if ins.startswith(("global_load", "buffer_load", "flat_load", "scratch_load")):
            out[ins] = out.get(ins, 0) + 1
    return out


def samples_isa():
    """static facts about the two instantiations of the kernel behind nrdHipPackInputsSamples (the `isa_samples` object of profiles/frontend_samples_bench.json), as isa():
    "pack_samples" and "pack_samples_checkerboard"; sample_loop_loads: the loads inside the kernel's loops -- the sample loops are its only ones"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_frontend.s")
        flags = [f for f in B._flags(SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
        txt = open(listing).read()
    out = {}
    for mangled, s in stats.items():
        if "PackSamplesKernel" not in mangled:
            continue
        name = "pack_samples_checkerboard" if "ILb1E" in mangled else "pack_samples"
        c = s["counter"]
        body = txt[txt.index("\n" + mangled + ":"):].split(".Lfunc_end")[0]
        out[name] = {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                     "global_load_dwordx4": c.get("global_load_dwordx4", 0), "v_div_scale_f32": c.get("v_div_scale_f32", 0), "transcendental": s["trans"],
                     "sample_loop_loads": _loop_loads(body)}
    assert set(out) == {"pack_samples", "pack_samples_checkerboard"}, list(stats)
    return out


SPLIT_KERNELS = {"PackInputsSplitKernel": "pack_split", "PackCheckerboardSplitKernel": "pack_checkerboard_split", "ResolveOutputsSplitKernel": "resolve_split", "ReJitterSplitKernel": "rejitter_split"}


def split_isa():
    """static facts about the split twins behind nrdHipPackInputsSplit / nrdHipResolveOutputsSplit (the `isa_split` object of profiles/frontend_bench.json), as isa(): VGPRs, waves per
    SIMD, scratch, LDS and the 12- and 16-byte accesses of "pack_split", "pack_checkerboard_split", "pack_samples_split", "pack_samples_checkerboard_split", "resolve_split" and
    "rejitter_split"; sibling_*: the same facts of the kernel each is a twin of; the samples twins also hold the loads inside their sample loops"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_frontend.s")
        flags = [f for f in B._flags(SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
        txt = open(listing).read()

    def facts(s):
        c = s["counter"]
        return {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                "global_load_dwordx3": c.get("global_load_dwordx3", 0), "global_load_dwordx4": c.get("global_load_dwordx4", 0), "global_load_dword": c.get("global_load_dword", 0),
                "global_store_dwordx3": c.get("global_store_dwordx3", 0), "global_store_dwordx4": c.get("global_store_dwordx4", 0)}

    def name_of(mangled):
        if "PackSamplesSplitKernel" in mangled or "PackSamplesKernel" in mangled:
            return "pack_samples" + ("_checkerboard" if "ILb1E" in mangled else "") + ("_split" if "Split" in mangled else "")
        for kernel, name in SPLIT_KERNELS.items():
            if kernel in mangled:
                return name
            if kernel.replace("Split", "") in mangled:
                return name[:-len("_split")]
        return None

    named = {name_of(m): (m, s) for m, s in stats.items() if name_of(m)}
    out = {}
    for name, (mangled, s) in named.items():
        if not name.endswith("_split"):
            continue
        out[name] = facts(s)
        sibling = facts(named[name[:-len("_split")]][1])
        out[name].update({"sibling_vgprs": sibling["vgprs"], "sibling_waves_per_simd": sibling["waves_per_simd"]})
        if "samples" in name:
            out[name]["sample_loop_loads"] = _loop_loads(txt[txt.index("\n" + mangled + ":"):].split(".Lfunc_end")[0])
    assert len(out) == 6, list(stats)
    return out


def samples_main(args):
    """--samples: see the module text"""
    result = {"isa_samples": samples_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    g = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    n = rand(h, w, 3) * 2.0 - 1.0
    n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    nr = torch.cat([n, rand(h, w, 1)], -1).contiguous()
    viewz, material, motion = 0.5 + rand(h, w) * 100.0, torch.floor(rand(h, w) * 4.0), rand(h, w, 4) - 0.5
    lib = api.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mode = frontend.SignalMode.REBLUR_RADIANCE
    scale = torch.tensor([4.0, 3.0, 5.0, 30.0], device="cuda")
    gbuffer_read = {"normal_roughness RGBA32_SFLOAT": 16, "viewZ R32_SFLOAT": 4, "materialID R32_SFLOAT": 4, "motion RGBA32_SFLOAT": 16}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    result.update({"device": torch.cuda.get_device_name(0), "width": w, "height": h, "reps": args.reps, "warmup": args.warmup, "copy_gigabytes_per_second": gbps.value,
                   "planes": "REBLUR_RADIANCE on both signals, N sample layers each ([N, H, W, 4] fp32), normal + roughness, viewZ, materialID, motion",
                   "times_are": "device events around --reps back-to-back calls, per call, the best of two alternated rounds", "samples": {}})
    slower = []
    for count in args.samples:
        diff, spec = rand(count, h, w, 4) * scale, rand(count, h, w, 4) * scale
        spec[..., 3] *= (rand(count, h, w) > 0.25)  # a quarter of the specular paths miss: hit distance 0
        sig = lambda t: dict(mode=mode, radiance_hitdist=t)
        packed, desc, keep = frontend.describe_pack(nr, viewz, material_id=material, motion=motion, diffuse=sig(diff), specular=sig(spec))
        samples = frontend.pack_samples(sig(diff), sig(spec))
        one_diff, one_spec = torch.empty(h, w, 4, device="cuda"), torch.empty(h, w, 4, device="cuda")
        _, desc_one, keep_one = frontend.describe_pack(nr, viewz, material_id=material, motion=motion, diffuse=sig(one_diff), specular=sig(one_spec), out=packed)
        inf = torch.tensor(float("inf"), device="cuda")
        zero = torch.zeros((), device="cuda")

        def new_call():
            assert lib.nrdHipPackInputsSamples(C.byref(desc), None, C.byref(samples), stream) == 0

        def composition():
            torch.mean(diff, dim=0, out=one_diff)
            torch.mean(spec, dim=0, out=one_spec)
            hit = spec[..., 3]
            smallest = torch.where(hit == 0, inf, hit).amin(0)
            one_spec[..., 3] = torch.where(smallest == inf, zero, smallest)
            assert lib.nrdHipPackInputs(C.byref(desc_one), stream) == 0

        def plain():
            assert lib.nrdHipPackInputs(C.byref(desc_one), stream) == 0

        rounds = [{"samples_ms": timed(new_call), "torch_reduce_then_pack_ms": timed(composition), "plain_pack_ms": timed(plain)} for _ in range(2)]
        best = {k: min(r[k] for r in rounds) for k in rounds[0]}
        read = dict(gbuffer_read, **{"diffuse radiance_hitdist RGBA32_SFLOAT x N": 16 * count, "specular radiance_hitdist RGBA32_SFLOAT x N": 16 * count})
        write_bytes = sum(t.numel() * t.element_size() for t, fmt in packed.values()) // px  # counted from the planes the call writes
        total = sum(read.values()) + write_bytes
        rate = total * px / (best["samples_ms"] * 1e-3) / 1e9
        result["samples"][str(count)] = dict(best, rounds=rounds, read_bytes_per_pixel=read, write_bytes_per_pixel=write_bytes, bytes_per_pixel=total, gigabytes_per_second=rate,
                                             fraction_of_copy_rate=rate / gbps.value, samples_over_torch_reduce_then_pack=best["samples_ms"] / best["torch_reduce_then_pack_ms"],
                                             samples_over_plain_pack=best["samples_ms"] / best["plain_pack_ms"])
        if best["samples_ms"] > best["torch_reduce_then_pack_ms"]:
            slower.append(count)
        del diff, spec, one_diff, one_spec, packed, keep, keep_one
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.samples_out), exist_ok=True)
    with open(args.samples_out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "isa_samples"}))
    assert not slower, "nrdHipPackInputsSamples is slower than torch reductions + nrdHipPackInputs at N = %s: the kernel is not finished" % slower


def split_main(args):
    """--split: see the module text"""
    result = {"isa_split": split_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    g = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    normal = rand(h, w, 3) * 2.0 - 1.0
    normal = (normal / normal.norm(dim=-1, keepdim=True).clamp_min(1e-6)).contiguous()
    scale = torch.tensor([4.0, 3.0, 5.0], device="cuda")
    # held the way synth.render_frame(want=("raw",)) holds it
    raw = {"normal": normal, "roughness": rand(h, w), "material": torch.floor(rand(h, w) * 4.0), "viewz": 0.5 + rand(h, w) * 100.0, "motion": rand(h, w, 4) - 0.5,
           "diff_radiance": rand(h, w, 3) * scale, "diff_hit_dist": rand(h, w) * 30.0, "spec_radiance": rand(h, w, 3) * scale, "spec_hit_dist": rand(h, w) * 30.0}
    mode = frontend.SignalMode.REBLUR_RADIANCE
    lib = api.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def widen():  # the copies the four-channel path needs for these planes: three allocations, six strided copies
        return frontend.rgba(raw["normal"], raw["roughness"]), frontend.rgba(raw["diff_radiance"], raw["diff_hit_dist"]), frontend.rgba(raw["spec_radiance"], raw["spec_hit_dist"])

    nr4, diff4, spec4 = widen()
    gbuffer = dict(material_id=raw["material"], motion=raw["motion"])
    packed, desc4, keep4 = frontend.describe_pack(nr4, raw["viewz"], diffuse=dict(mode=mode, radiance_hitdist=diff4), specular=dict(mode=mode, radiance_hitdist=spec4), **gbuffer)
    pairs = dict(diffuse=dict(mode=mode, radiance_hitdist=(raw["diff_radiance"], raw["diff_hit_dist"])), specular=dict(mode=mode, radiance_hitdist=(raw["spec_radiance"], raw["spec_hit_dist"])))
    packed3, desc3, keep3 = frontend.describe_pack((raw["normal"], raw["roughness"]), raw["viewz"], in_place=True, **pairs, **gbuffer)
    split = frontend.pack_split((raw["normal"], raw["roughness"]), **pairs)

    def pack():
        assert lib.nrdHipPackInputs(C.byref(desc4), stream) == 0

    def pack_split():
        assert lib.nrdHipPackInputsSplit(C.byref(desc3), None, None, C.byref(split), stream) == 0

    pack(), pack_split()
    torch.cuda.synchronize()
    for rt in packed:  # the same bytes, or the times below compare nothing
        assert torch.equal(packed[rt][0].view(torch.uint8), packed3[rt][0].view(torch.uint8)), rt
    R = api.ResourceType
    resolve_args = dict(diffuse=dict(mode=mode, in0=packed[R.IN_DIFF_RADIANCE_HITDIST][0]), specular=dict(mode=mode, in0=packed[R.IN_SPEC_RADIANCE_HITDIST][0]),
                        normal_roughness=packed[R.IN_NORMAL_ROUGHNESS][0], viewz=packed[R.IN_VIEWZ][0], denormalize_hit_dist=True)
    resolved4, rdesc4, rkeep4 = frontend.describe_resolve(**resolve_args)
    resolved3, rdesc3, rkeep3 = frontend.describe_resolve(channels=3, **resolve_args)
    rsplit = frontend.resolve_split(resolved3)

    def resolve():
        assert lib.nrdHipResolveOutputs(C.byref(rdesc4), stream) == 0

    def narrow():  # what a caller of the four-channel call does to hold [H, W, 3]
        return resolved4["diffuse"][..., :3].contiguous(), resolved4["specular"][..., :3].contiguous()

    def resolve_split():
        assert lib.nrdHipResolveOutputsSplit(C.byref(rdesc3), None, C.byref(rsplit), stream) == 0

    resolve(), resolve_split()
    torch.cuda.synchronize()
    for name in ("diffuse", "specular"):
        assert torch.equal(resolved4[name][..., :3].contiguous().view(torch.uint8), resolved3[name].view(torch.uint8)), name

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    calls = {"widen_ms": widen, "pack_ms": pack, "pack_split_ms": pack_split, "narrow_ms": narrow, "resolve_ms": resolve, "resolve_split_ms": resolve_split}
    rounds = [{k: timed(fn) for k, fn in calls.items()} for _ in range(2)]  # alternated twice: the spread between the rounds says how much a difference means
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    spread = {k: abs(rounds[0][k] - rounds[1][k]) for k in rounds[0]}
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    pack_bytes, resolve4_bytes = sum(PACK_READ.values()) + sum(PACK_WRITE.values()), sum(RESOLVE_READ.values()) + sum(RESOLVE_WRITE.values())
    resolve3_bytes = sum(RESOLVE_READ.values()) + 24
    rate = lambda bytes_per_px, ms: bytes_per_px * px / (ms * 1e-3) / 1e9
    baseline, margin = best["widen_ms"] + best["pack_ms"], spread["widen_ms"] + spread["pack_ms"] + spread["pack_split_ms"]
    ratio, ratio_spread = best["pack_split_ms"] / best["pack_ms"], (spread["pack_split_ms"] + spread["pack_ms"]) / best["pack_ms"]
    result["split"] = dict(
        best, rounds=rounds, spread_between_rounds_ms=spread, device=torch.cuda.get_device_name(0), width=w, height=h, reps=args.reps, warmup=args.warmup,
        planes="the plane set of `pack`, held as synth's raw holds it: normal [H, W, 3] + roughness [H, W], two radiance [H, W, 3] + hit_dist [H, W], viewz, material, motion [H, W, 4]",
        widen_is="frontend.rgba() for normal + roughness and the two radiance + hit distance pairs: three allocations, six strided copies -- what the four-channel path costs such a caller",
        narrow_is="[..., :3].contiguous() of the two [H, W, 4] outputs", widen_plus_pack_ms=baseline, pack_split_over_widen_plus_pack=best["pack_split_ms"] / baseline,
        pack_split_over_pack=ratio, pack_split_over_pack_spread=ratio_spread, in_place_is_no_slower=bool(best["pack_split_ms"] <= baseline + margin),
        narrow_plus_resolve_ms=best["narrow_ms"] + best["resolve_ms"], resolve_split_over_narrow_plus_resolve=best["resolve_split_ms"] / (best["narrow_ms"] + best["resolve_ms"]),
        resolve_split_over_resolve=best["resolve_split_ms"] / best["resolve_ms"], pack_bytes_per_pixel=pack_bytes, resolve_bytes_per_pixel=resolve4_bytes,
        resolve_split_bytes_per_pixel=resolve3_bytes, copy_gigabytes_per_second=gbps.value, pack_split_fraction_of_copy_rate=rate(pack_bytes, best["pack_split_ms"]) / gbps.value,
        resolve_split_fraction_of_copy_rate=rate(resolve3_bytes, best["resolve_split_ms"]) / gbps.value,
        times_are="device events around --reps back-to-back calls, per call, the best of two alternated rounds",
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)")
    record = {}
    if os.path.exists(args.out):  # the other fields of the record are another run's: kept as they are
        with open(args.out) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")
    print(json.dumps({k: v for k, v in result["split"].items() if k != "rounds"}))


CHECK_SRC = os.path.join(B.CSRC, "hip", "kernels_check_inputs.hip")
CHECK_READ = {"IN_VIEWZ R32_SFLOAT": 4, "IN_MV RGBA16_SFLOAT": 8, "IN_DIFF_RADIANCE_HITDIST RGBA16_SFLOAT": 8, "IN_SPEC_RADIANCE_HITDIST RGBA16_SFLOAT": 8}


def check_inputs_isa():
    """static facts about the kernel behind nrdHipCheckInputs (the `isa_check_inputs` object of profiles/frontend_bench.json), as isa(), per instantiation ("planes_<mask>";
    "diffuse_specular" = the one the measurement runs); atomics: the global atomics of the listing -- all of them sit behind the wave's exit"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_check_inputs.s")
        flags = [f for f in B._flags(CHECK_SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", CHECK_SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    out = {}
    for mangled, s in stats.items():
        m = re.search(r"CheckInputsKernelILj(\d+)E", mangled)
        if not m:
            continue
        c = s["counter"]
        facts = {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                 "global_load_dword": c.get("global_load_dword", 0), "global_load_dwordx2": c.get("global_load_dwordx2", 0),
                 "atomics": {k: v for k, v in c.items() if k.startswith("global_atomic")}}
        out["planes_%s" % m.group(1)] = facts
        if int(m.group(1)) == 23:  # viewZ, IN_MV, diffuse and specular radiance: the plane set of the measurement
            out["diffuse_specular"] = facts
    assert "diffuse_specular" in out and len(out) == 11, list(stats)
    return out


def check_inputs_main(args):
    """--check-inputs: see the module text"""
    result = {"isa_check_inputs": check_inputs_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, scene, synth
    from raytracingdenoiser_amd.executor import HipExecutor

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    name = "REBLUR_DIFFUSE_SPECULAR"
    frames = [synth.render_frame(w, h, f, device="cuda", want=tuple(scene.DENOISERS[name][1])) for f in range(2)]
    inst = api.Instance([(0, scene.DENOISERS[name][0])])
    ex = HipExecutor(inst, w, h)
    for rt, t, fmt in scene.user_planes(name, frames[1]):
        ex.bind(rt, t.contiguous(), fmt)
    cs = scene.common_settings(frames[1]["camera"], frames[0]["camera"], w, h, 1)
    assert inst.set_denoiser_settings(0, scene.denoiser_settings(name, frames[1], None)) == api.Result.SUCCESS and inst.set_common_settings(cs) == api.Result.SUCCESS
    r, ptr, n = inst.get_compute_dispatches_raw()
    assert r == api.Result.SUCCESS
    lib, stream = inst.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    report = torch.zeros(18, dtype=torch.int32, device="cuda")
    mask, raw_ptr, raw_report = C.c_uint32(), C.cast(ptr, C.c_void_p), C.c_void_p(report.data_ptr())

    def kernel():
        assert lib.nrdHipCheckInputsAsync(ex.handle, raw_ptr, n, raw_report, C.byref(mask)) == 0

    viewz, mv, diff, spec = (ex._bound[int(rt)] for rt in (api.ResourceType.IN_VIEWZ, api.ResourceType.IN_MV, api.ResourceType.IN_DIFF_RADIANCE_HITDIST, api.ResourceType.IN_SPEC_RADIANCE_HITDIST))
    denoising_range, scale = float(cs.denoisingRange), float(cs.viewZScale)

    def torch_host():  # the same yes / no without the rect origin, the checkerboard, the counts and the positions: four reductions, one answer left on the device
        sky = ((viewz * scale).abs() > denoising_range).unsqueeze(-1)
        return (torch.isfinite(viewz).all() & torch.isfinite(mv[..., :3]).all() & (torch.isfinite(diff) | sky).all() & (torch.isfinite(spec) | sky).all())

    kernel()
    torch.cuda.synchronize()
    words = report.cpu().numpy().view("uint32")
    assert mask.value == 0x3F and int(words[0]) == px and 0 < int(words[1]) < px and not words[2:10].any() and bool(torch_host()), words  # a clean frame, for both

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    rounds = [{"check_inputs_ms": timed(kernel), "torch_isfinite_ms": timed(torch_host)} for _ in range(2)]
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    bytes_per_px = sum(CHECK_READ.values())
    rate = bytes_per_px * px / (best["check_inputs_ms"] * 1e-3) / 1e9
    result["check_inputs"] = dict(
        best, rounds=rounds, device=torch.cuda.get_device_name(0), width=w, height=h, reps=args.reps, warmup=args.warmup, in_range_pixels=int(words[1]), pixels=px,
        planes="the bound REBLUR_DIFFUSE_SPECULAR inputs of synth.render_frame, frame 1: IN_VIEWZ, IN_MV, IN_DIFF_RADIANCE_HITDIST, IN_SPEC_RADIANCE_HITDIST",
        torch_isfinite_is="torch.isfinite over the four planes, the noisy ones masked with the range test, .all() of each, the four answers ANDed on the device; no rect origin, no "
                          "checkerboard, no counts, no positions", read_bytes_per_pixel=CHECK_READ, bytes_per_pixel=bytes_per_px,
        bytes_are="what the kernel loads: every texel of the four planes inside the rect, the noisy texels of sky pixels included (they are masked, not skipped)", gigabytes_per_second=rate, copy_gigabytes_per_second=gbps.value,
        fraction_of_copy_rate=rate / gbps.value, check_inputs_over_torch_isfinite=best["check_inputs_ms"] / best["torch_isfinite_ms"],
        times_are="device events around --reps back-to-back calls (each call: two 40- / 32-byte memsets and the kernel), per call, the best of two alternated rounds",
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)")
    record = {}
    if os.path.exists(args.out):  # the other fields of the record are another run's: kept as they are
        with open(args.out) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")
    print(json.dumps({k: v for k, v in result["check_inputs"].items() if k != "rounds"}))
    print(json.dumps(result["isa_check_inputs"]["diffuse_specular"]))
    assert best["check_inputs_ms"] <= best["torch_isfinite_ms"], "nrdHipCheckInputs is slower than the torch.isfinite chain it replaces: the kernel is not finished"


LIGHTS_SRC = os.path.join(B.CSRC, "hip", "kernels_shadow_lights.hip")
LIGHTS_KERNELS = {"PackLightsPerLightKernel": "pack_per_light", "PackLightsCombinedKernel": "pack_combined", "ResolveLightsPerLightKernel": "resolve_per_light",
                  "ResolveLightsCombinedKernel": "resolve_combined"}


def shadow_lights_isa():
    """static facts about the four kernels behind nrdHipPackShadowLights / nrdHipResolveShadowLights (the `isa_shadow_lights` object of profiles/frontend_bench.json), as isa()"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_shadow_lights.s")
        flags = [f for f in B._flags(LIGHTS_SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", LIGHTS_SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    out = {}
    for mangled, s in stats.items():
        for kernel, name in LIGHTS_KERNELS.items():
            if kernel in mangled:
                c = s["counter"]
                out[name] = {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                             "v_div_scale_f32": c.get("v_div_scale_f32", 0), "transcendental": s["trans"]}
    assert set(out) == set(LIGHTS_KERNELS.values()), list(stats)
    return out


def _shadow_light_planes(torch, api, frontend, w, h):
    """the planes and descriptors of the four timed shadow-light calls (four LOCAL lights, 40 % of the texels lit), and the bytes each moves per pixel, from the formats"""
    n = 4
    g = torch.Generator(device="cuda").manual_seed(17)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    sizes = [0.5, 1.0, 2.0, 4.0]
    lights = [(api.LightType.LOCAL, v) for v in sizes]
    d = 0.05 + 20.0 * rand(n, h, w)
    d[rand(n, h, w) < 0.4] = 1e5  # lit
    dl = d + 1.0 + 30.0 * rand(n, h, w)
    lighting = (4.0 * rand(n, h, w, 4)).contiguous()
    PL, CO = api.ShadowsMode.PER_LIGHT, api.ShadowsMode.COMBINED
    per_res, per_desc, keep0 = frontend.describe_pack_shadow_lights(lights, d, distance_to_light=dl, mode=PL)
    com_res, com_desc, keep1 = frontend.describe_pack_shadow_lights(lights, d, distance_to_light=dl, lighting=lighting, mode=CO)
    shadows = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    shadow4 = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda", generator=g)
    lsum = com_res["lighting_sum"][0]
    out_a, rdesc_a, _ = frontend.describe_resolve_shadow_lights(shadows, lighting, mode=PL)
    out_b, rdesc_b, _ = frontend.describe_resolve_shadow_lights(shadow4, lsum, mode=CO, lights_num=n)
    bytes_per_px = {"pack_per_light": n * (4 + 4) + n * 2, "pack_combined": n * (4 + 4 + 16) + 2 + 4 + 16, "resolve_per_light": n * (1 + 16) + 16, "resolve_combined": 4 + 16 + 16}
    return dict(n=n, sizes=sizes, d=d, dl=dl, lighting=lighting, shadows=shadows, shadow4=shadow4, lsum=lsum, per_res=per_res, per_desc=per_desc, com_res=com_res, com_desc=com_desc,
                out_a=out_a, rdesc_a=rdesc_a, out_b=out_b, rdesc_b=rdesc_b, keep=[keep0, keep1], bytes_per_px=bytes_per_px)


def shadow_lights_main(args):
    """--shadow-lights: nrdHipPackShadowLights (PER_LIGHT and COMBINED) and nrdHipResolveShadowLights (both modes) for four local lights at SIGMA's baseline size against the
    copy rate of the same process and against the same recipes written as torch elementwise operations -- all the parent commit offers a host without kernels"""
    result = {"isa_shadow_lights": shadow_lights_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    lib, stream = api.load_library(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = _shadow_light_planes(torch, api, frontend, w, h)
    n, sizes, d, dl, lighting, shadows, shadow4, lsum = t["n"], t["sizes"], t["d"], t["dl"], t["lighting"], t["shadows"], t["shadow4"], t["lsum"]
    per_res, per_desc, com_desc, out_a, rdesc_a, out_b, rdesc_b = t["per_res"], t["per_desc"], t["com_desc"], t["out_a"], t["rdesc_a"], t["out_b"], t["rdesc_b"]

    def call(fn, desc):
        def f():
            assert fn(C.byref(desc), stream) == 0
        return f

    fp16_max, eps = 65504.0, 1e-6

    def penumbra(i):
        r = (sizes[i] * d[i] / (dl[i] - d[i]).clamp_min(eps)) * 0.5
        return torch.where(d[i] >= fp16_max, fp16_max, r.clamp_max(32768.0))

    def torch_pack_per_light():
        return torch.stack([penumbra(i) for i in range(n)]).half()

    def torch_pack_combined():
        Lsum, LSsum = torch.zeros(h, w, 3, device="cuda"), torch.zeros(h, w, 3, device="cuda")
        Wsum, Psum, dmin = torch.zeros(h, w, device="cuda"), torch.zeros(h, w, device="cuda"), torch.full((h, w), float("inf"), device="cuda")
        for i in range(n):
            L = lighting[i, ..., :3]
            lit = d[i] >= fp16_max
            Lsum = Lsum + L
            LSsum = LSsum + L * lit.unsqueeze(-1)
            wgt = (~lit) * (L[..., 0] * 0.2126 + L[..., 1] * 0.7152 + L[..., 2] * 0.0722)
            Wsum, Psum, dmin = Wsum + wgt, Psum + penumbra(i) * wgt, torch.minimum(dmin, d[i])
        tr = torch.cat([(dmin >= fp16_max).float().unsqueeze(-1), (LSsum / Lsum.clamp_min(eps)).clamp(0.0, 1.0)], -1)
        return (torch.where(dmin >= fp16_max, fp16_max, Psum / Wsum.clamp_min(eps)).half(), torch.floor(tr * 255.0 + 0.5).to(torch.uint8),
                torch.cat([Lsum, torch.zeros(h, w, 1, device="cuda")], -1))

    def torch_resolve_per_light():
        acc = torch.zeros(h, w, 3, device="cuda")
        for i in range(n):
            s = shadows[i].float() / 255.0
            acc = acc + lighting[i, ..., :3] * (s * s).unsqueeze(-1)
        return torch.cat([acc, torch.zeros(h, w, 1, device="cuda")], -1)

    def torch_resolve_combined():
        s = shadow4.float() / 255.0
        s = s * s
        return torch.cat([lsum[..., :3] * s[..., 1:], s[..., :1]], -1)

    calls = {"pack_per_light": (call(lib.nrdHipPackShadowLights, per_desc), torch_pack_per_light), "pack_combined": (call(lib.nrdHipPackShadowLights, com_desc), torch_pack_combined),
             "resolve_per_light": (call(lib.nrdHipResolveShadowLights, rdesc_a), torch_resolve_per_light), "resolve_combined": (call(lib.nrdHipResolveShadowLights, rdesc_b), torch_resolve_combined)}
    # the two forms of each recipe agree (the torch chain is not held to the bits: it is timed, not tested)
    for name, (kernel, chain) in calls.items():
        kernel()
    torch.cuda.synchronize()
    chain = torch_pack_per_light().float()
    assert bool(((per_res[api.ResourceType.IN_PENUMBRA][0].float() - chain).abs() <= chain * 2.0 ** -10).all())  # one fp16 step of the value at the most
    assert float((out_a - torch_resolve_per_light()).abs().max()) <= 1e-3 and float((out_b - torch_resolve_combined()).abs().max()) <= 1e-3
    assert float((lsum - torch_pack_combined()[2]).abs().max()) <= 1e-4

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    rounds = [{name + suffix: timed(fn) for name, pair in calls.items() for suffix, fn in zip(("_ms", "_torch_ms"), pair)} for _ in range(2)]
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    bytes_per_px = t["bytes_per_px"]
    kernels = {}
    for name in calls:
        rate = bytes_per_px[name] * px / (best[name + "_ms"] * 1e-3) / 1e9
        kernels[name] = {"ms": best[name + "_ms"], "torch_ms": best[name + "_torch_ms"], "bytes_per_pixel": bytes_per_px[name], "gigabytes_per_second": rate,
                         "fraction_of_copy_rate": rate / gbps.value, "kernel_over_torch": best[name + "_ms"] / best[name + "_torch_ms"]}
    result["shadow_lights"] = dict(
        kernels=kernels, rounds=rounds, device=torch.cuda.get_device_name(0), width=w, height=h, lights=n, reps=args.reps, warmup=args.warmup, copy_gigabytes_per_second=gbps.value,
        planes="four LOCAL lights: distanceToOccluder / distanceToLight [4, H, W] fp32 (40 % of the texels lit), lighting [4, H, W, 4] fp32, shadows [4, H, W] uint8 (PER_LIGHT) "
               "or [H, W, 4] uint8 (COMBINED)",
        bytes_are="per pixel, from the formats: every input texel once (the 16-byte lighting texel whole, though 12 bytes of it are loaded) plus every output texel",
        torch_is="the same recipe as torch elementwise operations on the same tensors, allocations included: what a host without kernels writes",
        times_are="device events around --reps back-to-back calls, per call, the best of two alternated rounds",
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)")
    record = {}
    if os.path.exists(args.out):  # the other fields of the record are another run's: kept as they are
        with open(args.out) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")
    print(json.dumps({"shadow_lights": kernels, "copy_gigabytes_per_second": gbps.value}))
    for name, k in kernels.items():
        assert k["ms"] <= k["torch_ms"], "%s is slower than the torch chain it replaces (%.4f ms against %.4f ms): the kernel is not finished" % (name, k["ms"], k["torch_ms"])


GUIDES_SRC = os.path.join(B.CSRC, "hip", "kernels_guides.hip")


def guides_isa():
    """static facts about every instantiation of the kernel behind nrdHipPackGuides (the `isa_guides` object of profiles/frontend_bench.json), as isa(): named
    pack_guides_<bytes of a position texel>_<bytes of a positionPrev texel> (0 = the plane is absent)"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_guides.s")
        flags = [f for f in B._flags(GUIDES_SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", GUIDES_SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    out = {}
    for mangled, s in stats.items():
        m = re.search(r"PackGuidesKernelILj(\d+)ELj(\d+)E", mangled)
        if m:
            c = s["counter"]
            out["pack_guides_%s_%s" % m.groups()] = {
                "vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                "global_load_dwordx4": c.get("global_load_dwordx4", 0), "global_load_dwordx3": c.get("global_load_dwordx3", 0), "global_store_dwordx2": c.get("global_store_dwordx2", 0),
                "v_div_scale_f32": c.get("v_div_scale_f32", 0), "transcendental": s["trans"]}
    assert set(out) == {"pack_guides_%d_%d" % k for k in ((0, 0), (12, 0), (12, 12), (12, 16), (16, 0), (16, 12), (16, 16))}, list(stats)
    return out


def guides_main(args):
    """--guides: nrdHipPackGuides at 2560 x 1440 -- IN_VIEWZ and IN_MV from RGB32_SFLOAT position and positionPrev planes, 36 bytes per pixel -- against the copy rate of the same
    process, next to the four shadow-light calls on planes of the same size: streaming kernels of the same shape, its yardstick. The whole set is timed three times, the rows
    alternating; the spread of a row over the three rounds stands next to its number."""
    result = {"isa_guides": guides_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend, scene, synth

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    lib, stream = api.load_library(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(23)
    cam, cam_prev = synth.Camera(w, h, 1), synth.Camera(w, h, 0)
    cs = scene.common_settings(cam, cam_prev, w, h, 1, isMotionVectorInWorldSpace=False, motionVectorScale=(1.0 / w, 1.0 / h, 1.0))
    # points in front of both cameras, a tenth of them sky; the surface moved by a few centimetres
    depth = 2.0 + 30.0 * torch.rand(h, w, 1, device="cuda", generator=g)
    lateral = (torch.rand(h, w, 2, device="cuda", generator=g) - 0.5) * depth
    rot = torch.tensor([cam.right, cam.up, cam.fwd], device="cuda", dtype=torch.float32)
    position = (torch.cat([lateral, depth], -1) @ rot + torch.tensor(cam.pos, device="cuda")).contiguous()
    position[torch.rand(h, w, device="cuda", generator=g) < 0.1] = float("nan")
    position_prev = (position + 0.02 * (torch.rand(h, w, 3, device="cuda", generator=g) - 0.5)).contiguous()
    res, desc, keep = frontend.describe_pack_guides(position, cs, position_prev)
    t = _shadow_light_planes(torch, api, frontend, w, h)

    def call(fn, d):
        def f():
            assert fn(C.byref(d), stream) == 0, lib.nrdHipGetLastFrontEndError()
        return f

    calls = {"guides": call(lib.nrdHipPackGuides, desc), "pack_per_light": call(lib.nrdHipPackShadowLights, t["per_desc"]), "pack_combined": call(lib.nrdHipPackShadowLights, t["com_desc"]),
             "resolve_per_light": call(lib.nrdHipResolveShadowLights, t["rdesc_a"]), "resolve_combined": call(lib.nrdHipResolveShadowLights, t["rdesc_b"])}
    bytes_per_px = dict(t["bytes_per_px"], guides=12 + 12 + 4 + 8)
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    viewz = res.viewz
    sky = torch.isnan(position[..., 0])
    assert bool((viewz[sky] == frontend.MISS_VIEWZ).all()) and bool(torch.isfinite(viewz).all()) and bool(torch.isfinite(res[api.ResourceType.IN_MV][0].float()).all())

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    rounds = [{name: timed(fn) for name, fn in calls.items()} for _ in range(3)]
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    rows = {}
    for name in calls:
        ms = [r[name] for r in rounds]
        fraction = lambda v: bytes_per_px[name] * px / (v * 1e-3) / 1e9 / gbps.value
        rows[name] = {"ms": min(ms), "bytes_per_pixel": bytes_per_px[name], "fraction_of_copy_rate": fraction(min(ms)), "fraction_of_copy_rate_worst_round": fraction(max(ms)),
                      "spread": (max(ms) - min(ms)) / min(ms)}
    yardstick = min(rows[name]["fraction_of_copy_rate"] for name in rows if name != "guides")
    spread = max(rows[name]["spread"] for name in rows if name != "guides")  # of the yardstick rows: the guides row's own outliers must not widen what it is allowed
    result["guides"] = dict(
        rows=rows, rounds=rounds, device=torch.cuda.get_device_name(0), width=w, height=h, reps=args.reps, warmup=args.warmup, copy_gigabytes_per_second=gbps.value,
        lowest_shadow_light_fraction=yardstick, run_to_run_spread=spread, guides_meets_yardstick=rows["guides"]["fraction_of_copy_rate"] >= yardstick * (1.0 - spread),
        planes="position and positionPrev [H, W, 3] fp32 (RGB32_SFLOAT, a tenth of the texels NaN), IN_VIEWZ [H, W] fp32 and IN_MV [H, W, 4] fp16 out, screen-space 2.5D vectors; "
               "the four shadow-light calls of --shadow-lights on planes of the same size",
        bytes_are="per pixel, from the formats: every input texel once plus every output texel",
        times_are="device events around --reps back-to-back calls, per call; the whole set three times, the rows alternating; ms is the best round, spread = ( worst - best ) / best; run_to_run_spread is the largest spread among the four shadow-light rows",
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)")
    record = {}
    if os.path.exists(args.out):  # the other fields of the record are another run's: kept as they are
        with open(args.out) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")
    print(json.dumps({"guides": rows, "copy_gigabytes_per_second": gbps.value, "lowest_shadow_light_fraction": yardstick, "run_to_run_spread": spread}))


def upsample_isa():
    """static facts about the kernels behind nrdHipResolveOutputsUpsampled and nrdHipPackInputsDecimated (the `isa_upsample` object of profiles/frontend_bench.json), as isa(),
    next to the plain kernels they are twins of"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_frontend.s")
        flags = [f for f in B._flags(SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    names = {"ResolveUpsampledKernel": "resolve_upsampled", "ResolveUpsampledSplitKernel": "resolve_upsampled_split", "ResolveOutputsKernel": "resolve", "PackDecimatedKernel": "pack_decimated",
             "PackDecimatedSamplesKernel": "pack_decimated_samples", "PackDecimatedSplitKernel": "pack_decimated_split", "PackDecimatedSamplesSplitKernel": "pack_decimated_samples_split",
             "PackInputsKernel": "pack"}
    out = {}
    for mangled, s in stats.items():
        for kernel, name in names.items():
            if re.search(r"\d+" + kernel + "E", mangled):
                c = s["counter"]
                out[name] = {"vgprs": s["vgpr"], "waves_per_simd": s["occ"], "scratch_bytes": s["scratch"], "lds_bytes": s["ldsb"], "valu": s["valu"], "salu": s["salu"], "vmem": s["vmem"],
                             "global_load_dwordx4": c.get("global_load_dwordx4", 0), "global_load_dwordx2": c.get("global_load_dwordx2", 0), "global_load_dword": c.get("global_load_dword", 0),
                             "global_store_dwordx4": c.get("global_store_dwordx4", 0), "global_store_byte": c.get("global_store_byte", 0)}
    assert set(out) == set(names.values()), (sorted(out), list(stats))
    return out


def upsample_main(args):
    """--upsample (see the module text). Times are device events around --reps back-to-back calls, per call; five rounds with the rows alternating, the median of each row."""
    result = {"isa_upsample": upsample_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import statistics

    import torch

    from raytracingdenoiser_amd import api, frontend, scene, synth
    from raytracingdenoiser_amd.executor import HipExecutor

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    W, H = args.width, args.height
    w, h = (W + 1) >> 1, (H + 1) >> 1
    lib, stream = api.load_library(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    R, S, name = api.ResourceType, frontend.SignalMode, "REBLUR_DIFFUSE_SPECULAR"
    frame = synth.render_frame(W, H, 1, device="cuda", want=("reblur", "raw"))
    raw = frame["raw"]
    cat = lambda a, b: torch.cat([a, b.unsqueeze(-1)], -1).contiguous()
    nr, viewz, motion = cat(raw["normal"], raw["roughness"]), frame["viewz"].contiguous(), frame["mv"].float().contiguous()
    diff, spec = cat(raw["diff_radiance"], raw["diff_hit_dist"]), cat(raw["spec_radiance"], raw["spec_hit_dist"])
    g = torch.Generator(device="cuda").manual_seed(31)
    albedo, rf0 = (torch.rand(H, W, 4, device="cuda", generator=g).contiguous() * 0.9 + 0.05 for _ in range(2))
    dec = lambda t: t[::2, ::2].contiguous()
    sig = lambda d, s: dict(diffuse=dict(mode=S.REBLUR_RADIANCE, radiance_hitdist=d), specular=dict(mode=S.REBLUR_RADIANCE, radiance_hitdist=s))
    cam = frame["camera"]
    cs = {"full": scene.common_settings(cam, cam, W, H, 1), "low": scene.common_settings(cam, cam, w, h, 1)}  # halved: rectSize / resourceSize; the matrices are the frame's
    packed = {"full": frontend.describe_pack(nr, viewz, material_id=raw["material_id"].contiguous(), motion=motion, **sig(diff, spec)),
              "low": frontend.describe_pack(nr, viewz, material_id=raw["material_id"].contiguous(), motion=motion, guide_shift=1, **sig(dec(diff), dec(spec)))}
    guides = frontend.describe_pack(nr, viewz)  # the quarter-resolution frame's full-size guide pack: IN_NORMAL_ROUGHNESS and IN_VIEWZ for the upsampled resolve
    none = {"options": api.HipFrontEndOptions(), "samples": api.HipFrontEndSamples(), "split": api.HipFrontEndSplit()}

    def check(code):
        assert code == 0, lib.nrdHipGetLastFrontEndError()

    pack = {"full": lambda: check(lib.nrdHipPackInputs(C.byref(packed["full"][1]), stream)), "guides": lambda: check(lib.nrdHipPackInputs(C.byref(guides[1]), stream)),
            "low": lambda: check(lib.nrdHipPackInputsDecimated(C.byref(packed["low"][1]), C.byref(none["options"]), C.byref(none["samples"]), C.byref(none["split"]), 1, stream))}
    chains = {}
    for key, (cw, ch) in (("full", (W, H)), ("low", (w, h))):
        inst = api.Instance([(0, scene.DENOISERS[name][0])])
        ex = HipExecutor(inst, cw, ch)
        outs = {rt: (torch.zeros((ch, cw, c), dtype=dtype, device="cuda"), fmt) for rt, dtype, c, fmt in scene.output_planes(name, cw, ch)}
        for rt, (t, fmt) in outs.items():
            ex.bind(rt, t, fmt)
        ex.bind_packed(packed[key][0])
        assert inst.set_denoiser_settings(0, scene.denoiser_settings(name, frame)) == api.Result.SUCCESS and inst.set_common_settings(cs[key]) == api.Result.SUCCESS
        chains[key] = (inst, ex, outs)
    signals = lambda outs: dict(diffuse=dict(mode=S.REBLUR_RADIANCE, in0=outs[R.OUT_DIFF_RADIANCE_HITDIST][0]), specular=dict(mode=S.REBLUR_RADIANCE, in0=outs[R.OUT_SPEC_RADIANCE_HITDIST][0]))
    common = dict(normal_roughness=guides[0][R.IN_NORMAL_ROUGHNESS][0], viewz=guides[0][R.IN_VIEWZ][0], albedo=albedo, rf0=rf0, remodulate=True, want=("composed",))
    plain_res, plain_desc, keep_a = frontend.describe_resolve(common_settings=cs["full"], **signals(chains["full"][2]), **common)
    up_res, up_desc, keep_b = frontend.describe_resolve(common_settings=cs["low"], low_viewz=packed["low"][0][R.IN_VIEWZ][0], want_source=True, **signals(chains["low"][2]), **common)
    up_struct, no_options, no_split = frontend.resolve_upsample(up_res, packed["low"][0][R.IN_VIEWZ][0]), api.HipBackEndOptions(), api.HipBackEndSplit()
    resolve = lambda: check(lib.nrdHipResolveOutputs(C.byref(plain_desc), stream))
    resolve_upsampled = lambda: check(lib.nrdHipResolveOutputsUpsampled(C.byref(up_desc), C.byref(no_options), C.byref(no_split), C.byref(up_struct), stream))

    def frame_full():
        pack["full"]()
        chains["full"][1].denoise()
        resolve()

    def frame_quarter():
        pack["guides"]()
        pack["low"]()
        chains["low"][1].denoise()
        resolve_upsampled()

    for _ in range(8):  # history builds up; every call has run once
        frame_full()
        frame_quarter()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(up_res["composed"]).all()) and bool((up_res["source"][frame["viewz"].abs() <= cs["low"].denoisingRange] != api.NO_SOURCE).all())

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    rows = {"resolve": (resolve, args.reps), "resolve_upsampled": (resolve_upsampled, args.reps), "pack_decimated": (pack["low"], args.reps), "pack": (pack["full"], args.reps),
            "frame_full": (frame_full, max(args.reps // 10, 8)), "frame_quarter": (frame_quarter, max(args.reps // 10, 8))}
    rounds = [{k: timed(fn, reps) for k, (fn, reps) in rows.items()} for _ in range(5)]
    median = {k: statistics.median(r[k] for r in rounds) for k in rows}
    spread = {k: (max(r[k] for r in rounds) - min(r[k] for r in rounds)) / min(r[k] for r in rounds) for k in rows}
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    # per FULL pixel, from the formats: IN_NORMAL_ROUGHNESS 4, viewZ 4, albedo 16, rf0 16; three RGBA32_SFLOAT outputs 48; the two RGBA16_SFLOAT signal planes 16 at full size,
    # a quarter of that plus a quarter of lowViewZ (4) and outSource (1) when upsampling
    bytes_px = {"resolve": 4 + 4 + 16 + 16 + 48 + 16, "resolve_upsampled": 4 + 4 + 16 + 16 + 48 + (16 + 4) / 4.0 + 1}
    fraction = lambda k: bytes_px[k] * W * H / (median[k] * 1e-3) / 1e9 / gbps.value
    result["upsample"] = dict(
        device=torch.cuda.get_device_name(0), width=W, height=H, low_width=w, low_height=h, reps=args.reps, warmup=args.warmup, rounds=rounds, median_ms=median, spread=spread,
        copy_gigabytes_per_second=gbps.value, bytes_per_full_pixel=bytes_px, resolve_fraction_of_copy_rate=fraction("resolve"), resolve_upsampled_fraction_of_copy_rate=fraction("resolve_upsampled"),
        resolve_upsampled_over_resolve=median["resolve_upsampled"] / median["resolve"], frame_quarter_over_frame_full=median["frame_quarter"] / median["frame_full"],
        what="REBLUR_DIFFUSE_SPECULAR, radiance mode, remodulation, outComposed; `resolve` is nrdHipResolveOutputs on full-size OUT_* planes, `resolve_upsampled` nrdHipResolveOutputsUpsampled "
             "on the half-size ones (with outSource); frame_full = pack + denoise + resolve at full size, frame_quarter = full-size guide pack + decimated pack + denoise at the low size + "
             "upsampled resolve; default denoiser settings, one synthetic frame repeated",
        times_are="device events around back-to-back calls, per call (frames: a tenth of --reps); five rounds with the rows alternating; median_ms is the median over the rounds, "
                  "spread = ( worst - best ) / best",
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)")
    for inst, ex, outs in chains.values():
        ex.destroy()
    record = {}
    if os.path.exists(args.out):  # the other fields of the record are another run's: kept as they are
        with open(args.out) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")
    print(json.dumps({k: v for k, v in result["upsample"].items() if k != "rounds"}))


COVERAGE_SRC = os.path.join(B.CSRC, "hip", "kernels_coverage.hip")
LOBES_READ = {"normal_roughness RGBA32_SFLOAT": 16, "viewZ R32_SFLOAT": 4, "traced radiance_hitdist RGBA32_SFLOAT": 16, "lobe R8_UINT": 1, "probability R32_SFLOAT": 4}
LOBES_WRITE = {"IN_NORMAL_ROUGHNESS": 4, "IN_VIEWZ R32_SFLOAT": 4, "IN_DIFF_RADIANCE_HITDIST RGBA16_SFLOAT": 8, "IN_SPEC_RADIANCE_HITDIST RGBA16_SFLOAT": 8}
PLAIN_READ = {"normal_roughness RGBA32_SFLOAT": 16, "viewZ R32_SFLOAT": 4, "diffuse radiance_hitdist RGBA32_SFLOAT": 16, "specular radiance_hitdist RGBA32_SFLOAT": 16}
COVERAGE_READ = {"IN_VIEWZ R32_SFLOAT": 4, "IN_DIFF_RADIANCE_HITDIST .w": 2, "IN_SPEC_RADIANCE_HITDIST .w": 2}


def lobes_isa():
    """static facts about the kernels behind nrdHipPackInputsLobes and nrdHipCheckHitDistCoverage (the `isa_lobes` object of profiles/frontend_bench.json), as isa(): "pack_lobes",
    "coverage_3x3" and "coverage_5x5"; atomics: the global atomics of a listing -- all of them sit behind the wave's exit"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in (SRC, COVERAGE_SRC):
            listing = os.path.join(tmp, os.path.basename(src) + ".s")
            flags = [f for f in B._flags(src) if f not in ("-x", "hip")]
            subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", src, "-o", listing], check=True, capture_output=True, text=True)
            for mangled, k in isa_stats.parse(listing).items():
                m = re.search(r"HitDistCoverageKernelILi(\d)E", mangled)
                name = "pack_lobes" if "PackLobesKernel" in mangled else "coverage_%dx%d" % ((2 * int(m.group(1)) + 1,) * 2) if m else None
                if name:
                    c = k["counter"]
                    out[name] = dict(_facts(k), global_load_dwordx4=c.get("global_load_dwordx4", 0), global_load_dwordx3=c.get("global_load_dwordx3", 0),
                                     atomics={i: v for i, v in c.items() if i.startswith("global_atomic")})
    assert set(out) == {"pack_lobes", "coverage_3x3", "coverage_5x5"}, sorted(out)
    return out


def lobes_main(args):
    """--lobes: see the module text"""
    result = {"isa_lobes": lobes_isa()}
    if args.isa_only:
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    S = api.SignalMode
    g = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    normal = torch.nn.functional.normalize(rand(h, w, 3) - 0.5, dim=-1)
    nr = torch.cat([normal, rand(h, w, 1) * 0.95 + 0.05], -1).contiguous()
    viewz = rand(h, w) * 49.0 + 1.0
    traced = torch.cat([rand(h, w, 3) * 4.0, rand(h, w, 1) * 29.9 + 0.1], -1).contiguous()
    prob = rand(h, w) * 0.9 + 0.05
    bayer = torch.tensor([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], device="cuda", dtype=torch.float32)
    threshold = (bayer.repeat((h + 3) // 4, (w + 3) // 4)[:h, :w] + 0.5) / 16.0
    lobe = (threshold < prob).to(torch.uint8).contiguous()  # the application's dithering: a 4 x 4 Bayer threshold against the probability of the specular lobe
    lib, stream = api.load_library(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sig = dict(mode=S.REBLUR_RADIANCE)
    packed, lobes_desc, keep0 = frontend.describe_pack(nr, viewz, diffuse=sig, specular=sig)
    lo, keep1 = frontend.pack_lobes(traced, lobe, prob)
    options, split = frontend.pack_options(), api.HipFrontEndSplit()

    def prepare():  # what a tensor host does today before the plain call: two full RGBA32_SFLOAT planes
        q = torch.where(lobe == 1, prob, 1.0 - prob)
        scaled = torch.cat([traced[..., :3] / q.unsqueeze(-1), traced[..., 3:]], -1)
        return tuple(torch.where(((lobe == X) & (q > 0)).unsqueeze(-1), scaled, torch.zeros((), device="cuda")) for X in (0, 1))

    planes = prepare()
    plain_packed, plain_desc, keep2 = frontend.describe_pack(nr, viewz, diffuse=dict(sig, radiance_hitdist=planes[0]), specular=dict(sig, radiance_hitdist=planes[1]))
    R = api.ResourceType
    coverage_desc = frontend.describe_coverage(packed[R.IN_VIEWZ][0], packed[R.IN_DIFF_RADIANCE_HITDIST][0], packed[R.IN_SPEC_RADIANCE_HITDIST][0], area=2)
    report = torch.zeros(7, dtype=torch.int32, device="cuda")
    raw_report = C.c_void_p(report.data_ptr())

    def pack_lobes():
        assert lib.nrdHipPackInputsLobes(C.byref(lobes_desc), C.byref(options), C.byref(split), C.byref(lo), stream) == 0, lib.nrdHipGetLastFrontEndError()

    def pack_plain():
        assert lib.nrdHipPackInputs(C.byref(plain_desc), stream) == 0, lib.nrdHipGetLastFrontEndError()

    def coverage():
        assert lib.nrdHipCheckHitDistCoverage(C.byref(coverage_desc), raw_report, stream) == 0, lib.nrdHipGetLastFrontEndError()

    pack_lobes()
    pack_plain()
    coverage()
    torch.cuda.synchronize()
    for rt in packed:  # the two paths produce the same planes: what is timed is the same work
        assert torch.equal(packed[rt][0].view(torch.uint8), plain_packed[rt][0].view(torch.uint8)), rt
    words = report.cpu().numpy().view("uint32")
    assert int(words[0]) == px and int(words[1]) > px // 4 and int(words[2]) > px // 4, words

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    rows = {"pack_lobes_ms": pack_lobes, "pack_plain_ms": pack_plain, "torch_prepare_ms": prepare, "coverage_5x5_ms": coverage}
    rounds = [{k: timed(fn) for k, fn in rows.items()} for _ in range(5)]
    best = {k: min(r[k] for r in rounds) for k in rows}
    median = {k: sorted(r[k] for r in rounds)[2] for k in rows}
    spread = {k: (max(r[k] for r in rounds) - min(r[k] for r in rounds)) / min(r[k] for r in rounds) for k in rows}
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    rate = lambda bytes_per_px, ms: bytes_per_px * px / (ms * 1e-3) / 1e9
    lobes_bytes, plain_bytes, coverage_bytes = sum(LOBES_READ.values()) + sum(LOBES_WRITE.values()), sum(PLAIN_READ.values()) + sum(LOBES_WRITE.values()), sum(COVERAGE_READ.values())
    noise = max(spread["pack_lobes_ms"], spread["pack_plain_ms"])
    result["lobes"] = dict(
        best=best, median=median, run_to_run_spread=spread, rounds=rounds, device=torch.cuda.get_device_name(0), width=w, height=h, reps=args.reps, warmup=args.warmup,
        times_are="device events around --reps back-to-back calls, per call; five rounds with the four rows alternating inside each round; spread = ( max - min ) / min of a row over the rounds",
        scene="REBLUR_RADIANCE on both signals; lobe = a 4 x 4 Bayer threshold against a probability in [0.05, 0.95]; pack_plain_ms packs the two planes torch_prepare_ms builds, and both pack rows write the same bytes",
        lobes_read_bytes_per_pixel=LOBES_READ, plain_read_bytes_per_pixel=PLAIN_READ, write_bytes_per_pixel=LOBES_WRITE, coverage_read_bytes_per_pixel=COVERAGE_READ,
        pack_lobes_gigabytes_per_second=rate(lobes_bytes, best["pack_lobes_ms"]), pack_plain_gigabytes_per_second=rate(plain_bytes, best["pack_plain_ms"]),
        coverage_gigabytes_per_second=rate(coverage_bytes, best["coverage_5x5_ms"]), copy_gigabytes_per_second=gbps.value,
        pack_lobes_fraction_of_copy_rate=rate(lobes_bytes, best["pack_lobes_ms"]) / gbps.value, coverage_fraction_of_copy_rate=rate(coverage_bytes, best["coverage_5x5_ms"]) / gbps.value,
        coverage_bytes_are="the 8 bytes per pixel the kernel consumes (viewZ and the 16 bits of .w of either signal); the memory system moves whole 8-byte texels' sectors, 20 per pixel",
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)",
        pack_lobes_over_pack_plain=median["pack_lobes_ms"] / median["pack_plain_ms"], pack_lobes_over_plain_path=median["pack_lobes_ms"] / (median["pack_plain_ms"] + median["torch_prepare_ms"]),
        pack_lobes_slower_than_plain_beyond_the_spread=bool(median["pack_lobes_ms"] > median["pack_plain_ms"] * (1.0 + noise)), holes_5x5=[int(words[3]), int(words[4])])
    record = {}
    if os.path.exists(args.out):  # the other fields of the record are another run's: kept as they are
        with open(args.out) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")
    print(json.dumps({k: v for k, v in result["lobes"].items() if k != "rounds"}))
    print(json.dumps(result["isa_lobes"]))
    assert not result["lobes"]["pack_lobes_slower_than_plain_beyond_the_spread"], "nrdHipPackInputsLobes is slower than the plain pack it replaces by more than the run-to-run spread"


DIRECT_KERNELS = {"PackDirectKernel": "pack_direct", "PackDirectCheckerboardKernel": "pack_direct_checkerboard", "PackDirectDecimatedKernel": "pack_direct_decimated"}
DIRECT_READ = {"normal_roughness RGBA32_SFLOAT": 16, "viewZ R32_SFLOAT": 4, "diffuse indirect RGBA32_SFLOAT": 16, "specular indirect RGBA32_SFLOAT": 16, "diffuse direct RGBA32_SFLOAT": 16,
               "specular direct RGBA32_SFLOAT": 16}
DIRECT_WRITE = {"IN_NORMAL_ROUGHNESS": 4, "IN_VIEWZ R32_SFLOAT": 4, "IN_DIFF_RADIANCE_HITDIST RGBA16_SFLOAT": 8, "IN_SPEC_RADIANCE_HITDIST RGBA16_SFLOAT": 8}


def direct_isa():
    """static facts about the three kernels behind nrdHipPackInputsDirect (the `isa_direct` object of profiles/frontend_bench.json), as isa(): "pack_direct",
    "pack_direct_checkerboard" and "pack_direct_decimated", with their 12- and 16-byte loads"""
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, "kernels_frontend.s")
        flags = [f for f in B._flags(SRC) if f not in ("-x", "hip")]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-x", "hip", SRC, "-o", listing], check=True, capture_output=True, text=True)
        stats = isa_stats.parse(listing)
    out = {}
    for mangled, k in stats.items():
        for kernel, name in DIRECT_KERNELS.items():
            if kernel in mangled:
                c = k["counter"]
                out[name] = dict(_facts(k), global_load_dwordx4=c.get("global_load_dwordx4", 0), global_load_dwordx3=c.get("global_load_dwordx3", 0), global_load_dword=c.get("global_load_dword", 0))
    assert set(out) == set(DIRECT_KERNELS.values()), sorted(out)
    return out


def _update_record(path, result):
    record = {}
    if os.path.exists(path):  # the other fields of the record are another run's: kept as they are
        with open(path) as fp:
            record = json.load(fp)
    record.update(result)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")


def direct_main(args):
    """--direct: see the module text"""
    result = {"isa_direct": direct_isa()}
    if args.isa_only:
        _update_record(args.out, result)
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    S, R = api.SignalMode, api.ResourceType
    g = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    normal = torch.nn.functional.normalize(rand(h, w, 3) - 0.5, dim=-1)
    nr = torch.cat([normal, rand(h, w, 1) * 0.95 + 0.05], -1).contiguous()
    viewz = rand(h, w) * 49.0 + 1.0
    traced = lambda: torch.cat([rand(h, w, 3) * 4.0, rand(h, w, 1) * 29.9 + 0.1], -1).contiguous()
    indirect, lit = (traced(), traced()), (traced(), traced())  # (diffuse, specular)
    for plane in lit:  # a quarter of the pixels sampled no light
        plane[rand(h, w) < 0.25] = float("nan")
    max_contribution = api.DIRECT_MAX_CONTRIBUTION_DEFAULT
    lib, stream = api.load_library(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sig = lambda plane: dict(mode=S.REBLUR_RADIANCE, radiance_hitdist=plane)
    packed, desc, keep0 = frontend.describe_pack(nr, viewz, diffuse=sig(indirect[0]), specular=sig(indirect[1]))
    di, keep1 = frontend.pack_direct(lit[0], lit[1], max_contribution)
    options, samples, split = frontend.pack_options(), api.HipFrontEndSamples(), api.HipFrontEndSplit()
    composed = (torch.empty_like(indirect[0]), torch.empty_like(indirect[1]))
    plain_packed, plain_desc, keep2 = frontend.describe_pack(nr, viewz, diffuse=sig(composed[0]), specular=sig(composed[1]))
    luma = torch.tensor([0.2126, 0.7152, 0.0722], device="cuda")

    def compose():  # what a tensor host does today before the plain call: the README's rule in torch, two full RGBA32_SFLOAT planes
        for spec in (False, True):
            ind, d = indirect[spec], torch.nan_to_num(lit[spec], nan=0.0, posinf=0.0, neginf=0.0)
            rad = ind[..., :3] + d[..., :3]
            hit = ind[..., 3]
            if not spec:
                li, ld = (ind[..., :3].clamp(0.0, 65504.0) * luma).sum(-1), (d[..., :3].clamp(0.0, 65504.0) * luma).sum(-1)
                c = (ld / (ld + li + 1e-6)).clamp(max=max_contribution)
                hit = torch.where((c > 0) & (hit > 0) & (d[..., 3] > 0), hit + (d[..., 3] - hit) * c, hit)
            torch.cat([rad, hit.unsqueeze(-1)], -1, out=composed[spec])

    def pack_direct():
        assert lib.nrdHipPackInputsDirect(C.byref(desc), C.byref(options), C.byref(samples), C.byref(split), C.byref(di), 0, stream) == 0, lib.nrdHipGetLastFrontEndError()

    def pack_plain():
        assert lib.nrdHipPackInputs(C.byref(plain_desc), stream) == 0, lib.nrdHipGetLastFrontEndError()

    def host_path():
        compose()
        pack_plain()

    pack_direct()
    host_path()
    torch.cuda.synchronize()
    for rt in packed:  # the two paths pack the same frame: what is timed is the same work (the host sums before it packs: fp16 roundings apart)
        a, b = packed[rt][0].float(), plain_packed[rt][0].float()
        assert bool(torch.isfinite(a).all()) and torch.allclose(a, b, rtol=1e-2, atol=1e-2), rt

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    rows = {"pack_direct_ms": pack_direct, "host_path_ms": host_path, "torch_compose_ms": compose, "pack_plain_ms": pack_plain}
    rounds = [{k: timed(fn) for k, fn in rows.items()} for _ in range(5)]
    best = {k: min(r[k] for r in rounds) for k in rows}
    median = {k: sorted(r[k] for r in rounds)[2] for k in rows}
    spread = {k: (max(r[k] for r in rounds) - min(r[k] for r in rounds)) / min(r[k] for r in rounds) for k in rows}
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, stream, C.byref(gbps)) == 0
    rate = lambda bytes_per_px, ms: bytes_per_px * px / (ms * 1e-3) / 1e9
    direct_bytes = sum(DIRECT_READ.values()) + sum(DIRECT_WRITE.values())
    result["direct"] = dict(
        best=best, median=median, run_to_run_spread=spread, rounds=rounds, device=torch.cuda.get_device_name(0), width=w, height=h, reps=args.reps, warmup=args.warmup,
        times_are="device events around --reps back-to-back calls, per call; five rounds with the four rows alternating inside each round; spread = ( max - min ) / min of a row over the rounds",
        scene="REBLUR_RADIANCE on both signals, RGBA32_SFLOAT planes, maxHitDistContribution 0.5, a quarter of the direct texels NaN (no light sampled); host_path_ms = torch_compose_ms's "
              "work followed by pack_plain_ms's, timed as one row",
        read_bytes_per_pixel=DIRECT_READ, write_bytes_per_pixel=DIRECT_WRITE, pack_direct_bytes_per_pixel=direct_bytes,
        pack_direct_gigabytes_per_second=rate(direct_bytes, best["pack_direct_ms"]), copy_gigabytes_per_second=gbps.value,
        pack_direct_fraction_of_copy_rate=rate(direct_bytes, best["pack_direct_ms"]) / gbps.value,
        fraction_is_not="a share of HBM bandwidth: the working set partly fits the memory-side cache, as for pack and resolve (DESIGN.md section 3.4)",
        pack_direct_over_host_path=median["pack_direct_ms"] / median["host_path_ms"], pack_direct_slower_than_host_path=bool(median["pack_direct_ms"] > median["host_path_ms"]))
    _update_record(args.out, result)
    print(json.dumps({k: v for k, v in result["direct"].items() if k != "rounds"}))
    print(json.dumps(result["isa_direct"]))
    assert not result["direct"]["pack_direct_slower_than_host_path"], "nrdHipPackInputsDirect is slower than the torch composition and the plain pack it replaces"


def synth_pack(raw, synth, torch):
    """the packing of synth.render_frame for REBLUR_DIFFUSE_SPECULAR on the raw values: its packers, elementwise torch operations with fp32 intermediates"""
    out = {"normal_roughness": synth.pack_normal_roughness(raw["normal"], raw["roughness"], raw["material"]).contiguous(), "viewz": raw["viewz"].clone(),
           "mv": raw["motion"].clamp(-synth.FP16_MAX, synth.FP16_MAX).to(torch.float16).contiguous()}
    for which, rough in (("diff", torch.ones_like(raw["roughness"])), ("spec", raw["roughness"])):
        rad = raw[which][..., :3].clamp(0.0, synth.FP16_MAX)
        nhd = synth._norm_hit_dist(raw[which][..., 3], raw["viewz"], rough)
        out[which] = torch.cat([synth._ycocg(rad), nhd.unsqueeze(-1)], -1).clamp(-synth.FP16_MAX, synth.FP16_MAX).to(torch.float16).contiguous()
    return out


def rejitter_calls(args, lib, stream, pack_desc, torch, api, frontend):
    """{name: callable} of the --rejitter section: the SH plane set is packed by the pack kernel from smooth raw values, the descriptors are built once"""
    from raytracingdenoiser_amd import scene, synth

    w, h = args.width, args.height
    g = torch.Generator(device="cuda").manual_seed(11)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    cam = synth.Camera(w, h, 0)
    cs = scene.common_settings(cam, cam, w, h, 0)
    # normals facing the viewer with per-pixel detail, depth without steps: NRD_SG_ReJitter accepts its four neighbours at almost every pixel
    n_view = torch.cat([0.6 * (rand(h, w, 2) - 0.5), -torch.ones(h, w, 1, device="cuda")], -1)
    n_view = n_view / n_view.norm(dim=-1, keepdim=True)
    rot = torch.tensor([cam.right, cam.up, cam.fwd], device="cuda", dtype=torch.float32)  # rows: the view axes in world space
    normal = n_view @ rot
    nr = torch.cat([normal, 0.05 + 0.95 * rand(h, w, 1)], -1).contiguous()
    xs = torch.arange(w, device="cuda", dtype=torch.float32)
    viewz = (5.0 + 0.002 * xs).expand(h, w).contiguous()

    def signal():
        direction = normal + 0.8 * (rand(h, w, 3) - 0.5)
        direction = torch.cat([direction / direction.norm(dim=-1, keepdim=True), torch.zeros(h, w, 1, device="cuda")], -1).contiguous()
        return dict(mode=frontend.SignalMode.REBLUR_SH, radiance_hitdist=(rand(h, w, 4) * torch.tensor([4.0, 3.0, 5.0, 30.0], device="cuda")).contiguous(), direction=direction)

    packed = frontend.pack_inputs(nr, viewz, diffuse=signal(), specular=signal())
    R, S, RES = api.ResourceType, frontend.SignalMode, frontend.ResolveMode
    rf0 = torch.cat([(0.04 + 0.8 * rand(h, w, 1)).expand(h, w, 3), torch.zeros(h, w, 1, device="cuda")], -1).contiguous()
    planes = dict(diffuse=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=packed[R.IN_DIFF_SH0][0], in1=packed[R.IN_DIFF_SH1][0]),
                  specular=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=packed[R.IN_SPEC_SH0][0], in1=packed[R.IN_SPEC_SH1][0]), normal_roughness=packed[R.IN_NORMAL_ROUGHNESS][0],
                  viewz=packed[R.IN_VIEWZ][0], common_settings=cs)
    res_a, desc_a, keep_a = frontend.describe_resolve(**planes)
    res_b, desc_b, keep_b = frontend.describe_resolve(rf0=rf0, **planes)
    options = frontend.resolve_options(res_b, viewz, rejitter=True)
    front_options = frontend.pack_options(api.CheckerboardMode.BLACK, 0)
    keep = [packed, res_a, keep_a, res_b, keep_b, rf0, cs]

    def call(fn, *a):
        def f(keep=keep):
            assert fn(*a) == 0
        return f

    calls = {"sg_resolve": call(lib.nrdHipResolveOutputs, C.byref(desc_a), stream), "rejitter": call(lib.nrdHipResolveOutputsEx, C.byref(desc_b), C.byref(options), stream),
             "pack_checkerboard": call(lib.nrdHipPackInputsEx, C.byref(pack_desc), C.byref(front_options), stream)}
    if args.ab_library:
        other = api.load_library(args.ab_library)
        calls["rejitter_other_form"] = call(other.nrdHipResolveOutputsEx, C.byref(desc_b), C.byref(options), stream)
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    scale = frontend.resolve_outputs(rejitter=True, rf0=rf0, want=("rejitter_scale",), **planes)["rejitter_scale"]
    print("re-jitter planes: %.1f %% of the pixels scaled" % (100.0 * float((scale != 1.0).any(-1).float().mean())))
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, help="default: 2560, with --shadow-lights 1920 (SIGMA's baseline size)")
    ap.add_argument("--height", type=int, help="default: 1440, with --shadow-lights 1080")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_bench.json"))
    ap.add_argument("--isa-only", action="store_true", help="no GPU needed: print the static facts and leave")
    ap.add_argument("--rejitter", action="store_true", help="also time the SH plane set: SG resolve, SG resolve + re-jitter (nrdHipResolveOutputsEx), and the checkerboard pack")
    ap.add_argument("--ab-library", help="with --rejitter: a build of the other re-jitter form (-DNRD_REJITTER_TILE=0), timed on the same planes in the same rounds")
    ap.add_argument("--samples", type=int, nargs="*", help="a run of its own: nrdHipPackInputsSamples with N sample layers per signal (default 4) against torch reductions + nrdHipPackInputs")
    ap.add_argument("--samples-out", default=os.path.join(ROOT, "profiles", "frontend_samples_bench.json"))
    ap.add_argument("--split", action="store_true", help="a run of its own: nrdHipPackInputsSplit / nrdHipResolveOutputsSplit on three-channel planes in place against widening + the "
                    "four-channel calls; adds the `split` and `isa_split` objects to --out and leaves its other fields as they are")
    ap.add_argument("--check-inputs", action="store_true", help="a run of its own: nrdHipCheckInputsAsync on the bound REBLUR_DIFFUSE_SPECULAR planes against the copy rate and a "
                    "torch.isfinite chain; adds the `check_inputs` and `isa_check_inputs` objects to --out and leaves its other fields as they are")
    ap.add_argument("--shadow-lights", action="store_true", help="a run of its own: nrdHipPackShadowLights / nrdHipResolveShadowLights for four local lights (1920 x 1080 unless --width / "
                    "--height say otherwise) against the copy rate and the same recipes as torch elementwise operations; adds the `shadow_lights` and `isa_shadow_lights` objects to --out")
    ap.add_argument("--guides", action="store_true", help="a run of its own: nrdHipPackGuides on RGB32_SFLOAT position planes against the copy rate, next to the four shadow-light "
                    "calls on planes of the same size, the whole set three times; adds the `guides` and `isa_guides` objects to --out and leaves its other fields as they are")
    ap.add_argument("--direct", action="store_true", help="a run of its own: nrdHipPackInputsDirect against the torch composition of the README's rule followed by nrdHipPackInputs; "
                    "adds the `direct` and `isa_direct` objects to --out (--isa-only: isa_direct alone, no GPU needed)")
    ap.add_argument("--lobes", action="store_true", help="a run of its own: nrdHipPackInputsLobes against nrdHipPackInputs on two prepared planes and the torch chain that prepares them, "
                    "and nrdHipCheckHitDistCoverage against the copy rate; adds the `lobes` and `isa_lobes` objects to --out")
    ap.add_argument("--upsample", action="store_true", help="a run of its own: nrdHipResolveOutputsUpsampled (half-size planes to --width x --height) against the plain resolve of the same "
                    "configuration and the copy rate, and whole frames at full and at quarter resolution; adds the `upsample` and `isa_upsample` objects to --out")
    args = ap.parse_args()
    default_size = (1920, 1080) if args.shadow_lights else (2560, 1440)
    args.width, args.height = args.width or default_size[0], args.height or default_size[1]
    if args.lobes:
        return lobes_main(args)
    if args.direct:
        return direct_main(args)
    if args.upsample:
        return upsample_main(args)
    if args.guides:
        return guides_main(args)
    if args.shadow_lights:
        return shadow_lights_main(args)
    if args.check_inputs:
        return check_inputs_main(args)
    if args.split:
        return split_main(args)
    if args.samples is not None:
        args.samples = args.samples or [4]
        return samples_main(args)
    result = {"isa": isa(), "isa_options": options_isa()}
    if args.isa_only:  # the static half of the record: nothing here is a time
        result["isa_check_inputs"] = check_inputs_isa()
        print(json.dumps(result))
        return
    import torch

    from raytracingdenoiser_amd import api, frontend, synth

    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench.py measures on the GPU: none is visible (--isa-only needs none)")
    w, h = args.width, args.height
    px = w * h
    g = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    n = rand(h, w, 3) * 2.0 - 1.0
    n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    raw = {"normal": n, "roughness": rand(h, w), "material": torch.floor(rand(h, w) * 4.0), "viewz": 0.5 + rand(h, w) * 100.0, "motion": rand(h, w, 4) - 0.5,
           "diff": rand(h, w, 4) * torch.tensor([4.0, 3.0, 5.0, 30.0], device="cuda"), "spec": rand(h, w, 4) * torch.tensor([4.0, 3.0, 5.0, 30.0], device="cuda")}
    nr = torch.cat([raw["normal"], raw["roughness"].unsqueeze(-1)], -1).contiguous()
    sig = lambda t: dict(mode=frontend.SignalMode.REBLUR_RADIANCE, radiance_hitdist=t)

    lib = api.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the descriptors are built once; the timed loops call the C-ABI itself (ctypes, a few microseconds), not the Python wrappers that assemble a descriptor per call
    packed, pack_desc, keep_pack = frontend.describe_pack(nr, raw["viewz"], material_id=raw["material"], motion=raw["motion"], diffuse=sig(raw["diff"]), specular=sig(raw["spec"]))

    def pack():
        assert lib.nrdHipPackInputs(C.byref(pack_desc), stream) == 0

    pack()
    R = api.ResourceType
    resolve_args = dict(diffuse=dict(mode=frontend.SignalMode.REBLUR_RADIANCE, in0=packed[R.IN_DIFF_RADIANCE_HITDIST][0]),
                        specular=dict(mode=frontend.SignalMode.REBLUR_RADIANCE, in0=packed[R.IN_SPEC_RADIANCE_HITDIST][0]), normal_roughness=packed[R.IN_NORMAL_ROUGHNESS][0],
                        viewz=packed[R.IN_VIEWZ][0], denormalize_hit_dist=True)
    resolved, resolve_desc, keep_resolve = frontend.describe_resolve(**resolve_args)

    def resolve():
        assert lib.nrdHipResolveOutputs(C.byref(resolve_desc), stream) == 0

    resolve()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / args.reps

    extra = {}
    if args.rejitter:
        extra = rejitter_calls(args, lib, stream, pack_desc, torch, api, frontend)

    # alternate the measurements twice: the spread between the rounds says how much a difference means
    rounds = []
    for _ in range(2):
        rounds.append({"pack_ms": timed(pack), "resolve_ms": timed(resolve), "synth_pack_ms": timed(lambda: synth_pack(raw, synth, torch)),
                       "pack_through_python_wrapper_ms": timed(lambda: frontend.pack_inputs(nr, raw["viewz"], material_id=raw["material"], motion=raw["motion"], diffuse=sig(raw["diff"]),
                                                                                           specular=sig(raw["spec"]), out=packed))})
        rounds[-1].update({name + "_ms": timed(fn) for name, fn in extra.items()})
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    # how fast the host can enqueue: the same call on a 64 x 4 frame, where the kernel is one workgroup -- a window bounded by this rate would measure the host, not the kernel
    tiny = torch.zeros(4, 64, 4, device="cuda")
    _, tiny_desc, keep_tiny = frontend.describe_pack(tiny, tiny[..., 0].contiguous(), diffuse=sig(tiny), specular=sig(tiny))
    enqueue_ms = timed(lambda: lib.nrdHipPackInputs(C.byref(tiny_desc), stream))
    gbps = C.c_double()
    assert lib.nrdHipMeasureCopyBandwidth(256 << 20, 20, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(gbps)) == 0
    pack_bytes, resolve_bytes = sum(PACK_READ.values()) + sum(PACK_WRITE.values()), sum(RESOLVE_READ.values()) + sum(RESOLVE_WRITE.values())
    rate = lambda bytes_per_px, ms: bytes_per_px * px / (ms * 1e-3) / 1e9
    result.update({
        "device": torch.cuda.get_device_name(0), "width": w, "height": h, "reps": args.reps, "warmup": args.warmup, "rounds": rounds,
        "pack": {"ms": best["pack_ms"], "read_bytes_per_pixel": PACK_READ, "write_bytes_per_pixel": PACK_WRITE, "bytes_per_pixel": pack_bytes, "gigabytes_per_second": rate(pack_bytes, best["pack_ms"])},
        "resolve": {"ms": best["resolve_ms"], "read_bytes_per_pixel": RESOLVE_READ, "write_bytes_per_pixel": RESOLVE_WRITE, "bytes_per_pixel": resolve_bytes,
                    "gigabytes_per_second": rate(resolve_bytes, best["resolve_ms"])},
        "synth_pack": {"ms": best["synth_pack_ms"], "what": "raytracingdenoiser_amd/synth.py packers (pack_normal_roughness, _ycocg, _norm_hit_dist, fp16 casts) on CUDA tensors, same planes"},
        "copy_gigabytes_per_second": gbps.value,
        "times_are": "device events around --reps back-to-back launches through the C-ABI, per launch; enqueue_floor_ms is the same loop on a 64 x 4 frame",
        "enqueue_floor_ms": enqueue_ms, "pack_through_python_wrapper_ms": best["pack_through_python_wrapper_ms"],
        "pack_over_synth_pack": best["pack_ms"] / best["synth_pack_ms"],
        "pack_fraction_of_copy_rate": rate(pack_bytes, best["pack_ms"]) / gbps.value,
        "resolve_fraction_of_copy_rate": rate(resolve_bytes, best["resolve_ms"]) / gbps.value,
    })
    if args.rejitter:
        sg_bytes, rj_bytes = sum(SH_RESOLVE_READ.values()) + sum(RESOLVE_WRITE.values()), sum(REJITTER_READ.values()) + sum(RESOLVE_WRITE.values())
        result["rejitter"] = {
            "planes": "REBLUR_SH for both signals in RGBA16_SFLOAT planes, IN_NORMAL_ROUGHNESS, IN_VIEWZ, rf0; smooth normals and depth, so that most pixels are scaled",
            "sg_resolve_ms": best["sg_resolve_ms"], "sg_resolve_read_bytes_per_pixel": SH_RESOLVE_READ, "sg_resolve_bytes_per_pixel": sg_bytes,
            "sg_resolve_fraction_of_copy_rate": rate(sg_bytes, best["sg_resolve_ms"]) / gbps.value,
            "ms": best["rejitter_ms"], "read_bytes_per_pixel": REJITTER_READ, "write_bytes_per_pixel": RESOLVE_WRITE, "bytes_per_pixel": rj_bytes,
            "gigabytes_per_second": rate(rj_bytes, best["rejitter_ms"]), "fraction_of_copy_rate": rate(rj_bytes, best["rejitter_ms"]) / gbps.value,
            "rejitter_over_sg_resolve": best["rejitter_ms"] / best["sg_resolve_ms"],
            "shipped_form": "a 64 x 4 workgroup stages decoded N.xyz and viewZ of its tile plus a one-texel halo in LDS (NRD_REJITTER_TILE = 1)",
            "fraction_is_not": "a share of HBM bandwidth: the working set partly fits the memory-side cache, as for resolve (DESIGN.md section 3.4)"}
        if "rejitter_other_form" in extra:
            result["rejitter"]["other_form"] = {"what": "every lane loads and decodes its four neighbour texels itself (NRD_REJITTER_TILE = 0), same planes, same rounds",
                                                "ms": best["rejitter_other_form_ms"], "over_shipped_form": best["rejitter_other_form_ms"] / best["rejitter_ms"]}
        result["pack_checkerboard"] = {"ms": best["pack_checkerboard_ms"], "over_pack": best["pack_checkerboard_ms"] / best["pack_ms"],
                                       "what": "nrdHipPackInputsEx, checkerboardMode = BLACK, on the planes of `pack`: reads every other texel of the two signal planes, writes half of the two packed ones"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("rounds", "isa")}))
    assert best["pack_ms"] < best["synth_pack_ms"], "the pack kernel must beat the torch packers it replaces"


if __name__ == "__main__":
    main()
