"""nrdHipPackInputsLobes (include/NRDHip.h, raytracingdenoiser_amd/frontend.py): one traced lobe per sample -- the probabilistic diffuse / specular split of the reference's README
("NOISY INPUTS") packed from ONE traced plane set, a lobe byte and a probability.

As in tests/test_pack_samples.py every comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU), and every comparison is
byte equality. Expected values never come from the code under test:
  P  the existing calls (nrdHipPackInputsEx / nrdHipPackInputsSamples / nrdHipPackInputsSplit) fed the planes an application would have had to build on the host
     (tests/lobes_model.py host_planes: rad / q and h where the sample counts, zeros elsewhere)
  M  tests/lobes_model.py for the one channel in which the call differs from them: the diffuse hit distance, a mean over the counted samples only
67 x 21 (odd; the last 64 x 4 workgroup column and row are partly outside), every plane with a row pitch larger than its row, outputs in stamped allocations."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lobes_model as LM
import test_pack_resolve as TPR
import test_pack_samples as TPS
from raytracingdenoiser_amd import api, frontend
from test_pack_resolve import BACKENDS, HDP, Backend, assert_bits, f16, snorm16, unorm16

ROOT = TPR.ROOT
F, R, S, CB, RC = api.Format, api.ResourceType, api.SignalMode, api.CheckerboardMode, api.Result
f32 = np.float32
STAMP = TPS.STAMP
PAD, GAP = 5, 3
DIFF_MODES = [S.REBLUR_RADIANCE, S.REBLUR_SH, S.REBLUR_OCCLUSION, S.REBLUR_DIRECTIONAL_OCCLUSION, S.RELAX_RADIANCE, S.RELAX_SH]
SPEC_MODES = [S.REBLUR_RADIANCE, S.REBLUR_SH, S.REBLUR_OCCLUSION, S.RELAX_RADIANCE, S.RELAX_SH]
PAIRS = [(dm, sm) for dm in DIFF_MODES for sm in SPEC_MODES]  # every pair of modes the plain call accepts with both signals present
SOME_PAIRS = [(S.REBLUR_RADIANCE, S.REBLUR_RADIANCE), (S.REBLUR_SH, S.RELAX_SH), (S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION), (S.REBLUR_DIRECTIONAL_OCCLUSION, S.RELAX_RADIANCE),
              (S.RELAX_SH, S.REBLUR_SH), (S.RELAX_RADIANCE, S.REBLUR_OCCLUSION)]  # every mode on either side once
_SCENES = {}


def scene(n):
    """computed once per sample count, shared and left unchanged"""
    if n not in _SCENES:
        _SCENES[n] = LM.scene(n)
        for a in _SCENES[n].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _SCENES[n]


# ---------------------------------------------------------------------------------------------------------------------------------------------- running the kernels
def up_stack(be, a, plane_ndim, fill):
    """[H, W(, C)] or [N, H, W(, C)] on the backend inside a wider allocation: rows PAD texels longer than the plane, GAP rows between the layers, `fill` around the rects"""
    a = np.ascontiguousarray(a)
    if a.ndim == plane_ndim:
        return up_stack(be, a[None], plane_ndim, fill)[0]
    big = np.full((a.shape[0], a.shape[1] + GAP, a.shape[2] + PAD) + a.shape[3:], fill, dtype=a.dtype)
    big[:, :a.shape[1], :a.shape[2]] = a
    big = big if be.name == "emu" else torch.from_numpy(big).cuda()
    return big[:, :a.shape[1], :a.shape[2]]


def frame(be, s):
    """tests/test_pack_samples.py's Frame -- its calls check that no byte outside an output's rect is written -- over the G-buffer of a lobes_model scene"""
    fr = TPS.Frame.__new__(TPS.Frame)
    fr.be, fr.d, fr.w, fr.h, fr.pad = be, None, s["w"], s["h"], PAD
    fr.ins = dict(nr=s["nr"], viewz=s["viewz"], albedo=s["albedo"])
    fr.dev = {k: be.up_pitched(v, PAD) for k, v in fr.ins.items()}
    fr.dev.update(rad=None, direction=None)
    fr.rf0 = be.up_pitched(s["rf0"], PAD)
    fr.cs = TPR.frame_settings(s["w"], s["h"])
    return fr


def squeeze(a, n):
    return a[0] if n == 1 else a


def traced(be, s, probability=True, rgb=False):
    """the traced planes of scene `s` on the backend, as frontend.pack_lobes takes them; rgb: radiance [.., 3] + hit distance [..] and a three-channel direction"""
    n = s["n"]
    rad, dirn = squeeze(s["rad"], n), squeeze(s["dirn"], n)
    t = dict(lobe=up_stack(be, squeeze(s["lobe"], n), 2, 77), probability=up_stack(be, squeeze(s["prob"], n), 2, np.nan) if probability else None)
    if rgb:
        t["radiance_hit_dist"] = (up_stack(be, rad[..., :3], 3, np.nan), up_stack(be, rad[..., 3], 2, np.nan))
        t["direction"] = up_stack(be, dirn[..., :3], 3, np.nan)
    else:
        t["radiance_hit_dist"], t["direction"] = up_stack(be, rad, 3, np.nan), up_stack(be, dirn, 3, np.nan)
    return t


def host_built(be, fr, s, X, probability=True):
    """(radiance_hitdist, direction) of signal X as Frame.call takes them: the planes an application builds on the host, uploaded"""
    rad, dirn = LM.host_planes(s, X, probability)
    return fr.up((squeeze(rad, s["n"]), squeeze(dirn, s["n"])), gap=GAP)


def needs_direction(mode):
    return mode in (S.REBLUR_SH, S.RELAX_SH, S.REBLUR_DIRECTIONAL_OCCLUSION)


def call_lobes(fr, dm, sm, t, demodulate=False, lobes="auto", split=None, options=None, mutate=None, expect=RC.SUCCESS):
    """one nrdHipPackInputsLobes launch through the C-ABI on the traced planes `t`, the outputs in stamped allocations. Returns ({ResourceType: plane}, {ResourceType: whole
    allocation}) like Frame.call; with expect != SUCCESS the error text, after checking that every output still holds its stamp."""
    be, dev, lib = fr.be, fr.dev, fr.be.lib
    kw = dict(hit_dist_params=HDP, lib=lib, diffuse=dict(mode=dm), specular=dict(mode=sm))
    if demodulate:
        kw.update(albedo=dev["albedo"], rf0=fr.rf0, common_settings=fr.cs)
    probe = frontend.describe_pack(dev["nr"], dev["viewz"], **kw)[0]
    out, bigs = {}, {}
    for rt, (a, fmt) in probe.items():
        name = frontend._dtype_name(a)
        view, bigs[rt] = be.padded(tuple(a.shape), name, fr.pad, 0x5A if name == "uint8" else STAMP)
        out[rt] = (view, fmt)
    res, desc, keep = frontend.describe_pack(dev["nr"], dev["viewz"], out=out, **kw)
    if lobes == "auto":
        lobes, keep_lobes = frontend.pack_lobes(t["radiance_hit_dist"], t["lobe"], t["probability"], t["direction"] if needs_direction(dm) or needs_direction(sm) else None)
    if mutate:
        mutate(desc, lobes)
    code = lib.nrdHipPackInputsLobes(C.byref(desc), None if options is None else C.byref(options), None if split is None else C.byref(split), None if lobes is None else C.byref(lobes), None)
    text = lib.nrdHipGetLastFrontEndError().decode()
    assert RC(code) == expect, (RC(code).name, text)
    got = {rt: be.down(a).copy() for rt, (a, fmt) in res.items()}
    whole = {rt: be.down(b).copy() for rt, b in bigs.items()}
    for rt, big in whole.items():
        want = np.full(big.shape, 0x5A if big.dtype == np.uint8 else STAMP, dtype=big.dtype)
        if expect == RC.SUCCESS:
            want[:fr.h, :fr.w] = got[rt]
        assert np.array_equal(big.view(np.uint8), want.view(np.uint8)), "bytes outside the rect were written (or, on an error, any byte at all): %s" % rt.name
    return (got, whole) if expect == RC.SUCCESS else text


def hit_dist_channel(mode, a):
    return a if mode == S.REBLUR_OCCLUSION else a[..., 3]


def diffuse_slot(mode):
    return frontend.signal_slots("diffuse", mode, "IN")[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1. N = 1
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_sample_equals_the_plain_call_on_host_built_planes(backend):
    """every pair of modes: each byte of each output allocation equals nrdHipPackInputsEx fed the two RGBA32_SFLOAT planes an application would build on the host; then, for every
    mode once on either side, the same with demodulation, without the probability plane (q = 1), and with an RGB32_SFLOAT traced plane + its hitDist companion"""
    be, s = Backend(backend), scene(1)
    fr = frame(be, s)
    t = traced(be, s)
    planes = {X: host_built(be, fr, s, X) for X in (LM.DIFFUSE, LM.SPECULAR)}
    for dm, sm in PAIRS:
        _, want = fr.call(dm, sm, diff=planes[LM.DIFFUSE], spec=planes[LM.SPECULAR], entry="ex")
        _, got = call_lobes(fr, dm, sm, t)
        TPS.assert_same_planes(got, want, "lobes N = 1 vs nrdHipPackInputsEx on host-built planes, %s / %s" % (dm.name, sm.name))
    t_q1, t_rgb = traced(be, s, probability=False), traced(be, s, rgb=True)
    planes_q1 = {X: host_built(be, fr, s, X, probability=False) for X in (LM.DIFFUSE, LM.SPECULAR)}
    for dm, sm in SOME_PAIRS:
        for what, tt, pl, demodulate in (("demodulated", t, planes, True), ("no probability plane", t_q1, planes_q1, False), ("RGB32_SFLOAT + hitDist", t_rgb, planes, False),
                                         ("RGB32_SFLOAT + hitDist, demodulated", t_rgb, planes, True)):
            _, want = fr.call(dm, sm, diff=pl[LM.DIFFUSE], spec=pl[LM.SPECULAR], entry="ex", demodulate=demodulate)
            _, got = call_lobes(fr, dm, sm, tt, demodulate=demodulate)
            TPS.assert_same_planes(got, want, "lobes N = 1, %s, %s / %s" % (what, dm.name, sm.name))
    # both modes read the hit distance alone: the R32_SFLOAT plane will do, no radiance plane at all
    hit_only = dict(t_rgb, radiance_hit_dist=(None, t_rgb["radiance_hit_dist"][1]))
    _, want = fr.call(S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, diff=planes[LM.DIFFUSE], spec=planes[LM.SPECULAR], entry="ex")
    _, got = call_lobes(fr, S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, hit_only)
    TPS.assert_same_planes(got, want, "lobes N = 1, the hit-distance plane alone, REBLUR_OCCLUSION / REBLUR_OCCLUSION")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2. N > 1
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [2, 5])
def test_many_samples_equal_the_samples_call_except_the_diffuse_hit_distance(backend, n):
    """every channel equals nrdHipPackInputsSamples on host-built layer stacks except the diffuse hit distance, which equals the numpy model (the mean of the counted samples; 0
    where no sample is diffuse) through the store codec; the specular hit distance is the one the plain call writes for the smallest non-zero sample"""
    be, s = Backend(backend), scene(n)
    fr = frame(be, s)
    t = traced(be, s)
    planes = {X: host_built(be, fr, s, X) for X in (LM.DIFFUSE, LM.SPECULAR)}
    spec_rad, spec_dir = LM.host_planes(s, LM.SPECULAR)
    single = spec_rad[0].copy()
    single[..., 3] = LM.spec_hit_dist(spec_rad[..., 3])
    single = fr.up((single, spec_dir[0]), gap=GAP)
    differs = 0
    for dm, sm in SOME_PAIRS:
        want, _ = fr.call(dm, sm, diff=planes[LM.DIFFUSE], spec=planes[LM.SPECULAR], entry="samples")
        got, _ = call_lobes(fr, dm, sm, t)
        assert set(got) == set(want)
        slot = diffuse_slot(dm)
        for rt in got:
            if rt != slot:
                assert_bits(got[rt], want[rt], "lobes N = %d vs nrdHipPackInputsSamples, %s / %s: %s" % (n, dm.name, sm.name, rt.name))
            elif dm != S.REBLUR_OCCLUSION:
                assert_bits(got[rt][..., :3], want[rt][..., :3], "lobes N = %d vs nrdHipPackInputsSamples, %s / %s: %s .xyz" % (n, dm.name, sm.name, rt.name))
        reblur = dm not in (S.RELAX_RADIANCE, S.RELAX_SH)
        model, num = LM.diffuse_hit_dist(s, reblur, dm == S.REBLUR_DIRECTIONAL_OCCLUSION, HDP)
        assert num[12, 33] == 0 and (num == 0).sum() > 10 and (num == n).sum() > 10 and ((num > 0) & (num < n)).sum() > 100
        codec = unorm16 if dm == S.REBLUR_OCCLUSION else snorm16 if dm == S.REBLUR_DIRECTIONAL_OCCLUSION else f16
        got_hit = hit_dist_channel(dm, got[slot])
        assert_bits(got_hit, codec(model), "lobes N = %d, %s: the diffuse hit distance vs the numpy model" % (n, dm.name))
        assert (got_hit.view(np.uint16)[num == 0] == 0).all(), "no diffuse sample: the hit distance is 0"
        differs += int((got_hit != hit_dist_channel(dm, want[slot])).sum())
        plain, _ = fr.call(dm, sm, diff=single, spec=single, entry="plain")
        spec_slot = frontend.signal_slots("specular", sm, "IN")[0]
        assert_bits(hit_dist_channel(sm, got[spec_slot]), hit_dist_channel(sm, plain[spec_slot]), "lobes N = %d, %s: the specular hit distance is that of the smallest non-zero sample" % (n, sm.name))
    assert differs > 100, "a mean over all N samples would have passed: the scene does not tell the two rules apart"


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. NaN, q <= 0
@pytest.mark.parametrize("backend", BACKENDS)
def test_nan_of_the_unused_lobe_and_uncounted_samples_never_reach_an_output(backend):
    """the scene holds NaN radiance, hit distance and direction wherever a sample does not count (nothing traced, q = 0, a NaN probability): every output is finite, and it is the
    output of a frame in which those samples carry the byte 255 and zeros"""
    be = Backend(backend)
    for n in (1, 2):
        s = scene(n)
        fr = frame(be, s)
        nothing = ~(LM.counted(s["lobe"], s["prob"], LM.DIFFUSE) | LM.counted(s["lobe"], s["prob"], LM.SPECULAR))
        assert np.isnan(s["rad"][nothing]).all() and np.isnan(s["dirn"][nothing]).all() and (s["lobe"][nothing] != LM.NOTHING).sum() >= 5 * n and np.isnan(s["prob"]).any()
        clean = dict(s)
        clean["lobe"], clean["rad"], clean["dirn"], clean["prob"] = s["lobe"].copy(), s["rad"].copy(), s["dirn"].copy(), s["prob"].copy()
        clean["lobe"][nothing], clean["rad"][nothing], clean["dirn"][nothing], clean["prob"][nothing] = LM.NOTHING, 0, 0, 0.5
        for dm, sm in SOME_PAIRS[:4]:
            got, _ = call_lobes(fr, dm, sm, traced(be, s), demodulate=True)
            want, _ = call_lobes(fr, dm, sm, traced(be, clean), demodulate=True)
            for rt in got:
                if got[rt].dtype == np.float16:
                    assert np.isfinite(got[rt].astype(f32)).all(), rt.name
                assert_bits(got[rt], want[rt], "N = %d %s / %s: NaN where nothing counts vs zeros and the byte 255 there: %s" % (n, dm.name, sm.name, rt.name))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. guard bytes
@pytest.mark.parametrize("backend", BACKENDS)
def test_bytes_between_rows_and_beyond_the_planes_are_untouched(backend):
    """call_lobes holds every output allocation against its stamp outside the rect; here also the inputs: nothing but the outputs is written"""
    be, s = Backend(backend), scene(2)
    fr = frame(be, s)
    t = traced(be, s, rgb=True)
    inputs = [t["lobe"], t["probability"], t["direction"], t["radiance_hit_dist"][0], t["radiance_hit_dist"][1], fr.dev["nr"], fr.dev["viewz"]]
    whole = lambda a: be.down(a if be.name == "emu" else a).copy()
    before = [whole(a) for a in inputs]
    got, allocations = call_lobes(fr, S.REBLUR_SH, S.RELAX_SH, t, demodulate=True)
    for a, b in zip(inputs, before):
        assert np.array_equal(whole(a).view(np.uint8), b.view(np.uint8))
    assert {R.IN_DIFF_SH0, R.IN_DIFF_SH1, R.IN_SPEC_SH0, R.IN_SPEC_SH1, R.IN_NORMAL_ROUGHNESS, R.IN_VIEWZ} <= set(allocations)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("backend", BACKENDS)
def test_error_table(backend):
    """one case per sentence of the header: the code, the field named in the text, nothing enqueued (every output allocation still holds its stamp)"""
    be, s = Backend(backend), scene(2)
    fr = frame(be, s)
    t = traced(be, s)
    some = frontend._fp32_plane(fr.dev["albedo"], 4, "x")
    z = frontend._fp32_plane(fr.dev["viewz"], 1, "x")

    def case(expect, field, mutate, dm=S.REBLUR_SH, sm=S.REBLUR_RADIANCE, **kw):
        text = call_lobes(fr, dm, sm, t, mutate=mutate, expect=expect, **kw)
        assert text.startswith("nrdHipPackInputsLobes: ") and field in text, (field, text)

    INV, UNS = RC.INVALID_ARGUMENT, RC.UNSUPPORTED
    # the traced planes of the descriptor must be absent: two sources
    case(INV, "diffuse.radianceHitDist", lambda d, lo: setattr(d.diffuse, "radianceHitDist", some))
    case(INV, "diffuse.direction", lambda d, lo: setattr(d.diffuse, "direction", some))
    case(INV, "specular.radianceHitDist", lambda d, lo: setattr(d.specular, "radianceHitDist", some))
    case(INV, "specular.direction", lambda d, lo: setattr(d.specular, "direction", some))
    # both signals are produced
    case(INV, "diffuse.mode", lambda d, lo: setattr(d.diffuse, "mode", 0))
    case(INV, "specular.mode", lambda d, lo: setattr(d.specular, "mode", 0))
    # the split hit-distance companions belong to the descriptor's own traced planes
    split = api.HipFrontEndSplit()
    split.diffuseHitDist = z
    case(INV, "split: diffuseHitDist", None, split=split)
    split = api.HipFrontEndSplit()
    split.specularHitDist = z
    case(INV, "split: specularHitDist", None, split=split)
    # checkerboarding is the other way to split
    case(UNS, "checkerboardMode", None, options=api.HipFrontEndOptions(int(CB.BLACK), 0))
    case(UNS, "checkerboardMode", None, options=api.HipFrontEndOptions(int(CB.WHITE), 1))
    # the struct
    case(INV, "samplesNum", lambda d, lo: setattr(lo, "samplesNum", 65))
    case(INV, "reserved", lambda d, lo: setattr(lo, "reserved", 1))
    case(INV, "lobes: lobe", lambda d, lo: setattr(lo.lobe, "data", None))
    case(UNS, "lobes: lobe", lambda d, lo: setattr(lo.lobe, "format", int(F.R8_UNORM)))
    case(UNS, "lobes: probability", lambda d, lo: setattr(lo.probability, "format", int(F.R16_SFLOAT)))
    case(INV, "lobes: radianceHitDist", lambda d, lo: setattr(lo.radianceHitDist, "data", None))
    case(INV, "lobes: direction", lambda d, lo: setattr(lo.direction, "data", None))  # REBLUR_SH reads one
    case(INV, "lobes: hitDist", lambda d, lo: setattr(lo, "hitDist", z))  # next to an RGBA32_SFLOAT plane: .w would have two sources
    case(INV, "lobes: lobe", lambda d, lo: setattr(lo.lobe, "width", s["w"] - 1))
    case(INV, "lobes: probability", lambda d, lo: setattr(lo.probability, "rowPitchBytes", lo.probability.rowPitchBytes + 2))
    case(UNS, "lobes: radianceHitDist", lambda d, lo: setattr(lo.radianceHitDist, "rowPitchBytes", 1 << 24))  # the 32-bit limits
    # layer strides, N = 2: a multiple of 16 for RGBA32_SFLOAT, of 4 for the others, and not below the plane
    case(INV, "lobes: radianceHitDistLayerBytes", lambda d, lo: setattr(lo, "radianceHitDistLayerBytes", lo.radianceHitDistLayerBytes + 8))
    case(INV, "lobes: directionLayerBytes", lambda d, lo: setattr(lo, "directionLayerBytes", 16))
    case(INV, "lobes: lobeLayerBytes", lambda d, lo: setattr(lo, "lobeLayerBytes", lo.lobeLayerBytes + 2))
    case(INV, "lobes: probabilityLayerBytes", lambda d, lo: setattr(lo, "probabilityLayerBytes", lo.probabilityLayerBytes + 2))
    t_rgb = traced(be, s, rgb=True)
    text = call_lobes(fr, S.REBLUR_SH, S.REBLUR_RADIANCE, t_rgb, mutate=lambda d, lo: setattr(lo.hitDist, "data", None), expect=INV)
    assert "lobes: hitDist" in text  # an RGB32_SFLOAT plane without its companion: no hit distance is taken as 0 silently
    text = call_lobes(fr, S.REBLUR_SH, S.REBLUR_RADIANCE, t_rgb, mutate=lambda d, lo: setattr(lo, "hitDistLayerBytes", 4), expect=INV)
    assert "lobes: hitDistLayerBytes" in text
    call_lobes(fr, S.REBLUR_SH, S.REBLUR_RADIANCE, t)  # and the unmutated call succeeds


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. lobes == NULL, symbols
@pytest.mark.parametrize("backend", BACKENDS)
def test_null_lobes_is_the_split_call(backend):
    """nrdHipPackInputsLobes( desc, options, split, NULL ) == nrdHipPackInputsSplit( desc, options, NULL, split ): plain, checkerboarded, and with three-channel planes in place"""
    be, s = Backend(backend), scene(1)
    fr = frame(be, s)
    lib = be.lib
    rad, dirn = LM.host_planes(s, LM.DIFFUSE)
    dev = dict(rad=be.up_pitched(rad[0], PAD), rad3=be.up_pitched(rad[0][..., :3], PAD), hit=be.up_pitched(rad[0][..., 3], PAD), dirn=be.up_pitched(dirn[0][..., :3], PAD))
    nr3, rough = be.up_pitched(s["nr"][..., :3], PAD), be.up_pitched(s["nr"][..., 3], PAD)
    for what, nr, rh, options in (("four channels", fr.dev["nr"], dev["rad"], None), ("checkerboarded", fr.dev["nr"], dev["rad"], api.HipFrontEndOptions(int(CB.BLACK), 1)),
                                  ("three channels in place", (nr3, rough), (dev["rad3"], dev["hit"]), None)):
        sig = dict(mode=S.REBLUR_SH, radiance_hitdist=rh, direction=dev["dirn"])
        kw = dict(diffuse=sig, specular=dict(sig, mode=S.RELAX_SH), hit_dist_params=HDP, lib=lib, in_place=True)
        results = []
        for entry in ("split", "lobes"):
            packed, desc, keep = frontend.describe_pack(nr, fr.dev["viewz"], **kw)
            for a, fmt in packed.values():
                a[...] = 7
            split = frontend.pack_split(nr, kw["diffuse"], kw["specular"])
            opt = None if options is None else C.byref(options)
            if entry == "split":
                code = lib.nrdHipPackInputsSplit(C.byref(desc), opt, None, C.byref(split), None)
            else:
                code = lib.nrdHipPackInputsLobes(C.byref(desc), opt, C.byref(split), None, None)
            assert RC(code) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()
            results.append({rt: be.down(a).copy() for rt, (a, fmt) in packed.items()})
        TPS.assert_same_planes(results[1], results[0], "nrdHipPackInputsLobes(lobes = NULL) vs nrdHipPackInputsSplit, %s" % what)


def test_symbols_structs_and_python_surface():
    """the two entry points are exported by the product library and declared by the header, the three structs are mirrored with their sizes, the wrapper is there"""
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "NRDHip.h")).read()
    for name in ("nrdHipPackInputsLobes", "nrdHipCheckHitDistCoverage"):
        assert name in api.NRD_HIP_SYMBOLS and getattr(lib, name) and "uint32_t %s(" % name in hdr
    assert "static_assert(sizeof(NrdHipFrontEndLobes) == 168" in hdr and C.sizeof(api.HipFrontEndLobes) == 168
    assert "sizeof(NrdHipCoverageDesc) == 88 && sizeof(NrdHipCoverageReport) == 28" in hdr and C.sizeof(api.HipCoverageDesc) == 88 and C.sizeof(api.HipCoverageReport) == 28
    for lobe in api.Lobe:
        assert "#define NRD_HIP_LOBE_%s %du" % (lobe.name, int(lobe)) in hdr
    for mode in api.HitDistanceReconstructionMode:  # NrdHipCoverageDesc::area is nrd::HitDistanceReconstructionMode
        assert "%s," % mode.name in open(os.path.join(ROOT, "include", "NRDSettings.h")).read()
    assert callable(frontend.pack_lobes) and callable(frontend.check_hit_dist_coverage) and "lobes" in frontend.pack_inputs.__kwdefaults__


@pytest.mark.parametrize("backend", BACKENDS)
def test_pack_inputs_routes_lobes(backend):
    """frontend.pack_inputs(lobes=...) is the C-ABI call: the same bytes as call_lobes"""
    be, s = Backend(backend), scene(2)
    fr = frame(be, s)
    t = traced(be, s)
    want, _ = call_lobes(fr, S.REBLUR_RADIANCE, S.REBLUR_RADIANCE, t)
    packed = frontend.pack_inputs(fr.dev["nr"], fr.dev["viewz"], diffuse=dict(mode=S.REBLUR_RADIANCE), specular=dict(mode=S.REBLUR_RADIANCE), hit_dist_params=HDP, lib=be.lib,
                                  lobes=dict(radiance_hit_dist=t["radiance_hit_dist"], lobe=t["lobe"], probability=t["probability"]))
    TPS.assert_same_planes({rt: be.down(a) for rt, (a, fmt) in packed.items()}, want, "frontend.pack_inputs(lobes=...)")
