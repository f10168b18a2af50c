"""nrdHipPackInputsSplit / nrdHipResolveOutputsSplit (include/NRDHip.h, raytracingdenoiser_amd/frontend.py): three-channel RGB32_SFLOAT planes with `.w` (roughness, hit distance)
in R32_SFLOAT planes of their own -- the layout a tensor host holds -- packed and resolved where they lie.

As in tests/test_pack_resolve.py every comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU). Expected values never come
from the new code: they are the bytes of the EXISTING entry points (nrdHipPackInputs / Ex / Samples, nrdHipResolveOutputs / Ex) on RGBA32_SFLOAT planes holding the same .xyz and
the companion's value in .w. Every comparison is exact. Three-channel planes and companions are carved from wider allocations: rows 5 texels longer than the plane, the base 4 bytes
past a 16-byte boundary, NaN (inputs) or a stamp (outputs) everywhere around the rect -- a 16-byte store on a 12-byte texel shows in the stamp, a 16-byte load past the last texel
of a plane in tests/cpp/split_planes_bounds.cpp, whose planes end on a page edge."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_pack_resolve as TPR
import test_pack_samples as TPS
import test_rejitter_checkerboard as TRC
from raytracingdenoiser_amd import api, build as native_build, frontend
from test_pack_resolve import BACKENDS, HDP, PACK_CALLS, Backend, assert_bits, f16, img, snorm16, unorm8, unorm16

TFH = TPR.TFH


@pytest.fixture(scope="module")
def dump():
    """the host dump of tests/cpp/frontend_check, as the `dump` fixture of tests/test_pack_resolve.py makes it -- through a file of this process's own: test files run in parallel
    worker processes, and that fixture's fixed file name is already shared by three of them"""
    TFH._build()
    path = os.path.join(os.path.dirname(TFH.EXE), "split_planes_dump_%d.bin" % os.getpid())
    r = subprocess.run([TFH.EXE, "--dump-host", path, str(TPR.COUNT)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    d = TFH._load_dump(path, TPR.COUNT)
    os.remove(path)
    return d

ROOT = TPR.ROOT
F, R, S, CB, RC, RES = api.Format, api.ResourceType, api.SignalMode, api.CheckerboardMode, api.Result, api.ResolveMode
f32 = np.float32
COUNT = TPR.COUNT
W1, H1 = 197, 61  # 12 x 197 bytes per row: the row start moves through all four 16-byte phases; a 5-pixel last workgroup column, a 1-row last row of workgroups
W0, H0 = 67, 23
STAMP = 23130
PAD = 5


# ---------------------------------------------------------------------------------------------------------------------------------------------- carved planes
class Carved:
    """an [H, W], [H, W, C], [N, H, W] or [N, H, W, C] float32 array on the backend inside a wider flat allocation: rows PAD texels longer than the plane, `gap` rows between the
    layers, the base 4 bytes past a 16-byte boundary, everything around the rect = fill"""

    def __init__(self, be, shape, channels, layers, fill, gap=3, misalign=4):
        self.be = be
        n = shape[0] if layers else 1
        h, w = shape[1:3] if layers else shape[:2]
        c = max(channels, 1)
        row, layer = (w + PAD) * c, (h + gap) * (w + PAD) * c
        size = 4 + n * layer + row
        flat = np.full(size, fill, dtype=f32)
        if be.name != "emu":
            flat = torch.from_numpy(flat).cuda()
        address = flat.ctypes.data if be.name == "emu" else flat.data_ptr()
        assert address % 4 == 0
        self.offset = ((misalign - address) % 16) // 4  # in floats: the base lands `misalign` = 4 bytes past a 16-byte boundary
        self.flat, self.fill, self.shape = flat, fill, tuple(shape)
        self.strides = ((layer,) if layers else ()) + (row, c) + ((1,) if channels else ())
        if be.name == "emu":
            self.t = np.lib.stride_tricks.as_strided(flat[self.offset:], self.shape, tuple(4 * s for s in self.strides))
            assert self.t.ctypes.data % 16 == misalign
        else:
            self.t = flat.as_strided(self.shape, self.strides, self.offset)
            assert self.t.data_ptr() % 16 == misalign

    def view_of(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.offset:], self.shape, tuple(4 * s for s in self.strides))

    def write(self, a):
        assert tuple(a.shape) == self.shape, (a.shape, self.shape)
        if self.be.name == "emu":
            self.t[...] = a
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
        return self.t

    def check_surroundings(self, what):
        """(the rect as a dense array); asserts that every float of the allocation outside the rect still holds the fill"""
        flat = np.array(self.be.down(self.flat), copy=True)
        got = np.array(self.view_of(flat), copy=True)
        want = np.full(flat.shape, self.fill, dtype=f32)
        self.view_of(want)[...] = got
        assert np.array_equal(flat.view(np.uint32), want.view(np.uint32)), "%s: bytes outside the rect were written" % what
        return got


def carve(be, a, channels=None, layers=False, gap=3):
    """numpy `a` -> its Carved copy on the backend, NaN around it"""
    a = np.ascontiguousarray(a, dtype=f32)
    if channels is None:
        channels = a.shape[-1] if a.ndim == (4 if layers else 3) else 0
    return Carved(be, a.shape, channels, layers, np.nan, gap).write(a)


def halves(be, a, layers=False):
    """an [..., 4] array as the (xyz, w) pair a tensor host holds, carved"""
    return (carve(be, a[..., :3], 3, layers), carve(be, a[..., 3], 0, layers))


# ---------------------------------------------------------------------------------------------------------------------------------------------- the pack calls
class Frame:
    """the G-buffer of tests/test_pack_resolve.py's pack tests at one size on one backend. old(): the existing entry points on four-channel planes; new(): nrdHipPackInputsSplit on
    the planes `split` names held as three-channel arrays / pairs. Both return the whole stamped output allocations."""

    def __init__(self, be, d, w, h):
        self.be, self.d, self.w, self.h = be, d, w, h
        self.ins = TPR.pack_inputs_of(d, w, h)
        self.ins["rf0"] = img(d, "Rf0", np.zeros((COUNT, 1), f32), w=w, h=h)
        self.ins["motion"][..., 3] = 0  # motion.w of an RGB32_SFLOAT plane is 0, as .zw of RG32_SFLOAT: the four-channel expectation holds the same
        self.cs = TPR.frame_settings(w, h)
        self.wide = {k: be.up_pitched(v, PAD) for k, v in self.ins.items()}
        self.pair = {k: halves(be, self.ins[k]) for k in ("nr", "rad")}
        self.three = {k: carve(be, self.ins[k][..., :3]) for k in ("direction", "albedo", "rf0", "motion")}

    def kwargs(self, dm, sm, split, full, demodulate, diff=None, spec=None):
        """(normal_roughness argument, keywords of frontend.describe_pack); split: the names of the planes held three-channel -- any of nr, diff, spec, diff_dir, spec_dir, motion,
        albedo, rf0, translucency; diff / spec: (radiance_hitdist, direction) arguments replacing the frame's own"""
        wide, pair, three = self.wide, self.pair, self.three
        pick = lambda name, a, b: a if name in split else b
        kw = dict(hit_dist_params=HDP, lib=self.be.lib)
        for which, mode, given in (("diff", dm, diff), ("spec", sm, spec)):
            if mode is not None:
                rad, dirn = given or (pick(which, pair["rad"], wide["rad"]), pick(which + "_dir", three["direction"], wide["direction"]))
                kw["diffuse" if which == "diff" else "specular"] = dict(mode=mode, radiance_hitdist=rad, direction=dirn)
        if full:
            kw.update(material_id=wide["material"], motion=pick("motion", three["motion"], wide["motion"]), distance_to_occluder=wide["occluder"],
                      translucency=pick("translucency", three["albedo"], wide["albedo"]), tan_of_light_angular_radius=TPR.TAN_LIGHT)
        if demodulate:
            kw.update(albedo=pick("albedo", three["albedo"], wide["albedo"]), rf0=pick("rf0", three["rf0"], wide["rf0"]), common_settings=self.cs)
        return pick("nr", pair["nr"], wide["nr"]), kw

    def launch(self, nr, kw, in_place, cb=CB.OFF, frame_index=0, trim=0.0, entry=None, split_struct="auto"):
        be, lib = self.be, self.be.lib
        probe = frontend.describe_pack(nr, self.wide["viewz"], in_place=in_place, **kw)[0]  # (shapes and dtypes of this call's outputs)
        out, bigs = {}, {}
        for rt, (t, fmt) in probe.items():
            name = frontend._dtype_name(t)
            view, bigs[rt] = be.padded(tuple(t.shape), name, PAD, 0x5A if name == "uint8" else STAMP)
            out[rt] = (view, fmt)
        res, desc, keep = frontend.describe_pack(nr, self.wide["viewz"], out=out, in_place=in_place, hit_dist_trim=trim, **kw)
        options = api.HipFrontEndOptions(int(cb), frame_index)
        samples = frontend.pack_samples(kw.get("diffuse"), kw.get("specular"), trim, in_place=in_place)
        if in_place:
            split = frontend.pack_split(nr, kw.get("diffuse"), kw.get("specular")) if split_struct == "auto" else split_struct
            code = lib.nrdHipPackInputsSplit(C.byref(desc), C.byref(options), C.byref(samples), None if split is None else C.byref(split), None)
        elif entry == "ex":
            code = lib.nrdHipPackInputsEx(C.byref(desc), C.byref(options), None)
        else:
            code = lib.nrdHipPackInputsSamples(C.byref(desc), C.byref(options), C.byref(samples), None)
        assert RC(code) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()
        return {rt: np.array(be.down(b), copy=True) for rt, b in bigs.items()}

    def old(self, dm, sm, full=False, demodulate=False, diff=None, spec=None, **kw):
        nr, args = self.kwargs(dm, sm, (), full, demodulate, diff, spec)
        return self.launch(nr, args, False, **kw)

    def new(self, dm, sm, split, full=False, demodulate=False, diff=None, spec=None, **kw):
        nr, args = self.kwargs(dm, sm, split, full, demodulate, diff, spec)
        return self.launch(nr, args, True, **kw)


ALL = ("nr", "diff", "spec", "diff_dir", "spec_dir", "motion", "albedo", "rf0", "translucency")


def assert_same_allocations(new, old, what):
    """every output plane and the stamps around it (the whole allocations), bit for bit"""
    assert set(new) == set(old)
    for rt in old:
        assert_bits(new[rt], old[rt], "%s: %s" % (what, rt.name))
        assert not np.array_equal(old[rt], np.full_like(old[rt], 0x5A if old[rt].dtype == np.uint8 else STAMP)), "%s was not written" % rt.name


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1. pack, every mode
@pytest.mark.parametrize("backend", BACKENDS)
def test_pack_every_mode_from_three_channel_planes(backend, dump):
    """every entry of PACK_CALLS at 197 x 61 with every fp32 colour / vector plane three-channel and both companions, the full G-buffer (motion and translucency as RGB32_SFLOAT)
    where the entry has it, and once more demodulating with RGB32_SFLOAT albedo and rf0: every output allocation equals the four-channel call's"""
    fr = Frame(Backend(backend), dump, W1, H1)
    for dm, sm, full in PACK_CALLS:
        for demodulate in (False, True):
            old = fr.old(dm, sm, full=full, demodulate=demodulate, entry="ex")
            new = fr.new(dm, sm, ALL, full=full, demodulate=demodulate)
            assert_same_allocations(new, old, "split vs RGBA32, %s / %s%s" % (dm.name, sm.name if sm else "-", ", demodulated" if demodulate else ""))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2. mixed layouts
@pytest.mark.parametrize("backend", BACKENDS)
def test_mixed_layouts_in_one_call(backend, dump):
    """normal as RGB32_SFLOAT + companion, diffuse as RGBA32_SFLOAT, specular as RGB32_SFLOAT + companion -- and each permutation of one plane flipped"""
    fr = Frame(Backend(backend), dump, W1, H1)
    base = {"nr", "spec", "spec_dir"}
    layouts = [base] + [base ^ {flip} for flip in ("nr", "diff", "spec", "diff_dir", "spec_dir")]
    for dm, sm in ((S.REBLUR_SH, S.RELAX_SH), (S.REBLUR_RADIANCE, S.REBLUR_OCCLUSION)):
        old = fr.old(dm, sm, entry="ex")
        for layout in layouts:
            if layout & {"nr", "diff", "spec", "diff_dir", "spec_dir"}:
                assert_same_allocations(fr.new(dm, sm, tuple(layout)), old, "%s / %s, three-channel: %s" % (dm.name, sm.name, sorted(layout)))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. occlusion
@pytest.mark.parametrize("backend", BACKENDS)
def test_occlusion_mode_reads_the_hit_distance_plane_alone(backend, dump):
    """REBLUR_OCCLUSION with radianceHitDist.data == NULL and only the companion, and with an RGB32_SFLOAT plane full of NaN next to it: equal to the RGBA32 occlusion call"""
    be = Backend(backend)
    fr = Frame(be, dump, W1, H1)
    old = fr.old(S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, entry="ex")
    hit = fr.pair["rad"][1]
    alone = ((None, hit), None)
    assert_same_allocations(fr.new(S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, ("nr",), diff=alone, spec=alone), old, "occlusion, hit-distance plane alone")
    _, desc, _ = frontend.describe_pack(fr.pair["nr"], fr.wide["viewz"], diffuse=dict(mode=S.REBLUR_OCCLUSION, radiance_hitdist=(None, hit)), in_place=True, lib=be.lib)
    assert not desc.diffuse.radianceHitDist.data
    unread = ((carve(be, np.full((H1, W1, 3), np.nan, f32)), hit), None)
    assert_same_allocations(fr.new(S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, ("nr",), diff=unread, spec=unread), old, "occlusion, RGB32 plane of NaN + hit distance")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. checkerboard
@pytest.mark.parametrize("backend", BACKENDS)
def test_checkerboarded_three_channel_planes(backend, dump):
    """BLACK / WHITE x frame parity at 67 x 23: equal to nrdHipPackInputsEx; the pixels that carry no data for a signal hold NaN in both the RGB32_SFLOAT plane and the companion"""
    be = Backend(backend)
    w, h = W0, H0
    fr = Frame(be, dump, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    for cb_mode in (CB.BLACK, CB.WHITE):
        for frame_index in (0, 1):
            cells = {"diff": 0, "spec": 1} if cb_mode == CB.BLACK else {"diff": 1, "spec": 0}
            sig = {}
            for which, cell in cells.items():
                has = ((((xx ^ yy) ^ frame_index) & 1) == cell)[..., None]
                sig[which] = (halves(be, np.where(has, fr.ins["rad"], f32(np.nan)).astype(f32)), carve(be, np.where(has, fr.ins["direction"][..., :3], f32(np.nan)).astype(f32)))
            for dm, sm in ((S.REBLUR_RADIANCE, S.REBLUR_RADIANCE), (S.REBLUR_SH, S.RELAX_SH), (S.REBLUR_OCCLUSION, S.RELAX_RADIANCE)):
                old = fr.old(dm, sm, entry="ex", cb=cb_mode, frame_index=frame_index)
                new = fr.new(dm, sm, ("nr",), diff=sig["diff"], spec=sig["spec"], cb=cb_mode, frame_index=frame_index)
                assert_same_allocations(new, old, "%s frame %d %s / %s" % (cb_mode.name, frame_index, dm.name, sm.name))
                for a in new.values():
                    assert not np.isnan(a.astype(f32)).any()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. samples
@pytest.mark.parametrize("backend", BACKENDS)
def test_sample_stacks_of_three_channel_layers(backend, dump):
    """N = 5 (one batch of four plus a remainder) at 197 x 61: [N, H, W, 3] stacks with [N, H, W] hit-distance stacks, layers padded with a gap between them, one REBLUR and one
    RELAX mode (both with a direction stack), trim on and off -- equal to nrdHipPackInputsSamples on the widened stack; N = 1 with no trim equals the plain split call"""
    be = Backend(backend)
    w, h, n = W1, H1, 5
    fr = Frame(be, dump, w, h)
    rad, dirn = TPS.sample_layers(dump, w, h, n)
    wide = (TPS.up_layers(be, rad, PAD, 3), TPS.up_layers(be, dirn, PAD, 3))
    three = (halves(be, rad, layers=True), carve(be, dirn[..., :3], 3, layers=True))
    assert frontend._stride0_bytes(three[0][0]) == (h + 3) * (w + PAD) * 12 and frontend._stride0_bytes(three[0][1]) == (h + 3) * (w + PAD) * 4
    for dm, sm in ((S.REBLUR_SH, S.REBLUR_RADIANCE), (S.RELAX_RADIANCE, S.RELAX_SH), (S.REBLUR_DIRECTIONAL_OCCLUSION, S.REBLUR_OCCLUSION)):
        for trim in (0.0, 0.75):
            for cb in (CB.OFF, CB.WHITE):
                old = fr.old(dm, sm, diff=wide, spec=wide, trim=trim, cb=cb, frame_index=1)
                new = fr.new(dm, sm, ("nr",), diff=three, spec=three, trim=trim, cb=cb, frame_index=1)
                assert_same_allocations(new, old, "N = 5, %s / %s, trim %.2f, %s" % (dm.name, sm.name, trim, cb.name))
    # the occlusion mode on a stack of hit-distance layers alone
    alone = ((None, three[0][1]), None)
    assert_same_allocations(fr.new(S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, ("nr",), diff=alone, spec=alone), fr.old(S.REBLUR_OCCLUSION, S.REBLUR_OCCLUSION, diff=wide, spec=wide),
                            "N = 5, occlusion on the hit-distance stack alone")
    one = ((three[0][0][:1], three[0][1][:1]), three[1][:1])
    plain = ((three[0][0][0], three[0][1][0]), three[1][0])
    assert_same_allocations(fr.new(S.REBLUR_SH, S.RELAX_SH, ("nr",), diff=one, spec=one), fr.new(S.REBLUR_SH, S.RELAX_SH, ("nr",), diff=plain, spec=plain), "N = 1 vs the plain split call")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. resolve
def resolve_inputs(be, d, w, h):
    relax, occ, dirocc = f16(img(d, "relaxPacked", w=w, h=h)), unorm16(img(d, "normHitDist", w=w, h=h)), snorm16(img(d, "dirOcc", w=w, h=h))
    up = lambda a: be.up_pitched(a, PAD)
    albedo, rf0 = img(d, "albedo", np.zeros((COUNT, 1), f32), w=w, h=h), img(d, "Rf0", np.zeros((COUNT, 1), f32), w=w, h=h)
    return dict(sh0=up(img(d, "sh0", w=w, h=h)), sh1=up(img(d, "sh1", w=w, h=h)), packed=up(img(d, "reblurPacked", w=w, h=h)), packed16=up(f16(img(d, "reblurPacked", w=w, h=h))), relax=up(relax),
                occ=up(occ), dirocc=up(dirocc), shadow=up(unorm8(img(d, "roughness", w=w, h=h))), viewz=up(img(d, "viewZ", w=w, h=h)),
                word=up(img(d, d["word"].view(f32), w=w, h=h).view(np.int32)), albedo4=up(albedo), rf04=up(rf0), albedo3=carve(be, albedo[..., :3]), rf03=carve(be, rf0[..., :3]))


def resolve_cases(p, cs):
    """the modes and resolve kinds of tests/test_pack_resolve.py's resolve tests: (name, keywords without albedo / rf0, uses albedo and rf0)"""
    common = dict(normal_roughness=p["word"], viewz=p["viewz"], common_settings=cs, hit_dist_params=HDP)
    sh = lambda md, ms, res: dict(diffuse=dict(mode=md, resolve=res, in0=p["sh0"], in1=p["sh1"]), specular=dict(mode=ms, resolve=res, in0=p["sh0"], in1=p["sh1"]))
    return [
        ("SG, remodulated, every extra output", dict(sh(S.REBLUR_SH, S.RELAX_SH, RES.SG), remodulate=True, want=("view_vector", "factors", "composed"), **common), True),
        ("SH, remodulated", dict(sh(S.RELAX_SH, S.REBLUR_SH, RES.SH), remodulate=True, want=("composed",), denormalize_hit_dist=True, **common), True),
        ("SG_EXTRACT_COLOR", dict(sh(S.REBLUR_SH, S.REBLUR_SH, RES.SG_EXTRACT_COLOR), hit_dist_params=HDP), False),
        ("REBLUR radiance fp32 / fp16, hit distances in world units", dict(diffuse=dict(mode=S.REBLUR_RADIANCE, in0=p["packed"]), specular=dict(mode=S.REBLUR_RADIANCE, in0=p["packed16"]),
                                                                        denormalize_hit_dist=True, want=("composed",), **common), False),
        ("REBLUR occlusion / RELAX radiance, shadow", dict(diffuse=dict(mode=S.REBLUR_OCCLUSION, in0=p["occ"]), specular=dict(mode=S.RELAX_RADIANCE, in0=p["relax"]), shadow=p["shadow"],
                                                           hit_dist_params=HDP), False),
        ("directional occlusion, SH", dict(diffuse=dict(mode=S.REBLUR_DIRECTIONAL_OCCLUSION, resolve=RES.SH, in0=p["dirocc"]), want=("factors",), **common), True)]


def check_split_resolve(be, w, h, kw, old, companions, what, rejitter=False):
    """frontend.resolve_outputs(channels=3) into carved, stamped outputs against the planes `old` of the four-channel call"""
    want = tuple(kw.get("want", ())) + tuple(n + "_hit_dist" for n in companions)
    probe = frontend.describe_resolve(**dict(kw, want=tuple(n for n in want if n != "rejitter_scale"), channels=3))[0]
    carved = {n: Carved(be, tuple(t.shape), 3 if t.ndim == 3 and n != "shadow" else (t.shape[2] if t.ndim == 3 else 0), False, f32(STAMP)) for n, t in probe.items()}
    if "rejitter_scale" in want:
        carved["rejitter_scale"] = Carved(be, (h, w, 2), 2, False, f32(STAMP), misalign=8)  # (RG32_SFLOAT keeps its format and its 8-byte alignment)
    res = frontend.resolve_outputs(rejitter=rejitter, **dict(kw, want=want, channels=3, out={n: c.t for n, c in carved.items()}))
    assert set(res) == set(carved)
    for n, c in carved.items():
        got = c.check_surroundings("%s: %s" % (what, n))  # the stamps between the rows and around the plane: what a 16-byte store would hit
        if n.endswith("_hit_dist"):
            assert_bits(got, be.down(old[n[:-9]])[..., 3], "%s: %s == .w" % (what, n))
        elif got.ndim == 3 and got.shape[2] == 3:
            assert_bits(got, be.down(old[n])[..., :3], "%s: %s == .rgb" % (what, n))
        else:
            assert_bits(got, be.down(old[n]), "%s: %s" % (what, n))


@pytest.mark.parametrize("backend", BACKENDS)
def test_resolve_every_mode_into_three_channel_planes(backend, dump):
    """every mode and resolve kind at 197 x 61, outputs RGB32_SFLOAT with and without the hit-distance companions, albedo and rf0 RGB32_SFLOAT"""
    be = Backend(backend)
    w, h = W1, H1
    p = resolve_inputs(be, dump, w, h)
    for name, kw, factors in resolve_cases(p, TPR.frame_settings(w, h)):
        kw = dict(kw, lib=be.lib)
        old = frontend.resolve_outputs(**dict(kw, **(dict(albedo=p["albedo4"], rf0=p["rf04"]) if factors else {})))
        new_kw = dict(kw, **(dict(albedo=p["albedo3"], rf0=p["rf03"]) if factors else {}))
        signals = [n for n in ("diffuse", "specular") if n in kw and kw[n]["mode"] != S.REBLUR_OCCLUSION]
        check_split_resolve(be, w, h, new_kw, old, signals, name + ", with companions")
        check_split_resolve(be, w, h, new_kw, old, (), name + ", hit distances dropped")
        if len(signals) == 2:
            check_split_resolve(be, w, h, new_kw, old, signals[:1], name + ", one companion")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7. re-jitter
@pytest.mark.parametrize("backend", BACKENDS)
def test_rejitter_with_three_channel_planes(backend):
    """the constructed scene of tests/test_rejitter_checkerboard.py at 67 x 23: RGB32_SFLOAT rf0 and albedo, RGB32_SFLOAT outputs -- equal to nrdHipResolveOutputsEx"""
    be, sc = Backend(backend), TRC.make_scene(W0, H0)
    p = TRC.Planes(be, sc)
    d = p.dev
    for resolve, remodulate in ((RES.SG, True), (RES.SH, False)):
        kw = dict(diffuse=dict(mode=S.REBLUR_SH, resolve=resolve, in0=d["diff_sh0"], in1=d["diff_sh1"]), specular=dict(mode=S.REBLUR_SH, resolve=resolve, in0=d["spec_sh0"], in1=d["spec_sh1"]),
                  normal_roughness=d["word"], viewz=d["viewz"], common_settings=sc["cs"], hit_dist_params=HDP, lib=be.lib, remodulate=remodulate, denormalize_hit_dist=True,
                  want=("composed", "view_vector", "factors", "rejitter_scale") if remodulate else ("rejitter_scale",))
        old = frontend.resolve_outputs(rejitter=True, rf0=d["rf0"], **dict(kw, **(dict(albedo=d["albedo"]) if remodulate else {})))
        assert (be.down(old["rejitter_scale"]) != 1.0).any()
        new_kw = dict(kw, rf0=carve(be, sc["rf0"][..., :3]), **(dict(albedo=carve(be, sc["albedo"][..., :3])) if remodulate else {}))
        check_split_resolve(be, W0, H0, new_kw, old, ("diffuse", "specular"), "re-jitter %s" % resolve.name, rejitter=True)
        check_split_resolve(be, W0, H0, new_kw, old, (), "re-jitter %s, hit distances dropped" % resolve.name, rejitter=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 8. nothing to split
@pytest.mark.parametrize("backend", BACKENDS)
def test_all_rgba32_calls_are_the_old_entry_points(backend, dump):
    """the new entry points with every plane RGBA32_SFLOAT, `split` NULL and zeroed: the bytes of the old entry points (pack: plain, checkerboarded, N = 3; resolve: plain, re-jitter)"""
    be = Backend(backend)
    w, h = W0, H0
    fr = Frame(be, dump, w, h)
    rad, dirn = TPS.sample_layers(dump, w, h, 3)
    layers = (TPS.up_layers(be, rad, PAD, 3), TPS.up_layers(be, dirn, PAD, 3))
    for dm, sm, full in PACK_CALLS[:2]:
        for kw in (dict(), dict(cb=CB.BLACK, frame_index=1), dict(diff=layers, spec=layers, trim=0.5)):
            old = fr.old(dm, sm, full=full, **kw)
            for what, s in (("NULL", None), ("zeroed", api.HipFrontEndSplit())):
                assert_same_allocations(fr.new(dm, sm, (), full=full, split_struct=s, **kw), old, "nrdHipPackInputsSplit(split = %s), all RGBA32, %s %s" % (what, dm.name, sorted(kw)))
    sc = TRC.make_scene(w, h)
    d = TRC.Planes(be, sc).dev
    kw = dict(diffuse=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=d["diff_sh0"], in1=d["diff_sh1"]), specular=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=d["spec_sh0"], in1=d["spec_sh1"]),
              normal_roughness=d["word"], viewz=d["viewz"], common_settings=sc["cs"], hit_dist_params=HDP, lib=be.lib, rf0=d["rf0"], albedo=d["albedo"], remodulate=True, want=("composed",))
    for rejitter in (False, True):
        old = frontend.resolve_outputs(rejitter=rejitter, **kw)
        res, desc, keep = frontend.describe_resolve(**kw)
        options = frontend.resolve_options(res, d["viewz"], rejitter=rejitter)
        for what, s in (("NULL", None), ("zeroed", api.HipBackEndSplit())):
            for t in res.values():
                t[...] = 0
            assert RC(be.lib.nrdHipResolveOutputsSplit(C.byref(desc), C.byref(options), None if s is None else C.byref(s), None)) == RC.SUCCESS, be.lib.nrdHipGetLastFrontEndError()
            for n in old:
                assert_bits(be.down(res[n]), be.down(old[n]), "nrdHipResolveOutputsSplit(split = %s), all RGBA32, rejitter %s: %s" % (what, rejitter, n))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 9. validation
def test_split_validation_rules_return_their_codes_without_a_device():
    """every new rule of the header comment on the real library with no GPU present: the code and a text that names the field"""
    lib = api.load_library()
    keep = []
    h, w = 32, 64
    _plane = TPR._plane
    rgb3, comp, rgba = np.zeros((4, h, w, 3), f32), np.ones((4, h, w), f32), np.zeros((h, w, 4), f32)
    keep += [rgb3, comp, rgba]
    rgb_plane = lambda: _plane(rgb3[0], F.RGB32_SFLOAT)
    comp_plane = lambda: _plane(comp[0], F.R32_SFLOAT)

    def pack(mutate, entry="split", with_samples=False):
        d = TPR._front_desc(keep, w, h)
        s = api.HipFrontEndSplit()
        smp = api.HipFrontEndSamples()
        if with_samples:
            smp.specular.samplesNum, smp.specular.radianceHitDistLayerBytes, smp.specular.directionLayerBytes = 4, h * w * 12, h * w * 12
            s.specularHitDistLayerBytes = h * w * 4
        mutate(d, s, smp)
        if entry == "split":
            code = lib.nrdHipPackInputsSplit(C.byref(d), None, C.byref(smp), C.byref(s), None)
        elif entry == "plain":
            code = lib.nrdHipPackInputs(C.byref(d), None)
        elif entry == "ex":
            code = lib.nrdHipPackInputsEx(C.byref(d), None, None)
        else:
            code = lib.nrdHipPackInputsSamples(C.byref(d), None, C.byref(smp), None)
        return RC(code), lib.nrdHipGetLastFrontEndError().decode()

    def expect(result, code, *words):
        assert result[0] == code and result[1] and all(word in result[1] for word in words), result

    def spec_rgb(d, s, smp):
        d.specular.radianceHitDist = rgb_plane()
        s.specularHitDist = comp_plane()

    def nr_rgb(d, s, smp):
        d.normalRoughness = rgb_plane()
        s.roughness = comp_plane()

    # a missing companion
    expect(pack(lambda d, s, smp: setattr(d, "normalRoughness", rgb_plane())), RC.INVALID_ARGUMENT, "split: roughness")
    expect(pack(lambda d, s, smp: setattr(d.specular, "radianceHitDist", rgb_plane())), RC.INVALID_ARGUMENT, "split: specularHitDist")
    assert RC(lib.nrdHipPackInputsSplit(C.byref(TPR._front_desc(keep, w, h)), None, None, None, None)) != RC.INVALID_ARGUMENT  # (NULL split, nothing to split: valid)
    d = TPR._front_desc(keep, w, h)
    d.normalRoughness = rgb_plane()
    assert RC(lib.nrdHipPackInputsSplit(C.byref(d), None, None, None, None)) == RC.INVALID_ARGUMENT and b"split: roughness" in lib.nrdHipGetLastFrontEndError()
    # a companion next to RGBA32_SFLOAT, or for a signal that is not there
    expect(pack(lambda d, s, smp: setattr(s, "roughness", comp_plane())), RC.INVALID_ARGUMENT, "split: roughness", "two sources")
    expect(pack(lambda d, s, smp: setattr(s, "specularHitDist", comp_plane())), RC.INVALID_ARGUMENT, "split: specularHitDist", "two sources")
    expect(pack(lambda d, s, smp: setattr(s, "diffuseHitDist", comp_plane())), RC.INVALID_ARGUMENT, "split: diffuseHitDist", "NONE")
    # the plane rules of RGB32_SFLOAT: pointer and pitch multiples of 4 (not 12, not 16), pitch >= 12 x width, the 32-bit limits
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(d.specular.radianceHitDist, "rowPitchBytes", w * 12 + 2))), RC.INVALID_ARGUMENT, "specular.radianceHitDist", "multiple of 4")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(d.specular.radianceHitDist, "data", rgb3.ctypes.data + 2))), RC.INVALID_ARGUMENT, "specular.radianceHitDist", "multiple of 4")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(d.specular.radianceHitDist, "rowPitchBytes", w * 12 - 4))), RC.INVALID_ARGUMENT, "specular.radianceHitDist", "below the row")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(d.specular.radianceHitDist, "rowPitchBytes", 1 << 24))), RC.UNSUPPORTED, "specular.radianceHitDist")
    assert pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(d.specular.radianceHitDist, "rowPitchBytes", w * 12 + 4), setattr(d.specular.radianceHitDist, "data", rgb3.ctypes.data + 4)))[0] \
        != RC.INVALID_ARGUMENT  # (4-byte steps are fine)
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(s.specularHitDist, "format", int(F.R16_SFLOAT)))), RC.UNSUPPORTED, "split: specularHitDist")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(s.specularHitDist, "width", w - 1))), RC.INVALID_ARGUMENT, "split: specularHitDist")
    # RGB32_SFLOAT on planes that do not take it
    expect(pack(lambda d, s, smp: setattr(d.viewZ, "format", int(F.RGB32_SFLOAT))), RC.UNSUPPORTED, "viewZ")
    expect(pack(lambda d, s, smp: setattr(d.specular.out0, "format", int(F.RGB32_SFLOAT))), RC.UNSUPPORTED, "specular.out0")
    # layer strides
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(smp.specular, "radianceHitDistLayerBytes", h * w * 12 + 2)), with_samples=True), RC.INVALID_ARGUMENT,
           "specular.radianceHitDistLayerBytes", "multiple of 4")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(smp.specular, "radianceHitDistLayerBytes", h * w * 12 - 4)), with_samples=True), RC.INVALID_ARGUMENT,
           "specular.radianceHitDistLayerBytes", "rowPitchBytes")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(s, "specularHitDistLayerBytes", h * w * 4 + 2)), with_samples=True), RC.INVALID_ARGUMENT, "split: specularHitDistLayerBytes", "multiple of 4")
    expect(pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(s, "specularHitDistLayerBytes", h * w * 4 - 4)), with_samples=True), RC.INVALID_ARGUMENT, "split: specularHitDistLayerBytes", "rowPitchBytes")
    expect(pack(lambda d, s, smp: setattr(smp.specular, "radianceHitDistLayerBytes", h * w * 16 + 4), with_samples=True), RC.INVALID_ARGUMENT, "specular.radianceHitDistLayerBytes", "16")  # RGBA32: unchanged
    assert pack(lambda d, s, smp: (spec_rgb(d, s, smp), setattr(smp.specular, "radianceHitDistLayerBytes", h * w * 12 + 4)), with_samples=True)[0] != RC.INVALID_ARGUMENT
    assert pack(nr_rgb)[0] != RC.INVALID_ARGUMENT and pack(spec_rgb)[0] != RC.INVALID_ARGUMENT
    # the old entry points still answer UNSUPPORTED
    for entry in ("plain", "ex", "samples"):
        expect(pack(nr_rgb, entry=entry), RC.UNSUPPORTED, "normalRoughness")
        expect(pack(spec_rgb, entry=entry), RC.UNSUPPORTED, "specular.radianceHitDist")

    # ---- back end
    sh0, sh1, out3, out4, word, z = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), np.zeros((h, w, 3), f32), np.zeros((h, w, 4), f32), np.zeros((h, w), np.int32), np.ones((h, w), f32)
    import parity
    from raytracingdenoiser_amd import synth
    persp = parity.common_settings(synth.Camera(w, h, 0), synth.Camera(w, h, 0), w, h, 0)

    def resolve(mutate, entry="split"):
        d = api.HipBackEndDesc()
        s = api.HipBackEndSplit()
        d.hitDistParams[:] = HDP
        d.specular.mode, d.specular.resolve = int(S.REBLUR_SH), int(RES.SG)
        d.specular.in0, d.specular.in1, d.specular.out = _plane(sh0, F.RGBA32_SFLOAT), _plane(sh1, F.RGBA32_SFLOAT), _plane(out3, F.RGB32_SFLOAT)
        d.normalRoughness, d.viewZ = _plane(word, F[api.NORMAL_ROUGHNESS_FORMAT_NAME]), _plane(z, F.R32_SFLOAT)
        d.commonSettings = C.cast(C.byref(persp), C.c_void_p)
        mutate(d, s)
        if entry == "split":
            code = lib.nrdHipResolveOutputsSplit(C.byref(d), None, C.byref(s), None)
        elif entry == "plain":
            code = lib.nrdHipResolveOutputs(C.byref(d), None)
        else:
            code = lib.nrdHipResolveOutputsEx(C.byref(d), None, None)
        return RC(code), lib.nrdHipGetLastFrontEndError().decode()

    assert resolve(lambda d, s: None)[0] != RC.INVALID_ARGUMENT and resolve(lambda d, s: setattr(s, "specularHitDist", comp_plane()))[0] != RC.INVALID_ARGUMENT
    expect(resolve(lambda d, s: None, entry="plain"), RC.UNSUPPORTED, "specular.out")
    expect(resolve(lambda d, s: None, entry="ex"), RC.UNSUPPORTED, "specular.out")
    expect(resolve(lambda d, s: (setattr(d.specular, "out", _plane(out4, F.RGBA32_SFLOAT)), setattr(s, "specularHitDist", comp_plane()))), RC.INVALID_ARGUMENT, "split: specularHitDist", "two sources")
    expect(resolve(lambda d, s: setattr(s, "diffuseHitDist", comp_plane())), RC.INVALID_ARGUMENT, "split: diffuseHitDist", "NONE")
    expect(resolve(lambda d, s: setattr(d.specular.out, "rowPitchBytes", w * 12 + 2)), RC.INVALID_ARGUMENT, "specular.out", "multiple of 4")
    expect(resolve(lambda d, s: setattr(d.specular.out, "rowPitchBytes", w * 12 - 4)), RC.INVALID_ARGUMENT, "specular.out", "below the row")
    expect(resolve(lambda d, s: setattr(d.specular.in0, "format", int(F.RGB32_SFLOAT))), RC.UNSUPPORTED, "specular.in0")
    expect(resolve(lambda d, s: setattr(d, "outShadow", _plane(out3, F.RGB32_SFLOAT))), RC.INVALID_ARGUMENT, "shadow")  # (no shadow plane; and with one, outShadow keeps its formats:)
    shadow = np.zeros((h, w, 4), np.uint8)
    expect(resolve(lambda d, s: (setattr(d, "shadow", _plane(shadow, F.RGBA8_UNORM)), setattr(d, "outShadow", _plane(out3, F.RGB32_SFLOAT)))), RC.UNSUPPORTED, "outShadow")

    def occlusion(d, s):
        d.specular.mode = int(S.REBLUR_OCCLUSION)
        d.specular.in0, d.specular.out = _plane(np.zeros((h, w), np.uint16), F.R16_UNORM), _plane(z, F.R32_SFLOAT)
        s.specularHitDist = comp_plane()
    expect(resolve(occlusion), RC.INVALID_ARGUMENT, "split: specularHitDist", "R32_SFLOAT")
    opt = api.HipBackEndOptions()
    opt.outReJitterScale = _plane(out3, F.RGB32_SFLOAT)
    opt.reJitter = 1
    d = api.HipBackEndDesc()
    assert RC(lib.nrdHipResolveOutputsSplit(C.byref(d), C.byref(opt), None, None)) == RC.INVALID_ARGUMENT and lib.nrdHipGetLastFrontEndError()
    assert RC(lib.nrdHipResolveOutputsSplit(None, None, None, None)) == RC.INVALID_ARGUMENT and RC(lib.nrdHipPackInputsSplit(None, None, None, None, None)) == RC.INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------------------------- 10. the Python surface
def test_symbols_structs_header_and_integration_class():
    lib = api.load_library()
    for name in ("nrdHipPackInputsSplit", "nrdHipResolveOutputsSplit"):
        assert name in api.NRD_HIP_SYMBOLS and getattr(lib, name)
    assert (C.sizeof(api.HipFrontEndSplit), C.sizeof(api.HipBackEndSplit)) == (88, 48)
    hdr = open(os.path.join(ROOT, "include", "NRDHip.h")).read()
    assert "uint32_t nrdHipPackInputsSplit(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, const NrdHipFrontEndSplit* split, void* hipStream);" in hdr
    assert "uint32_t nrdHipResolveOutputsSplit(const NrdHipBackEndDesc* desc, const NrdHipBackEndOptions* options, const NrdHipBackEndSplit* split, void* hipStream);" in hdr
    assert "sizeof(NrdHipFrontEndSplit) == 88 && sizeof(NrdHipBackEndSplit) == 48" in hdr
    hpp = open(os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")).read()
    assert "const NrdHipFrontEndSplit& split" in hpp and "const NrdHipBackEndSplit& split" in hpp
    from raytracingdenoiser_amd.executor import HipExecutor

    assert "channels=3" in HipExecutor.resolve.__doc__ and callable(frontend.rgba)


@pytest.mark.parametrize("backend", BACKENDS)
def test_python_surface_packs_and_resolves_in_place(backend, dump, monkeypatch):
    """with frontend.rgba unusable, pack_inputs(in_place=True) on pairs, on three-channel arrays and on a [5, H, W, 3] stack succeeds -- through a raw stream handle as well -- and
    returns the bytes of the four-channel call; resolve_outputs(channels=3) returns the documented shapes; the in-place describe_pack descriptor relaunched after the caller
    overwrote its three-channel tensor packs the NEW values"""
    be = Backend(backend)
    w, h = W0, H0
    fr = Frame(be, dump, w, h)
    rad, dirn = TPS.sample_layers(dump, w, h, 5)
    wide_layers = (be.up(rad), be.up(dirn))
    mode = S.REBLUR_SH
    nr4, kw4 = fr.kwargs(mode, mode, (), True, True)
    want = frontend.pack_inputs(nr4, fr.wide["viewz"], **kw4)
    want_layers = frontend.pack_inputs(nr4, fr.wide["viewz"], **dict(kw4, diffuse=dict(mode=mode, radiance_hitdist=wide_layers[0], direction=wide_layers[1]),
                                                                     specular=dict(mode=mode, radiance_hitdist=wide_layers[0], direction=wide_layers[1])))

    def no_rgba(*a, **k):
        raise AssertionError("frontend.rgba was called: a widened copy")
    monkeypatch.setattr(frontend, "rgba", no_rgba)
    nr3, kw3 = fr.kwargs(mode, mode, ALL, True, True)
    raw_stream = 0 if backend == "emu" else torch.cuda.current_stream().cuda_stream
    for stream in (None, raw_stream):
        got = frontend.pack_inputs(nr3, fr.wide["viewz"], in_place=True, stream=stream, **kw3)
        for rt in want:
            assert_bits(be.down(got[rt][0]), be.down(want[rt][0]), "pack_inputs(in_place=True, stream=%r): %s" % (stream, rt.name))
        stack = dict(mode=mode, radiance_hitdist=(be.up(rad[..., :3]), be.up(rad[..., 3])), direction=be.up(dirn[..., :3]))
        got = frontend.pack_inputs(nr3, fr.wide["viewz"], in_place=True, stream=stream, **dict(kw3, diffuse=stack, specular=stack))
        for rt in want_layers:
            assert_bits(be.down(got[rt][0]), be.down(want_layers[rt][0]), "pack_inputs(in_place=True) on a [5, H, W, 3] stack: %s" % rt.name)
    # the descriptor points at the caller's arrays: a relaunch packs what they hold then
    normal, rough = be.up(fr.ins["nr"][..., :3]), be.up(fr.ins["nr"][..., 3])
    sig = dict(mode=S.RELAX_RADIANCE, radiance_hitdist=(be.up(fr.ins["rad"][..., :3]), be.up(fr.ins["rad"][..., 3])))
    res, desc, keep = frontend.describe_pack((normal, rough), fr.wide["viewz"], diffuse=sig, in_place=True, lib=be.lib)
    split, samples = frontend.pack_split((normal, rough), sig), frontend.pack_samples(sig, in_place=True)
    launch = lambda: be.lib.nrdHipPackInputsSplit(C.byref(desc), None, C.byref(samples), C.byref(split), None)
    assert RC(launch()) == RC.SUCCESS
    first = {rt: np.array(be.down(t), copy=True) for rt, (t, fmt) in res.items()}
    fresh = np.roll(fr.ins["rad"], 7, axis=1)
    sig["radiance_hitdist"][0][...] = be.up(fresh[..., :3])
    sig["radiance_hitdist"][1][...] = be.up(fresh[..., 3])
    assert RC(launch()) == RC.SUCCESS
    monkeypatch.undo()
    fresh_want = frontend.pack_inputs(be.up(fr.ins["nr"]), fr.wide["viewz"], diffuse=dict(mode=S.RELAX_RADIANCE, radiance_hitdist=be.up(fresh)), lib=be.lib)
    rt = R.IN_DIFF_RADIANCE_HITDIST
    assert_bits(be.down(res[rt][0]), be.down(fresh_want[rt][0]), "the relaunched in-place descriptor packs the refreshed tensor")
    assert not np.array_equal(first[rt], be.down(res[rt][0]))
    # resolve_outputs(channels=3): the documented shapes
    p = resolve_inputs(be, dump, w, h)
    out = frontend.resolve_outputs(diffuse=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=p["sh0"], in1=p["sh1"]), specular=dict(mode=S.RELAX_SH, resolve=RES.SG, in0=p["sh0"], in1=p["sh1"]),
                                   normal_roughness=p["word"], viewz=p["viewz"], common_settings=TPR.frame_settings(w, h), albedo=p["albedo3"], rf0=p["rf03"], remodulate=True, lib=be.lib,
                                   want=("composed", "view_vector", "factors", "diffuse_hit_dist", "specular_hit_dist"), channels=3)
    assert {n: tuple(t.shape) for n, t in out.items()} == dict({n: (h, w, 3) for n in ("diffuse", "specular", "composed", "view_vector", "diff_factor", "spec_factor")},
                                                               diffuse_hit_dist=(h, w), specular_hit_dist=(h, w))
    default = frontend.resolve_outputs(diffuse=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=p["sh0"], in1=p["sh1"]), hit_dist_params=HDP, normal_roughness=p["word"], viewz=p["viewz"],
                                       common_settings=TPR.frame_settings(w, h), lib=be.lib)
    assert tuple(default["diffuse"].shape) == (h, w, 4)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 11. bounds (CPU only)
def test_last_texel_on_a_page_edge():
    """tests/cpp/split_planes_bounds.cpp against the emulation library: every RGB32_SFLOAT plane and companion ends on the last byte of a page in front of an inaccessible one;
    pack, samples (N = 5), resolve and re-jitter run and the program exits 0 (a 16-byte access on the last 12-byte texel would end it with SIGSEGV)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from emu import build_emu

    lib = build_emu.build()
    src = os.path.join(ROOT, "tests", "cpp", "split_planes_bounds.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "build", "split_planes_bounds" + api.ENCODING_SUFFIX)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not (os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(src), os.path.getmtime(lib))):
        cmd = [build_emu.CLANG, "-std=c++17", "-O1", "-Wno-attributes", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, lib, "-fopenmp", "-Wl,-rpath," + os.path.dirname(lib)]
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "split planes bounds OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------------------------------- 12. the C++ class
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "split_planes_integration.cpp")
CPP_EXE = os.path.join(ROOT, "tests", "cpp", "build", "split_planes_integration")


def _build_cpp():
    """as tests/test_pack_samples.py builds its program: g++, the installed headers, libNRD_hip.so"""
    lib = native_build.build_product()
    os.makedirs(os.path.dirname(CPP_EXE), exist_ok=True)
    hpp = os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")
    if os.path.exists(CPP_EXE) and os.path.getmtime(CPP_EXE) > max(os.path.getmtime(CPP_SRC), os.path.getmtime(lib), os.path.getmtime(hpp)):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-attributes", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", CPP_SRC, "-o", CPP_EXE,
           "-L" + os.path.dirname(lib), "-lNRD_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../../../raytracingdenoiser_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_cpp_overloads_compile_and_validate_on_the_host():
    _build_cpp()
    r = subprocess.run([CPP_EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host-only OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_overloads_pack_and_resolve_split_planes():
    _build_cpp()
    r = subprocess.run([CPP_EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "split pack vs RGBA32 pack: 0 mismatching values" in r.stdout and "split resolve vs RGBA32 resolve: 0 wrong values" in r.stdout and \
        "split planes integration OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------------- 13. static facts
def test_static_facts_of_the_split_twins():
    """what the compiler made of the twins for gfx950 (tools/frontend_bench.py split_isa(), the `isa_split` object of profiles/frontend_bench.json): no scratch anywhere, no LDS in the
    pack and resolve twins, 12-byte loads in the pack families and 12-byte stores in the resolve families. isa() returns what it returned: the plain kernels are untouched."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import json

    import frontend_bench

    facts = frontend_bench.split_isa()
    assert set(facts) == {"pack_split", "pack_checkerboard_split", "pack_samples_split", "pack_samples_checkerboard_split", "resolve_split", "rejitter_split"}
    for name, k in facts.items():
        print(name, k)
        assert k["scratch_bytes"] == 0 and k["vgprs"] > 0 and k["waves_per_simd"] >= 1, (name, k)
        if name != "rejitter_split":
            assert k["lds_bytes"] == 0, (name, k)
        if name.startswith("pack"):
            assert k["global_load_dwordx3"] > 0 and k["global_store_dwordx3"] == 0, (name, k)
        else:
            assert k["global_store_dwordx3"] > 0, (name, k)
    recorded = json.load(open(os.path.join(ROOT, "profiles", "frontend_bench.json")))["isa"]
    assert frontend_bench.isa() == recorded
