"""nrdHipPackGuides (include/NRDHip.h, raytracingdenoiser_amd/frontend.py): IN_VIEWZ and IN_MV derived on the device from world-space positions and the matrices of
nrd::CommonSettings, and the four optional UNORM guide slots encoded from fp32 planes.

As in tests/test_shadow_lights.py every kernel comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU). Expected values
never come from the code under test:
  M   tests/guides_model.py pack(): a float32 numpy restatement of the header text -- bit for bit, no tolerance
  E64 tests/guides_model.py exact(): float64 from the raw matrices -- within the rounding budget derived at test_against_float64
  S   synth.render_frame(want="mv2d"): the repository's independent statement of the same convention
Inputs live in wider allocations whose surroundings are NaN; outputs in stamped ones that are compared whole."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import guides_model as M
import parity
import test_pack_resolve as TPR
from raytracingdenoiser_amd import api, build as native_build, frontend, synth
from test_pack_resolve import BACKENDS, Backend, assert_bits, f16, unorm8

ROOT = TPR.ROOT
F, R, RC = api.Format, api.ResourceType, api.Result
f32 = np.float32
W1, H1 = 197, 61  # a 5-pixel last workgroup column, a 1-row last row of workgroups
W0, H0 = 67, 23   # odd; a dense RGB32_SFLOAT row is 804 bytes: a multiple of 4 and of nothing more
PAD, GAP = 5, 3
STAMP16, STAMP8, STAMP32 = 23130, 0x5A, 7.5
MISS = f32(1e6)
ROW_NAN, ROW_INF, ROW_PREV_NAN, ROW_BEHIND, ROW_OVERFLOW = 0, 1, 2, 3, 4  # the rows the special cases of the issue are planted in
MODES = {"2.5d": (False, lambda w, h: (1.0 / w, 1.0 / h, 1.0)), "2d": (False, lambda w, h: (1.0 / w, 1.0 / h, 0.0)), "world": (True, lambda w, h: (1e-3, 2e-3, 5e-4)),
         "world0": (True, lambda w, h: (0.0, 0.0, 0.0))}


# ---------------------------------------------------------------------------------------------------------------------------------------------- inputs
def right_handed(cam):
    """the same camera with view z pointing backwards: row 2 of world-to-view and column 2 of view-to-clip negated (column-major lists)"""
    out = synth.Camera(cam.width, cam.height, 0)
    out.__dict__.update(cam.__dict__)
    out.world_to_view = [-v if i % 4 == 2 else v for i, v in enumerate(cam.world_to_view)]
    out.view_to_clip = [-v if 8 <= i < 12 else v for i, v in enumerate(cam.view_to_clip)]
    return out


def settings(w, h, mode, handed="lh", frames=(8, 0), **kw):
    """CommonSettings of the synthetic camera at frame frames[0] with the one of frames[1] as the previous frame: under 4 pixels of motion for the scenes below"""
    cam, cam_prev = synth.Camera(w, h, frames[0]), synth.Camera(w, h, frames[1])
    if handed == "rh":
        cam, cam_prev = right_handed(cam), right_handed(cam_prev)
    world, scale = MODES[mode]
    kw = dict(dict(isMotionVectorInWorldSpace=world, motionVectorScale=scale(w, h)), **kw)
    return parity.common_settings(cam, cam_prev, w, h, 1, **kw), synth.Camera(w, h, frames[0]), synth.Camera(w, h, frames[1])


def scene(w, h, cam, cam_prev, seed=0, plant=True):
    """position, position_prev [h, w, 4] float32 (.w = NaN: never read): points 2 .. 12 units in front of the camera, |X| <= 20, the surface moved by up to a centimetre; with
    `plant` the special cases of the issue in rows 0 .. 4"""
    rng = np.random.RandomState(seed)
    z = rng.uniform(2.0, 12.0, (h, w))
    view = np.stack([rng.uniform(-0.6, 0.6, (h, w)) * z, rng.uniform(-0.25, 0.25, (h, w)) * z, z], -1)
    rot = np.array([cam.right, cam.up, cam.fwd], np.float64)
    X = (view @ rot + np.array(cam.pos, np.float64)).astype(f32)
    Xp = (X + rng.uniform(-0.01, 0.01, (h, w, 3))).astype(f32)
    assert np.abs(X).max() <= 20 and np.abs(Xp).max() <= 20
    if plant:
        X[ROW_NAN, :, 0] = np.nan
        X[ROW_INF, :, 1] = np.inf
        X[ROW_INF, ::2, 1] = -np.inf
        Xp[ROW_PREV_NAN, :, 2] = np.nan
        Xp[ROW_PREV_NAN, ::3, 0] = np.inf
        Xp[ROW_BEHIND] = (np.array(cam_prev.pos) - 5.0 * np.array(cam_prev.fwd) + rng.uniform(-1, 1, (w, 3))).astype(f32)
        Xp[ROW_OVERFLOW] = (np.array(cam_prev.pos) + 0.001 * np.array(cam_prev.fwd) + 1000.0 * np.array(cam_prev.right)).astype(f32)
    nan = np.full((h, w, 1), np.nan, f32)
    return np.concatenate([X, nan], -1), np.concatenate([Xp, nan], -1)


def up_pad(be, a, pad=PAD, gap=GAP):
    """[H, W(, C)] on the backend inside a wider allocation: rows `pad` texels longer, `gap` rows more, everything around the rect NaN"""
    h, w = a.shape[:2]
    big = np.full((h + gap, w + pad) + a.shape[2:], np.nan, dtype=a.dtype)
    big[:h, :w] = a
    big = big if be.name == "emu" else torch.from_numpy(big).cuda()
    return big[:h, :w]


def xyz_plane(be, a, channels, w):
    """the position as RGBA32_SFLOAT (padded rows) or RGB32_SFLOAT -- at the odd width dense, so that the row pitch is a multiple of 4 only"""
    a = np.ascontiguousarray(a[..., :channels])
    return up_pad(be, a, pad=0 if channels == 3 and w == W0 else PAD)


def assert_whole(be, big, got, stamp, what):
    """no byte outside the output rect changed"""
    whole = be.down(big)
    want = np.full(whole.shape, stamp, dtype=whole.dtype)
    want[:got.shape[0], :got.shape[1]] = got
    assert np.array_equal(np.ascontiguousarray(whole).view(np.uint8), want.view(np.uint8)), "bytes outside the rect were written: " + what


OUT_PLANES = {R.IN_VIEWZ: ((), "float32", STAMP32, F.R32_SFLOAT), R.IN_MV: ((4,), "float16", STAMP16, F.RGBA16_SFLOAT), R.IN_BASECOLOR_METALNESS: ((4,), "uint8", STAMP8, F.RGBA8_UNORM),
              R.IN_DIFF_CONFIDENCE: ((), "uint8", STAMP8, F.R8_UNORM), R.IN_SPEC_CONFIDENCE: ((), "uint8", STAMP8, F.R8_UNORM), R.IN_DISOCCLUSION_THRESHOLD_MIX: ((), "uint8", STAMP8, F.R8_UNORM)}


def pack(be, w, h, slots, position=None, cs=None, position_prev=None, **kw):
    """one nrdHipPackGuides launch through the C-ABI into stamped, padded outputs; returns {slot: downloaded plane}. Every output allocation is held against its stamp."""
    out, bigs = {}, {}
    for slot in slots:
        tail, dtype, stamp, fmt = OUT_PLANES[slot]
        view, bigs[slot] = be.padded((h, w) + tail, dtype, PAD, stamp)
        out[slot] = (view, fmt)
    want = tuple(name for name, slot in (("viewz", R.IN_VIEWZ), ("mv", R.IN_MV)) if slot in slots)
    res, desc, keep = frontend.describe_pack_guides(position, cs, position_prev, miss_viewz=float(MISS), out=out, lib=be.lib, want=want or ("viewz", "mv"), **kw)
    assert set(res) == set(out), (set(res), set(out))
    code = be.lib.nrdHipPackGuides(C.byref(desc), None)
    assert RC(code) == RC.SUCCESS, be.lib.nrdHipGetLastFrontEndError()
    got = {slot: be.down(t).copy() for slot, (t, fmt) in res.items()}
    for slot, big in bigs.items():
        assert_whole(be, big, got[slot], np.array(OUT_PLANES[slot][2]).astype(got[slot].dtype), str(slot))
    return got


COMBOS = [(pc, prev) for pc in (4, 3) for prev in (None, 4, 3)]  # channels of position, of positionPrev (None: absent): the six instantiations with a position


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", list(MODES))
def test_bit_for_bit_against_the_model(backend, mode):
    """screen-space 2.5D, 2D (.z stored as 0), world space and world space with s = (0, 0, 0) (everything stored as 0); position as RGBA32_SFLOAT and RGB32_SFLOAT, with and
    without positionPrev in either format, a left-handed and a right-handed camera pair, 197 x 61 and 67 x 23. Planted: NaN and INF positions (the miss path), a non-finite
    positionPrev at a hit (the static path), a point behind the previous camera (99999, then the clamp), a motion that overflows fp16, .w = NaN everywhere. No tolerance."""
    be = Backend(backend)
    for w, h in ((W1, H1), (W0, H0)):
        left = {}
        for handed in ("lh", "rh"):
            cs, cam, cam_prev = settings(w, h, mode, handed)
            X, Xp = scene(w, h, cam, cam_prev, seed=len(mode) + w)
            for pc, prev in COMBOS:
                want_z, want_mv = M.pack(cs, X, Xp if prev else None, MISS)
                got = pack(be, w, h, (R.IN_VIEWZ, R.IN_MV), xyz_plane(be, X, pc, w), cs, xyz_plane(be, Xp, prev, w) if prev else None)
                what = "%s %s %dx%d position x%d prev %s: " % (mode, handed, w, h, pc, prev)
                # Not through the model: the passes take abs( IN_VIEWZ ) and flip a right-handed pair of matrices to the left-handed one themselves, so the right-handed twin
                # of a camera pair must get the very vectors of the left-handed pair -- .z included -- and the negated depth (the miss depth is the caller's number)
                if handed == "lh":
                    left[pc, prev] = got
                else:
                    assert_bits(got[R.IN_MV], left[pc, prev][R.IN_MV], what + "IN_MV == the left-handed pair's")
                    assert_bits(got[R.IN_VIEWZ][2:], -left[pc, prev][R.IN_VIEWZ][2:], what + "IN_VIEWZ == - the left-handed pair's")
                assert_bits(got[R.IN_VIEWZ], want_z, what + "IN_VIEWZ vs M")
                assert_bits(got[R.IN_MV], f16(want_mv), what + "IN_MV vs M")
                mv = got[R.IN_MV].astype(f32)
                assert np.isfinite(mv).all() and (mv[..., 3] == 0).all()
                assert (got[R.IN_VIEWZ][[ROW_NAN, ROW_INF]] == MISS).all() and (mv[[ROW_NAN, ROW_INF]] == 0).all()
                assert ((got[R.IN_VIEWZ][2:] > 0) == (handed == "lh")).all()  # IN_VIEWZ has the sign of the caller's convention
                if mode == "world0" or (prev is None and mode == "world"):
                    assert (mv == 0).all()
                if mode == "2d":
                    assert (mv[..., 2] == 0).all()
                if prev and mode in ("2.5d", "2d"):
                    assert (np.abs(mv[ROW_BEHIND, :, :2]) == 65504).all(), "behind the previous camera: 99999 / s, clamped"
                    assert (np.abs(mv[ROW_OVERFLOW, :, 0]) == 65504).all(), "a motion beyond fp16"
                if prev and mode == "world":
                    assert (np.abs(mv[ROW_OVERFLOW]).max(-1) == 65504).all(), "a motion beyond fp16"
                if prev and mode != "world0":  # a non-finite positionPrev is the static point: the vector of the call without positionPrev
                    static = M.pack(cs, X, None, MISS)[1]
                    assert_bits(got[R.IN_MV][ROW_PREV_NAN], f16(static)[ROW_PREV_NAN], what + "non-finite positionPrev == static")
            # each output alone: the other is not written, the bytes are the same
            alone = pack(be, w, h, (R.IN_VIEWZ,), xyz_plane(be, X, 3, w), cs, None)
            assert_bits(alone[R.IN_VIEWZ], want_z, "outViewZ alone")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2. float64
def ulp16(x):
    """spacing of fp16 at |x| (denormals: 2^-24)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 10)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["2.5d", "2d", "world"])
def test_against_float64(backend, mode):
    """The same scenes without the planted rows (|X| <= 20, motion under 4 pixels), the projection evaluated in float64 from the raw matrices: a model and a kernel that share a
    wrong reading fail here. Bound: |stored - exact| <= ulp16( exact ) / 2 + E.
    Derivation of E. The stored fp16 value is the fp32 result rounded once: half an fp16 ulp. The fp32 result differs from the exact one by the roundings on the way: a uv
    is a number near 1 (|uv| <= 1.02 for these scenes), one fp32 rounding of it is at most 2^-24, and the chain camera-relative subtraction, three-term rotation, projection,
    division, scale and bias, for the two frames, then the difference, is 16 roundings that reach the uv at a gain of about one: 16 * 2^-24 in uv units, times max( w, h )
    after the division by s = ( 1 / w, 1 / h ): E = 16 * 2^-24 * max( w, h ) pixels. For .z the same count of roundings applies to numbers as large as the largest |viewZ|:
    E_z = 16 * 2^-24 * max |viewZ|. World-space vectors are one subtraction and one division of the inputs: far inside the same E."""
    be = Backend(backend)
    for w, h in ((W1, H1), (W0, H0)):
        for handed in ("lh", "rh"):
            cs, cam, cam_prev = settings(w, h, mode, handed)
            X, Xp = scene(w, h, cam, cam_prev, seed=3 + w, plant=False)
            for pc, prev in ((4, 3), (3, None)):
                z64, mv64 = M.exact(cs, X, Xp if prev else None)
                if mode != "world":
                    assert np.abs(mv64[..., :2]).max() < 4.0, "the scenes of this test move by less than 4 pixels"
                got = pack(be, w, h, (R.IN_VIEWZ, R.IN_MV), xyz_plane(be, X, pc, w), cs, xyz_plane(be, Xp, prev, w) if prev else None)
                E = 16.0 * 2.0 ** -24 * max(w, h)
                Ez = 16.0 * 2.0 ** -24 * np.abs(z64).max()
                err = np.abs(got[R.IN_MV][..., :3].astype(np.float64) - mv64) - ulp16(mv64) / 2
                print("%s %s %dx%d prev %s: worst excess over the fp16 half-ulp: xy %.3g (E %.3g), z %.3g (Ez %.3g)" % (mode, handed, w, h, prev, err[..., :2].max(), E, err[..., 2].max(), Ez))
                assert err[..., :2].max() <= E and err[..., 2].max() <= Ez
                assert np.abs(got[R.IN_VIEWZ] - z64).max() <= Ez
                assert (got[R.IN_MV][..., 3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. synth
SYNTH_W, SYNTH_H = 192, 128


@pytest.fixture(scope="module")
def synth_frames():
    """frames 1 .. 3 of the moving camera at 192 x 128 with the raw values and synth's own screen-space vectors: (frame, CommonSettings for s = (1 / w, 1 / h, 1))"""
    w, h = SYNTH_W, SYNTH_H
    out = []
    for f in (1, 2, 3):
        frame = synth.render_frame(w, h, f, want=("raw", "mv2d"))
        cs = parity.common_settings(frame["camera"], synth.Camera(w, h, f - 1), w, h, f, isMotionVectorInWorldSpace=False, motionVectorScale=(1.0 / w, 1.0 / h, 1.0))
        out.append((frame, cs))
    return out


def synth_budget(synth_frames):
    """E of test_against_float64 for this frame size, or twice what the reference pair -- the float64 model against synth's own planes -- shows beyond the fp16 half-ulp, if more"""
    w, h = SYNTH_W, SYNTH_H
    E, shown = 16.0 * 2.0 ** -24 * max(w, h), 0.0
    for frame, cs in synth_frames:
        hit = ~frame["is_sky"].numpy()
        z64, mv64 = M.exact(cs, frame["raw"]["position"].numpy())
        mv = frame["mv"].numpy().astype(np.float64)[..., :3]
        shown = max(shown, float((np.abs(mv - mv64) - ulp16(mv64) / 2)[hit].max()))
    return max(E, 2.0 * shown), shown, E


def test_float64_model_against_synth(synth_frames):
    """the reference pair on the CPU: float64 exact() against synth's fp16 vectors on the non-sky pixels. Measured: the pair differs by 3.43e-4 beyond the fp16 half-ulp
    (pixels / view-depth units; synth computes in float32, absolute coordinates, from the same rounded position) where E = 16 * 2^-24 * 192 = 1.83e-4: the pair itself
    exceeds E, so the budget of the test below is twice what it shows, 6.86e-4 (synth_budget computes it from the two references, never from the code under test)"""
    budget, shown, E = synth_budget(synth_frames)
    print("float64 model vs synth: %.3g beyond the fp16 half-ulp, E = %.3g, budget %.3g" % (shown, E, budget))
    assert shown <= 1e-2  # two statements of one convention: a sign or a unit apart would show as pixels, not as roundings


@pytest.mark.parametrize("backend", BACKENDS)
def test_against_synth(backend, synth_frames):
    """outMv equals synth's mv within one fp16 ulp of the larger value plus the budget, outViewZ equals viewz within 8 * 2^-24 * |viewz|, on every non-sky pixel; on the sky the
    motion is 0 and the depth is missViewZ"""
    be = Backend(backend)
    w, h = SYNTH_W, SYNTH_H
    budget, shown, E = synth_budget(synth_frames)
    for frame, cs in synth_frames:
        sky = frame["is_sky"].numpy()
        assert sky.any() and (~sky).any()
        position = frame["raw"]["position"].numpy()
        assert np.isnan(position[sky]).all()
        got = pack(be, w, h, (R.IN_VIEWZ, R.IN_MV), up_pad(be, np.ascontiguousarray(position)), cs, None)
        mv, want = got[R.IN_MV].astype(np.float64), frame["mv"].numpy().astype(np.float64)
        viewz = frame["viewz"].numpy().astype(np.float64)
        err = np.abs(mv - want) - ulp16(np.maximum(np.abs(mv), np.abs(want)))
        zerr = np.abs(got[R.IN_VIEWZ] - viewz) / np.abs(viewz)
        print("frame %d: worst excess over one fp16 ulp %.3g (budget %.3g), viewZ relative %.3g (allowed %.3g)" % (cs.frameIndex, err[~sky].max(), budget, zerr[~sky].max(), 8 * 2.0 ** -24))
        assert err[~sky].max() <= budget
        assert zerr[~sky].max() <= 8 * 2.0 ** -24
        assert (mv[sky] == 0).all() and (got[R.IN_VIEWZ][sky] == MISS).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. UNORM slots
def saturate_hlsl(a):
    return np.clip(np.where(np.isnan(a), f32(0), a), 0, 1).astype(f32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_unorm_slots_against_the_model(backend):
    """IN_BASECOLOR_METALNESS, IN_DIFF_CONFIDENCE, IN_SPEC_CONFIDENCE, IN_DISOCCLUSION_THRESHOLD_MIX: every code 0 .. 255 occurs, with the values -0.25, 1.25 and NaN;
    floor( saturate( x ) * 255 + 0.5 ) with saturate( NaN ) = 0, bit for bit. Base colour as RGBA32_SFLOAT (.w = NaN, never read) and as RGB32_SFLOAT; with and without the
    position outputs in the same launch"""
    be = Backend(backend)
    for w, h in ((W1, H1), (W0, H0)):
        rng = np.random.RandomState(w)
        planes = rng.uniform(-0.05, 1.05, (6, h, w)).astype(f32)
        ramp = (np.arange(256) / 255.0).astype(f32)
        for p in planes:
            p[5, :w] = np.resize(ramp, w)
            p[6:10] = np.resize(np.concatenate([ramp, (ramp + f32(0.49 / 255)).astype(f32), (ramp - f32(0.49 / 255)).astype(f32)]), (4, w))
            p[10, 0::3], p[10, 1::3], p[10, 2::3] = -0.25, 1.25, np.nan
        base = np.concatenate([np.moveaxis(planes[:3], 0, -1), np.full((h, w, 1), np.nan, f32)], -1)
        metal, diff, spec, mix = planes[3], planes[4], planes[5], planes[3][::-1].copy()
        want = {R.IN_BASECOLOR_METALNESS: unorm8(saturate_hlsl(np.concatenate([base[..., :3], metal[..., None]], -1))), R.IN_DIFF_CONFIDENCE: unorm8(saturate_hlsl(diff)),
                R.IN_SPEC_CONFIDENCE: unorm8(saturate_hlsl(spec)), R.IN_DISOCCLUSION_THRESHOLD_MIX: unorm8(saturate_hlsl(mix))}
        for plane in want.values():
            assert len(np.unique(plane)) == 256
        assert (want[R.IN_DIFF_CONFIDENCE][10, 0:3] == [0, 255, 0]).all()
        for channels in (4, 3):
            kw = dict(base_color=xyz_plane(be, base, channels, w), metalness=up_pad(be, metal), diff_confidence=up_pad(be, diff), spec_confidence=up_pad(be, spec),
                      disocclusion_threshold_mix=up_pad(be, mix))
            got = pack(be, w, h, tuple(want), **kw)
            for slot in want:
                assert_bits(got[slot], want[slot], "%dx%d base colour x%d: %s vs M" % (w, h, channels, slot.name))
        # one slot alone, and all of them next to the position outputs: the same bytes
        got = pack(be, w, h, (R.IN_SPEC_CONFIDENCE,), spec_confidence=up_pad(be, spec))
        assert_bits(got[R.IN_SPEC_CONFIDENCE], want[R.IN_SPEC_CONFIDENCE], "IN_SPEC_CONFIDENCE alone")
        cs, cam, cam_prev = settings(w, h, "2.5d")
        X, Xp = scene(w, h, cam, cam_prev, seed=9)
        got = pack(be, w, h, (R.IN_VIEWZ, R.IN_MV) + tuple(want), xyz_plane(be, X, 3, w), cs, xyz_plane(be, Xp, 4, w), **kw)
        want_z, want_mv = M.pack(cs, X, Xp, MISS)
        assert_bits(got[R.IN_VIEWZ], want_z, "all outputs in one launch: IN_VIEWZ vs M")
        assert_bits(got[R.IN_MV], f16(want_mv), "all outputs in one launch: IN_MV vs M")
        for slot in want:
            assert_bits(got[slot], want[slot], "all outputs in one launch: %s vs M" % slot.name)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. validation
def _np_plane(a, fmt, **kw):
    return TPR._plane(a, fmt, **kw)


class HostCase:
    """a valid descriptor over host arrays (64 x 32, every input and output) that a test mutates; the outputs are stamped and compared after every refused call"""

    W, H = 64, 32

    def __init__(self):
        h, w = self.H, self.W
        self.cs = settings(w, h, "2.5d")[0]
        self.pos, self.prev, self.base = np.ones((h, w, 4), f32), np.ones((h, w, 3), f32), np.ones((h, w, 4), f32)
        self.r32 = np.ones((h, w), f32)
        self.z, self.mv = np.full((h, w), STAMP32, f32), np.full((h, w, 4), STAMP16, np.float16)
        self.bcm, self.c8 = np.full((h, w, 4), STAMP8, np.uint8), np.full((3, h, w), STAMP8, np.uint8)

    def desc(self):
        d = api.HipGuidesDesc()
        d.commonSettings, d.missViewZ = C.cast(C.byref(self.cs), C.c_void_p), float(MISS)
        d.position, d.positionPrev, d.baseColor = _np_plane(self.pos, F.RGBA32_SFLOAT), _np_plane(self.prev, F.RGB32_SFLOAT), _np_plane(self.base, F.RGBA32_SFLOAT)
        d.metalness = d.diffConfidence = d.specConfidence = d.disocclusionThresholdMix = _np_plane(self.r32, F.R32_SFLOAT)
        d.outViewZ, d.outMv, d.outBaseColorMetalness = _np_plane(self.z, F.R32_SFLOAT), _np_plane(self.mv, F.RGBA16_SFLOAT), _np_plane(self.bcm, F.RGBA8_UNORM)
        d.outDiffConfidence, d.outSpecConfidence, d.outDisocclusionThresholdMix = (_np_plane(self.c8[i], F.R8_UNORM) for i in range(3))
        return d

    def untouched(self):
        return (self.z == f32(STAMP32)).all() and (self.mv == np.float16(STAMP16)).all() and (self.bcm == STAMP8).all() and (self.c8 == STAMP8).all()

    def restamp(self):
        self.z[:], self.mv[:], self.bcm[:], self.c8[:] = STAMP32, STAMP16, STAMP8, STAMP8


OUTPUTS = ("outViewZ", "outMv", "outBaseColorMetalness", "outDiffConfidence", "outSpecConfidence", "outDisocclusionThresholdMix")


@pytest.mark.parametrize("which", ["emu", "product"])
def test_validation_rules_name_the_field_and_touch_nothing(which):
    """every rule of the header comment: the stated code, a text that names the field, no output byte touched. On the emulated device code (where an accepted call would write) and
    on the product library with no GPU present (all of it happens in front of the first HIP call)"""
    lib = Backend("emu").lib if which == "emu" else api.load_library()
    case = HostCase()
    inv, uns = RC.INVALID_ARGUMENT, RC.UNSUPPORTED
    absent = api.HipPlaneDesc

    def run(mutate, code, *words, cs=None):
        d = case.desc()
        if cs is not None:
            d.commonSettings = C.cast(C.byref(cs), C.c_void_p)
        mutate(d)
        got, text = RC(lib.nrdHipPackGuides(C.byref(d), None)), lib.nrdHipGetLastFrontEndError().decode()
        assert got == code and all(word in text for word in words) and text.startswith("nrdHipPackGuides"), (got, text, words)
        assert case.untouched(), text

    def field(path, value):
        def f(d):
            obj, names = d, path.split(".")
            for name in names[:-1]:
                obj = getattr(obj, name)
            setattr(obj, names[-1], value)
        return f

    def drop(*names):
        def f(d):
            for name in names:
                setattr(d, name, absent())
        return f

    def only(*names):  # the descriptor reduced to these planes (and the scalars)
        return drop(*[n for n, _ in api.HipGuidesDesc._fields_ if n not in names and n not in ("commonSettings", "missViewZ", "reserved")])

    def both(*fs):
        return lambda d: [f(d) for f in fs]

    assert RC(lib.nrdHipPackGuides(None, None)) == inv
    # no output at all
    run(drop(*OUTPUTS), inv, "no output")
    # an output whose input is missing
    run(drop("position", "positionPrev"), inv, "position")
    run(both(only("position", "outViewZ"), field("commonSettings", None)), inv, "commonSettings")
    run(both(only("position", "outMv"), field("commonSettings", None)), inv, "commonSettings")
    run(drop("baseColor"), inv, "baseColor", "outBaseColorMetalness")
    run(drop("metalness"), inv, "metalness", "outBaseColorMetalness")
    for name in ("diffConfidence", "specConfidence", "disocclusionThresholdMix"):
        run(drop(name), inv, name, "out" + name[0].upper() + name[1:])
    # an input without any output that reads it
    run(drop("outViewZ", "outMv"), inv, "position")
    run(drop("outMv"), inv, "positionPrev", "outMv")
    run(drop("outBaseColorMetalness"), inv, "baseColor")
    run(drop("outBaseColorMetalness", "baseColor"), inv, "metalness")
    for name in ("diffConfidence", "specConfidence", "disocclusionThresholdMix"):
        run(drop("out" + name[0].upper() + name[1:]), inv, name)
    run(field("reserved", 1), inv, "reserved")
    # the settings: rectSize, the sky predicate, the scale, the projection
    w, h = case.W, case.H
    run(lambda d: None, inv, "commonSettings", "rectSize", cs=settings(w, h, "2.5d", rectSize=(w, h - 1))[0])
    for bad in (float("nan"), float("inf"), -float("inf")):
        run(field("missViewZ", bad), inv, "missViewZ")
    run(field("missViewZ", 499999.0), inv, "missViewZ", "denoisingRange")
    run(field("missViewZ", 500000.0), inv, "missViewZ", "denoisingRange")  # not ABOVE the range: the passes denoise such a pixel
    run(field("missViewZ", 1e6), inv, "missViewZ", cs=settings(w, h, "2.5d", viewZScale=0.25)[0])  # 2.5e5 after the scale
    run(field("missViewZ", 1e6), inv, "missViewZ", cs=settings(w, h, "2.5d", denoisingRange=2e6)[0])
    for scale in ((0.0, 1.0 / h, 1.0), (1.0 / w, 0.0, 1.0)):
        run(lambda d: None, inv, "commonSettings", "motionVectorScale", cs=settings(w, h, "2.5d", motionVectorScale=scale)[0])
    ortho = settings(w, h, "2.5d")[0]
    for k, v in ((11, 0.0), (15, 1.0)):
        ortho.viewToClipMatrix[k] = v
    run(lambda d: None, uns, "commonSettings", "orthographic", cs=ortho)
    ortho_prev = settings(w, h, "2.5d")[0]
    for k, v in ((11, 0.0), (15, 1.0)):
        ortho_prev.viewToClipMatrixPrev[k] = v
    run(lambda d: None, uns, "commonSettings", "orthographic", cs=ortho_prev)
    # sizes, pitches, alignment, the 32-bit limits, formats
    run(field("positionPrev.width", w - 1), inv, "positionPrev", "size")
    run(field("outMv.height", h + 1), inv, "outMv", "size")
    run(field("metalness.rowPitchBytes", w * 4 - 4), inv, "metalness", "row pitch")
    run(field("position.rowPitchBytes", w * 16 + 8), inv, "position", "multiple")
    run(field("position.data", case.pos.ctypes.data + 4), inv, "position", "multiple")
    run(field("positionPrev.rowPitchBytes", w * 12 + 2), inv, "positionPrev", "RGB32_SFLOAT", "multiple of 4")
    run(field("positionPrev.data", case.prev.ctypes.data + 2), inv, "positionPrev", "multiple of 4")
    run(field("outMv.data", case.mv.ctypes.data + 4), inv, "outMv", "multiple")
    run(field("position.rowPitchBytes", 1 << 24), uns, "position", "16 MiB")
    for name, fmt in (("position", F.RG32_SFLOAT), ("positionPrev", F.RGBA16_SFLOAT), ("baseColor", F.RGBA8_UNORM), ("metalness", F.R16_SFLOAT), ("diffConfidence", F.R8_UNORM),
                      ("outViewZ", F.R16_SFLOAT), ("outMv", F.RGBA32_SFLOAT), ("outBaseColorMetalness", F.RGBA8_SNORM), ("outDiffConfidence", F.R16_UNORM),
                      ("outDisocclusionThresholdMix", F.R32_SFLOAT)):
        run(field(name + ".format", int(fmt)), uns, name, "format")
    if which == "emu":  # (an accepted descriptor launches: over host arrays that is for the emulated device code alone)
        # what the rules leave alone: world-space mode with a zero scale, missViewZ without outViewZ, the previous projection without outMv, -missViewZ (either sign is sky)
        accepted = [(lambda d: None, settings(w, h, "world0")[0]), (both(drop("outViewZ"), field("missViewZ", 0.0)), None), (drop("outMv", "positionPrev"), ortho_prev),
                    (field("missViewZ", -1e6), None), (only("diffConfidence", "outDiffConfidence"), None)]
        for mutate, cs in accepted:
            d = case.desc()
            if cs is not None:
                d.commonSettings = C.cast(C.byref(cs), C.c_void_p)
            mutate(d)
            assert RC(lib.nrdHipPackGuides(C.byref(d), None)) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()
            assert lib.nrdHipGetLastFrontEndError() == b""
            case.restamp()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. surface
def test_symbols_structs_and_header():
    """The descriptor holds 13 planes of 24 bytes behind 16 bytes of scalars: 328 bytes (the "224" of the issue text counts 16-byte planes, which NrdHipPlaneDesc is not)"""
    lib = api.load_library()
    assert "nrdHipPackGuides" in api.NRD_HIP_SYMBOLS and lib.nrdHipPackGuides
    hdr = open(os.path.join(ROOT, "include", "NRDHip.h")).read()
    assert "uint32_t nrdHipPackGuides(const NrdHipGuidesDesc* desc, void* hipStream);" in hdr
    assert "static_assert(sizeof(NrdHipGuidesDesc) == 328" in hdr
    assert C.sizeof(api.HipGuidesDesc) == 328 == 16 + 13 * C.sizeof(api.HipPlaneDesc)
    assert [n for n, _ in api.HipGuidesDesc._fields_] == ["commonSettings", "missViewZ", "reserved", "position", "positionPrev", "baseColor", "metalness", "diffConfidence",
                                                          "specConfidence", "disocclusionThresholdMix", "outViewZ", "outMv", "outBaseColorMetalness", "outDiffConfidence",
                                                          "outSpecConfidence", "outDisocclusionThresholdMix"]
    hpp = open(os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")).read()
    assert "PackGuides(const NrdHipGuidesDesc& desc)" in hpp
    # the Python surface: in place, numpy or torch, a dict bind_packed takes plus `viewz`
    pos = np.zeros((9, 16, 3), f32)[:8, :12]
    cs = settings(12, 8, "2.5d")[0]
    res, desc, keep = frontend.describe_pack_guides(pos, cs, np.zeros((8, 12, 4), f32), diff_confidence=np.zeros((8, 12), f32))
    assert (desc.position.format, desc.position.rowPitchBytes, desc.positionPrev.format, desc.position.data) == (int(F.RGB32_SFLOAT), 16 * 12, int(F.RGBA32_SFLOAT), pos.ctypes.data)
    assert set(res) == {R.IN_VIEWZ, R.IN_MV, R.IN_DIFF_CONFIDENCE} and res.viewz is res[R.IN_VIEWZ][0] and all(isinstance(k, R) for k in res)
    assert res[R.IN_MV][1] == F.RGBA16_SFLOAT and res[R.IN_MV][0].shape == (8, 12, 4) and res[R.IN_DIFF_CONFIDENCE][0].dtype == np.uint8
    assert desc.missViewZ == frontend.MISS_VIEWZ and not desc.baseColor.data and not desc.outBaseColorMetalness.data
    res, desc, keep = frontend.describe_pack_guides(pos, cs, want=("mv",))
    assert set(res) == {R.IN_MV} and res.viewz is None and desc.outMv.data and not desc.outViewZ.data
    res, desc, keep = frontend.describe_pack_guides(pos, cs, want=("viewz",))
    assert set(res) == {R.IN_VIEWZ} and res.viewz is res[R.IN_VIEWZ][0] and desc.outViewZ.data and not desc.outMv.data
    assert synth.render_frame(16, 8, 0, want=("raw",))["raw"]["position"].shape == (8, 16, 3)


@pytest.mark.parametrize("backend", BACKENDS)
def test_python_surface_packs_and_reuses_its_outputs(backend):
    """frontend.pack_guides on dense arrays, no `out`; then with out= its own result: the same arrays, written again"""
    be = Backend(backend)
    w, h = W0, H0
    cs, cam, cam_prev = settings(w, h, "2.5d")
    X, Xp = scene(w, h, cam, cam_prev, seed=21)
    want_z, want_mv = M.pack(cs, X, Xp, frontend.MISS_VIEWZ)
    conf = np.random.RandomState(22).uniform(0, 1, (h, w)).astype(f32)
    res = frontend.pack_guides(be.up(X[..., :3]), cs, be.up(Xp), diff_confidence=be.up(conf), lib=be.lib)
    assert_bits(be.down(res[R.IN_VIEWZ][0]), want_z, "frontend.pack_guides: IN_VIEWZ vs M")
    assert_bits(be.down(res[R.IN_MV][0]), f16(want_mv), "frontend.pack_guides: IN_MV vs M")
    assert_bits(be.down(res[R.IN_DIFF_CONFIDENCE][0]), unorm8(conf), "frontend.pack_guides: IN_DIFF_CONFIDENCE vs M")
    again = frontend.pack_guides(be.up(X[..., :3]), cs, None, diff_confidence=be.up(conf), out=res, lib=be.lib)
    assert again[R.IN_MV][0] is res[R.IN_MV][0] and again.viewz is res.viewz
    assert_bits(be.down(again[R.IN_MV][0]), f16(M.pack(cs, X, None, frontend.MISS_VIEWZ)[1]), "frontend.pack_guides(out=...): IN_MV vs M")


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "guides_integration.cpp")
CPP_EXE = os.path.join(ROOT, "tests", "cpp", "build", "guides_integration")


def _build_cpp():
    """as tests/test_shadow_lights.py builds its program: g++, the installed headers, libNRD_hip.so"""
    lib = native_build.build_product()
    os.makedirs(os.path.dirname(CPP_EXE), exist_ok=True)
    hpp = os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")
    if os.path.exists(CPP_EXE) and os.path.getmtime(CPP_EXE) > max(os.path.getmtime(CPP_SRC), os.path.getmtime(lib), os.path.getmtime(hpp)):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-attributes", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", CPP_SRC, "-o", CPP_EXE,
           "-L" + os.path.dirname(lib), "-lNRD_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../../../raytracingdenoiser_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_cpp_integration_compiles_and_validates_on_the_host():
    _build_cpp()
    r = subprocess.run([CPP_EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host-only OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_integration_packs_guides():
    _build_cpp()
    r = subprocess.run([CPP_EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "guides integration OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7. / 8. the denoisers (GPU)
@functools.lru_cache(maxsize=None)
def rendered(f):
    return synth.render_frame(SYNTH_W, SYNTH_H, f, want=("reblur", "raw", "mv2d"))


def denoise_sequence(name, frames, guides, validation=False, handed="lh"):
    """`frames` frames of the moving camera at 192 x 128 through one instance; guides: "synth" (synth's own mv2d), "packed" (IN_VIEWZ / IN_MV from frontend.pack_guides, both
    with s = (1 / w, 1 / h, 1)) or "world" (world-space mode, zero vectors). handed="rh": the application works right-handed -- the matrices of right_handed() for the packer
    and for the denoiser, IN_VIEWZ negative. Returns per frame {ResourceType: output as numpy}, the sky masks, and what check_inputs() said."""
    from raytracingdenoiser_amd.executor import HipExecutor

    w, h = SYNTH_W, SYNTH_H
    inst = api.Instance([(0, parity.DENOISERS[name][0])])
    ex = HipExecutor(inst, w, h)
    outs = {}
    for rt, dtype, ch, fmt in parity.output_planes(name, w, h, validation):
        outs[rt] = torch.zeros((h, w, ch), dtype=dtype, device="cuda")
        ex.bind(rt, outs[rt], fmt)
    results, skies, checks = [], [], []
    for f in range(frames):
        frame = rendered(f)
        if guides != "synth":
            frame = dict(frame, mv=torch.zeros_like(frame["mv"]))
        cam_prev = synth.Camera(w, h, max(f - 1, 0))
        kw = dict(enableValidation=validation)
        if guides != "world":
            kw.update(isMotionVectorInWorldSpace=False, motionVectorScale=(1.0 / w, 1.0 / h, 1.0))
        cam = frame["camera"]
        if handed == "rh":
            assert guides == "packed"
            cam, cam_prev = right_handed(cam), right_handed(cam_prev)
        cs = parity.common_settings(cam, cam_prev, w, h, f, **kw)
        planes = {rt: (t.cuda().clone().contiguous(), fmt) for rt, t, fmt in parity.user_planes(name, frame)}
        if guides == "packed":
            position = frame["raw"]["position"].cuda().contiguous()
            assert bool(torch.isnan(position[frame["is_sky"]]).all())
            planes.update(frontend.pack_guides(position, cs, miss_viewz=synth.SKY_VIEWZ))
        ex.bind_packed(planes)
        assert inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame)) == api.Result.SUCCESS
        assert inst.set_common_settings(cs) == api.Result.SUCCESS
        checks.append(ex.check_inputs())
        ex.denoise()
        torch.cuda.synchronize()
        results.append({rt: t.cpu().numpy().copy() for rt, t in outs.items()})
        skies.append(frame["is_sky"].numpy())
    ex.destroy()
    return results, skies, checks


@pytest.mark.gpu
def test_the_validation_overlay_judges_the_packed_vectors():
    """REBLUR_DIFFUSE with enableValidation, 192 x 128, 3 frames, the moving camera. Viewport 3 of OUT_VALIDATION (kernels_validation.hip) shows, per texel, |uv + mv - the
    projection of the reconstructed position into the previous frame| in pixels as red / green, and blue where the previous position is off screen. With IN_VIEWZ / IN_MV from
    pack_guides: red and green <= 1 / 255 (motion is under 4 pixels: the fp16 half-ulp is 2^-9 pixels, below 1.5 / 255), blue as in the world-space run with zero vectors,
    whose red and green are 0 by construction; check_inputs() reports nothing although the position plane holds NaN on the sky.
    Those bounds are judged on the viewport texels whose source texel and its eight neighbours are geometry: on the sky the call stores a zero vector by the rule of the header (as
    synth does), and there the overlay shows the camera's rotation (about 0.2 pixels per frame here), whatever packed the vectors. The rest of the viewport is held against run
    (a), synth's own mv2d: where the whole neighbourhood is sky both runs bind the same depth and the same zero vector, so the bytes are equal; on the silhouette ring a texel
    shows either that or geometry, where both runs are within 1: at most 1 apart.
    The same sequence once more the way a right-handed application runs it (right-handed matrices for the packer and the denoiser, IN_VIEWZ negative): the denoiser flips such
    matrices to its left-handed convention and takes abs( IN_VIEWZ ), so viewport 3 and the denoised output must be the left-handed run's, byte for byte -- which they are only if
    the packed vectors, .z included, are in the passes' convention for either handedness."""
    w, h = SYNTH_W, SYNTH_H
    vw, vh = w // 4, h // 4
    packed, skies, checks = denoise_sequence("REBLUR_DIFFUSE", 3, "packed", validation=True)
    world, _, _ = denoise_sequence("REBLUR_DIFFUSE", 3, "world", validation=True)
    own, _, _ = denoise_sequence("REBLUR_DIFFUSE", 3, "synth", validation=True)
    right, _, right_checks = denoise_sequence("REBLUR_DIFFUSE", 3, "packed", validation=True, handed="rh")
    for check in right_checks:
        assert check, check.rules
    for f in range(3):
        assert_bits(right[f][R.OUT_DIFF_RADIANCE_HITDIST], packed[f][R.OUT_DIFF_RADIANCE_HITDIST], "frame %d: right-handed run == left-handed run: OUT_DIFF_RADIANCE_HITDIST" % f)
        assert_bits(right[f][R.OUT_VALIDATION][:vh, 3 * vw:4 * vw], packed[f][R.OUT_VALIDATION][:vh, 3 * vw:4 * vw], "frame %d: right-handed run == left-handed run: viewport 3" % f)
    assert len(np.unique(packed[2][R.OUT_DIFF_RADIANCE_HITDIST])) > 100
    for check in checks:
        assert check, check.rules
    for f in (1, 2):  # (the frame that resets the history clears the overlay)
        b = packed[f][R.OUT_VALIDATION][:vh, 3 * vw:4 * vw]
        c = world[f][R.OUT_VALIDATION][:vh, 3 * vw:4 * vw]
        sky = torch.from_numpy(skies[f]).float()[None, None]
        near_sky = torch.nn.functional.max_pool2d(sky, 3, 1, 1)[0, 0].numpy() > 0
        geometry = ~near_sky[2::4, 2::4][:vh, :vw]
        assert geometry.mean() > 0.3 and b[..., 3].min() == 255
        print("frame %d: viewport 3 red / green max on geometry %d / %d (world-space run: %d / %d), blue texels %d" % (
            f, b[..., 0][geometry].max(), b[..., 1][geometry].max(), c[..., 0][geometry].max(), c[..., 1][geometry].max(), int((b[..., 2] != 0).sum())))
        assert (c[..., :2][geometry] == 0).all()
        assert b[..., 0][geometry].max() <= 1 and b[..., 1][geometry].max() <= 1
        assert (b[..., 2][geometry] == c[..., 2][geometry]).all()
        a = own[f][R.OUT_VALIDATION][:vh, 3 * vw:4 * vw]
        all_sky = (torch.nn.functional.max_pool2d(1.0 - sky, 3, 1, 1)[0, 0].numpy() == 0)[2::4, 2::4][:vh, :vw]
        assert all_sky.any() and (b[all_sky] == a[all_sky]).all()
        print("frame %d: off geometry: %d sky texels equal to run (a), worst byte distance to run (a) elsewhere %d" % (
            f, int(all_sky.sum()), int(np.abs(b.astype(np.int32) - a.astype(np.int32))[~geometry].max())))
        assert np.abs(b.astype(np.int32) - a.astype(np.int32))[~geometry].max() <= 1


def differing_share(xs, ys):
    """share of output texels where x differs from y by more than 1e-3 relative"""
    count = total = 0
    for x, y in zip(xs, ys):
        for rt in x:
            a, b = x[rt].astype(np.float64), y[rt].astype(np.float64)
            count += int((np.abs(a - b) > 1e-3 * np.abs(b)).sum())
            total += a.size
    return count / total


@pytest.mark.gpu
def test_end_to_end_packed_guides_denoise_like_synths_own():
    """REBLUR_DIFFUSE_SPECULAR, 192 x 128, 4 frames, the moving camera: (a) synth's own mv2d, (b) IN_VIEWZ / IN_MV from pack_guides, (c) world-space zero vectors. The share of
    output texels where (b) differs from (a) by more than 1e-3 relative is no larger than the share for the pair (a, c) -- the spread two correct conventions already have at the
    parent commit. Measured on an MI355X: 0.00035 for (a, b), 0.00100 for (a, c)."""
    a, _, _ = denoise_sequence("REBLUR_DIFFUSE_SPECULAR", 4, "synth")
    b, _, checks = denoise_sequence("REBLUR_DIFFUSE_SPECULAR", 4, "packed")
    c, _, _ = denoise_sequence("REBLUR_DIFFUSE_SPECULAR", 4, "world")
    for check in checks:
        assert check, check.rules
    share_ab, share_ac = differing_share(b, a), differing_share(c, a)
    print("share of output texels more than 1e-3 apart: packed guides vs synth's mv2d %.5f, world-space zero vectors vs synth's mv2d %.5f" % (share_ab, share_ac))
    assert share_ab <= share_ac


# ---------------------------------------------------------------------------------------------------------------------------------------------- 9. graph capture
@pytest.mark.gpu
def test_captured_call_replays_the_same_bytes():
    """the contract of the other front-end calls: no allocation, no synchronisation -- the call is capturable by torch.cuda.graph and replays the same bytes"""
    w, h = W0, H0
    cs, cam, cam_prev = settings(w, h, "2.5d")
    X, Xp = scene(w, h, cam, cam_prev, seed=50)
    rng = np.random.RandomState(51)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(position_prev=dev(Xp), base_color=dev(rng.uniform(0, 1, (h, w, 3)).astype(f32)), metalness=dev(rng.uniform(0, 1, (h, w)).astype(f32)),
              disocclusion_threshold_mix=dev(rng.uniform(0, 1, (h, w)).astype(f32)))
    position = dev(X[..., :3])
    packed = frontend.pack_guides(position, cs, **kw)
    torch.cuda.synchronize()
    eager = {k: t.cpu().numpy().copy() for k, (t, fmt) in packed.items()}
    assert_bits(eager[R.IN_MV], f16(M.pack(cs, X, Xp, frontend.MISS_VIEWZ)[1]), "eager IN_MV vs M")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frontend.pack_guides(position, cs, out=packed, **kw)
    for t, fmt in packed.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, (t, fmt) in packed.items():
        assert_bits(t.cpu().numpy(), eager[k], "captured nrdHipPackGuides == eager: %s" % k.name)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 10. static facts
def test_static_facts_of_the_guides_kernels():
    """what the compiler made of every instantiation for gfx950 (tools/frontend_bench.py guides_isa(), the `isa_guides` object of profiles/frontend_bench.json): no scratch, no
    LDS. VGPRs and waves per SIMD are printed and recorded, not bounded."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import frontend_bench

    facts = frontend_bench.guides_isa()
    assert len(facts) == 7
    for name, k in facts.items():
        print(name, k)
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0, (name, k)
        assert k["vgprs"] > 0 and k["waves_per_simd"] >= 1
    # 16-byte loads for RGBA32_SFLOAT planes, 12-byte ones for RGB32_SFLOAT: two positions, and the base colour in either form behind a scalar branch on its format
    for name, (x4, x3) in {"pack_guides_0_0": (1, 1), "pack_guides_16_16": (3, 1), "pack_guides_12_12": (1, 3), "pack_guides_16_12": (2, 2), "pack_guides_12_0": (1, 2)}.items():
        assert (facts[name]["global_load_dwordx4"], facts[name]["global_load_dwordx3"]) == (x4, x3), (name, facts[name])
