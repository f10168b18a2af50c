"""nrdHipPackShadowLights / nrdHipResolveShadowLights (include/NRDHip.h, raytracingdenoiser_amd/frontend.py): SIGMA's front end and back end for local lights and for many
lights per pixel -- per light, or combined into one SIGMA_SHADOW_TRANSLUCENCY pass by the README's recipe.

As in tests/test_pack_samples.py every comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU). Expected values never
come from the code under test:
  P  the parent commit's nrdHipPackInputs on the same planes (one directional light)
  M  tests/shadow_lights_model.py, a float32 numpy restatement of the formulas of the header. They use only + - * / min max and selects, every intermediate is np.float32,
     so every comparison is bit for bit on both backends: there is no tolerance anywhere in this file.
Inputs live in wider allocations (rows longer than the plane, rows between the layers) whose surroundings are NaN; outputs in stamped ones that are compared whole."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import shadow_lights_model as M
import test_pack_resolve as TPR
from raytracingdenoiser_amd import api, build as native_build, frontend
from test_pack_resolve import BACKENDS, Backend, assert_bits, f16, unorm8

ROOT = TPR.ROOT
F, R, RC, LT, SM = api.Format, api.ResourceType, api.Result, api.LightType, api.ShadowsMode
f32 = np.float32
W1, H1 = 197, 61  # a 5-pixel last workgroup column, a 1-row last row of workgroups
W0, H0 = 67, 23
PAD, GAP = 5, 3
STAMP16, STAMP8, STAMP32 = 23130, 0x5A, 7.5
MISS = f32(1e5)


# ---------------------------------------------------------------------------------------------------------------------------------------------- inputs
def lights_of(n):
    """n lights of mixed types whose parameters reach the 32768 clamp: (type, tan of the angular radius | light size)"""
    table = [(LT.LOCAL, 0.5), (LT.DIRECTIONAL, 0.02), (LT.LOCAL, 3e6), (LT.DIRECTIONAL, 5e3), (LT.LOCAL, 0.0), (LT.DIRECTIONAL, 0.0), (LT.LOCAL, 12.0)]
    return [table[i % len(table)] for i in range(n)]


def scene(n, w, h, seed=0):
    """d, dl [n, h, w], lighting / translucency [n, h, w, 4], weight [n, h, w]: random values with the special cases of the issue planted in known rows"""
    rng = np.random.RandomState(seed)
    d = rng.uniform(0.01, 60.0, (n, h, w)).astype(f32)
    kind = rng.randint(0, 8, (n, h, w))
    d[kind == 0] = 0.0          # NoL <= 0
    d[kind == 1] = 65504.0      # a miss, exactly the threshold
    d[kind == 2] = MISS         # a miss
    dl = (d + rng.uniform(0.001, 30.0, (n, h, w))).astype(f32)
    at = rng.randint(0, 10, (n, h, w))
    dl[at == 0] = d[at == 0]                                # d = distanceToLight: the max( ..., NRD_EPS ) branch
    dl[at == 1] = (d[at == 1] * f32(0.5)).astype(f32)       # d > distanceToLight
    lighting = rng.uniform(0.0, 4.0, (n, h, w, 4)).astype(f32)
    lighting[..., 3] = np.nan                               # .w is never consumed
    d[:, 0, :] = MISS                                       # row 0: every light lit
    d[:, 1, :] = rng.uniform(0.01, 60.0, (n, w))            # row 1: every light occluded
    lighting[:, 2, :, :3] = 0.0                             # row 2: Lsum = 0
    if n > 1:
        lighting[1, ..., :3] = 0.0                          # a light with L = 0
    translucency = rng.uniform(-0.25, 1.25, (n, h, w, 4)).astype(f32)
    translucency[..., 3] = np.nan
    weight = rng.uniform(0.0, 2.0, (n, h, w)).astype(f32)
    weight[d >= 65504.0] = 0.0                              # the README's rule for a caller's weights
    return dict(d=d, dl=dl, lighting=lighting, translucency=translucency, weight=weight)


def up_stack(be, a, fill=np.nan, pad=PAD, gap=GAP):
    """[N, H, W(, C)] on the backend inside a wider allocation: rows `pad` texels longer, `gap` rows between the layers, everything around the rects = `fill`"""
    n, h, w = a.shape[:3]
    big = np.full((n, h + gap, w + pad) + a.shape[3:], fill, dtype=a.dtype)
    big[:, :h, :w] = a
    big = big if be.name == "emu" else torch.from_numpy(big).cuda()
    return big[:, :h, :w]


def out_stack(be, shape, dtype, stamp, stacked, pad=PAD, gap=GAP):
    """(view, whole allocation) of a stamped output: a stack [N, H, W(, C)] with `gap` rows between the layers, or one plane [H, W(, C)]; rows `pad` texels longer"""
    if not stacked:
        return be.padded(shape, dtype, pad, stamp)
    n, h, w = shape[:3]
    big = np.full((n, h + gap, w + pad) + tuple(shape[3:]), stamp, dtype=dtype)
    big = big if be.name == "emu" else torch.from_numpy(big).cuda()
    return big[:, :h, :w], big


def assert_whole(be, big, got, stamp, stacked, what):
    """no byte outside the output rects changed"""
    whole = be.down(big)
    want = np.full(whole.shape, stamp, dtype=whole.dtype)
    if stacked:
        want[:, :got.shape[1], :got.shape[2]] = got
    else:
        want[:got.shape[0], :got.shape[1]] = got
    assert np.array_equal(np.ascontiguousarray(whole).view(np.uint8), want.view(np.uint8)), "bytes outside the rect were written: " + what


def pack(be, lights, ins, mode, translucency=False, weight=False, sum_channels=4, colour_channels=4, need_dl=True):
    """one nrdHipPackShadowLights launch through the C-ABI on padded, gapped stacks; returns {slot: downloaded plane}. Every output allocation is held against its stamp."""
    n, h, w = ins["d"].shape
    colour = lambda a: np.ascontiguousarray(a[..., :colour_channels])
    kw = dict(mode=mode, lib=be.lib)
    if need_dl:
        kw["distance_to_light"] = up_stack(be, ins["dl"])
    if mode == SM.COMBINED:
        kw["lighting"] = up_stack(be, colour(ins["lighting"]))
        if weight:
            kw["weight"] = up_stack(be, ins["weight"])
    elif translucency:
        kw["translucency"] = up_stack(be, colour(ins["translucency"]))
    d = up_stack(be, ins["d"])
    stack = () if mode == SM.COMBINED else (n,)
    out, bigs = {}, {}
    view, bigs[R.IN_PENUMBRA] = out_stack(be, stack + (h, w), "float16", STAMP16, bool(stack))
    out[R.IN_PENUMBRA] = (view, F.R16_SFLOAT)
    if mode == SM.COMBINED or translucency:
        view, bigs[R.IN_TRANSLUCENCY] = out_stack(be, stack + (h, w, 4), "uint8", STAMP8, bool(stack))
        out[R.IN_TRANSLUCENCY] = (view, F.RGBA8_UNORM)
    if mode == SM.COMBINED:
        view, bigs["lighting_sum"] = be.padded((h, w, sum_channels), "float32", PAD, STAMP32)
        out["lighting_sum"] = (view, F.RGB32_SFLOAT if sum_channels == 3 else F.RGBA32_SFLOAT)
    res, desc, keep = frontend.describe_pack_shadow_lights(lights, d, out=out, **kw)
    assert set(res) == set(out)
    code = be.lib.nrdHipPackShadowLights(C.byref(desc), None)
    assert RC(code) == RC.SUCCESS, be.lib.nrdHipGetLastFrontEndError()
    got = {slot: be.down(t).copy() for slot, (t, fmt) in res.items()}
    for slot, big in bigs.items():
        stamp = {R.IN_PENUMBRA: STAMP16, R.IN_TRANSLUCENCY: STAMP8, "lighting_sum": STAMP32}[slot]
        assert_whole(be, big, got[slot], np.array(stamp).astype(got[slot].dtype), bool(stack) and slot != "lighting_sum", str(slot))
    return got


def model_per_light(lights, ins):
    p = np.stack([M.penumbra(l, ins["d"][i], ins["dl"][i]) for i, l in enumerate(lights)])
    t = np.stack([M.pack_translucency(ins["d"][i], ins["translucency"][i]) for i in range(len(lights))])
    return f16(p), unorm8(t)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1. one directional light
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_directional_light_writes_the_bytes_of_the_plain_pack_call(backend):
    """N = 1, DIRECTIONAL, PER_LIGHT == the parent's nrdHipPackInputs on the same planes: IN_PENUMBRA and IN_TRANSLUCENCY, bit for bit"""
    be = Backend(backend)
    w, h, tan = W1, H1, 0.02
    ins = scene(1, w, h, seed=1)
    nr = np.zeros((h, w, 4), f32)
    nr[..., 2] = 1.0
    d, t = be.up_pitched(ins["d"][0], PAD), be.up_pitched(ins["translucency"][0], PAD)
    old = frontend.pack_inputs(be.up(nr), be.up(np.ones((h, w), f32)), distance_to_occluder=d, translucency=t, tan_of_light_angular_radius=tan, lib=be.lib)
    new = pack(be, [(LT.DIRECTIONAL, tan)], ins, SM.PER_LIGHT, translucency=True, need_dl=False)
    assert_bits(new[R.IN_PENUMBRA][0], be.down(old[R.IN_PENUMBRA][0]), "one directional light: IN_PENUMBRA == nrdHipPackInputs")
    assert_bits(new[R.IN_TRANSLUCENCY][0], be.down(old[R.IN_TRANSLUCENCY][0]), "one directional light: IN_TRANSLUCENCY == nrdHipPackInputs")
    # the same through the Python surface, one [H, W] plane instead of a stack
    res = frontend.pack_shadow_lights([dict(type=LT.DIRECTIONAL, tan_of_light_angular_radius=tan)], d, translucency=t, lib=be.lib)
    assert res[R.IN_PENUMBRA][1] == F.R16_SFLOAT and tuple(res[R.IN_PENUMBRA][0].shape) == (1, h, w) and tuple(res[R.IN_TRANSLUCENCY][0].shape) == (1, h, w, 4)
    assert_bits(be.down(res[R.IN_PENUMBRA][0])[0], be.down(old[R.IN_PENUMBRA][0]), "frontend.pack_shadow_lights: IN_PENUMBRA == nrdHipPackInputs")
    assert_bits(be.down(res[R.IN_TRANSLUCENCY][0])[0], be.down(old[R.IN_TRANSLUCENCY][0]), "frontend.pack_shadow_lights: IN_TRANSLUCENCY == nrdHipPackInputs")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2. local lights
@pytest.mark.parametrize("backend", BACKENDS)
def test_local_lights_against_the_model(backend):
    """LOCAL lights, N = 4 (one full batch): d = 0, d >= 65504, d = distanceToLight, d > distanceToLight and sizes that reach the 32768 clamp, all present in the inputs"""
    be = Backend(backend)
    lights = [(LT.LOCAL, 0.5), (LT.LOCAL, 3e6), (LT.LOCAL, 0.0), (LT.LOCAL, 12.0)]
    ins = scene(4, W1, H1, seed=2)
    d, dl = ins["d"], ins["dl"]
    assert (d == 0).sum() > 100 and (d == 65504).sum() > 100 and (d > 65504).sum() > 100 and (dl == d).sum() > 100 and ((dl < d) & (d < 65504)).sum() > 100
    want_p, want_t = model_per_light(lights, ins)
    assert (want_p[1] == 32768).sum() > 100 and (want_p == 65504).sum() > 100 and (want_p[2][d[2] < 65504] == 0).all()
    got = pack(be, lights, ins, SM.PER_LIGHT, translucency=True)
    assert_bits(got[R.IN_PENUMBRA], want_p, "four local lights: IN_PENUMBRA vs M")
    assert_bits(got[R.IN_TRANSLUCENCY], want_t, "four local lights: IN_TRANSLUCENCY vs M")
    assert np.isfinite(got[R.IN_PENUMBRA].astype(f32)).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. mixed types
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("colour_channels", [4, 3])
def test_per_light_mixed_types_read_only_what_they_need(backend, colour_channels):
    """PER_LIGHT, N = 3 (less than a batch), local / directional / local: the gaps between the layers, the row padding and the WHOLE distanceToLight layer of the directional
    light hold NaN, and no output is NaN -- they are not read; translucency as RGBA32_SFLOAT and as RGB32_SFLOAT; no byte outside the output rects changes (pack())"""
    be = Backend(backend)
    lights = lights_of(3)
    assert [l[0] for l in lights] == [LT.LOCAL, LT.DIRECTIONAL, LT.LOCAL]
    ins = scene(3, W1, H1, seed=3)
    want_p, want_t = model_per_light(lights, ins)
    poisoned = dict(ins, dl=ins["dl"].copy())
    poisoned["dl"][1] = np.nan
    got = pack(be, lights, poisoned, SM.PER_LIGHT, translucency=True, colour_channels=colour_channels)
    assert_bits(got[R.IN_PENUMBRA], want_p, "three mixed lights: IN_PENUMBRA vs M")
    assert_bits(got[R.IN_TRANSLUCENCY], want_t, "three mixed lights (%d-channel translucency): IN_TRANSLUCENCY vs M" % colour_channels)
    assert np.isfinite(got[R.IN_PENUMBRA].astype(f32)).all()
    alone = pack(be, lights, poisoned, SM.PER_LIGHT)  # without translucency: the penumbra stack alone
    assert set(alone) == {R.IN_PENUMBRA}
    assert_bits(alone[R.IN_PENUMBRA], want_p, "three mixed lights, no translucency: IN_PENUMBRA vs M")


@pytest.mark.parametrize("backend", BACKENDS)
def test_per_light_thirty_two_lights(backend):
    """the largest count at 67 x 23: eight full batches"""
    be = Backend(backend)
    lights = lights_of(32)
    ins = scene(32, W0, H0, seed=4)
    want_p, want_t = model_per_light(lights, ins)
    got = pack(be, lights, ins, SM.PER_LIGHT, translucency=True)
    assert_bits(got[R.IN_PENUMBRA], want_p, "32 lights: IN_PENUMBRA vs M")
    assert_bits(got[R.IN_TRANSLUCENCY], want_t, "32 lights: IN_TRANSLUCENCY vs M")


@pytest.mark.parametrize("backend", BACKENDS)
def test_python_surface_on_an_odd_frame_with_dense_stacks(backend):
    """frontend.pack_shadow_lights / resolve_shadow_lights with N = 3 at 67 x 23, no `out`: H x W is odd, so a dense float16 [N, H, W] stack (stride 3082) and a dense uint8 one
    (1541) break the layer-stride rule of the header. The helper allocates its outputs with padded layers, shadow_stack does the same, and a dense uint8 shadow stack handed to
    the resolve is restacked -- all three against the model"""
    be = Backend(backend)
    n, w, h = 3, W0, H0
    assert (w * h * 2) % 4 and (w * h) % 4
    lights = lights_of(n)
    ins = scene(n, w, h, seed=7)
    want_p, want_t = model_per_light(lights, ins)
    res = frontend.pack_shadow_lights(lights, be.up(ins["d"]), be.up(ins["dl"]), be.up(ins["translucency"]), lib=be.lib)
    pen, tr = res[R.IN_PENUMBRA][0], res[R.IN_TRANSLUCENCY][0]
    assert tuple(pen.shape) == (n, h, w) and frontend._stride0_bytes(pen) % 4 == 0 and frontend._rows_dense(be.up(ins["d"])[0], 0)
    assert_bits(be.down(pen), want_p, "frontend.pack_shadow_lights 67 x 23, N = 3: IN_PENUMBRA vs M")
    assert_bits(be.down(tr), want_t, "frontend.pack_shadow_lights 67 x 23, N = 3: IN_TRANSLUCENCY vs M")
    again = frontend.pack_shadow_lights(lights, be.up(ins["d"]), be.up(ins["dl"]), be.up(ins["translucency"]), out=res, lib=be.lib)  # its own outputs, written again
    assert again[R.IN_PENUMBRA][0] is pen
    assert_bits(be.down(pen), want_p, "frontend.pack_shadow_lights(out=...): IN_PENUMBRA vs M")
    rng = np.random.RandomState(8)
    shadows = rng.randint(0, 256, (n, h, w)).astype(np.uint8)
    lighting = np.ascontiguousarray(ins["lighting"][..., :3])
    want = M.resolve_per_light(shadows, lighting)
    dense = be.up(shadows)
    assert frontend._stride0_bytes(dense) == w * h
    assert_bits(be.down(frontend.resolve_shadow_lights(dense, be.up(lighting), lib=be.lib)), want, "frontend.resolve_shadow_lights, dense uint8 [3, 23, 67] vs M")
    stack = frontend.shadow_stack(dense, n, h, w)
    assert frontend._stride0_bytes(stack) == w * h + 3 and tuple(stack.shape) == (n, h, w)
    stack[...] = dense
    t, desc, keep = frontend.describe_resolve_shadow_lights(stack, be.up(lighting), lib=be.lib)
    assert not keep and desc.shadowLayerBytes == w * h + 3  # read where it lies
    assert_bits(be.down(frontend.resolve_shadow_lights(stack, be.up(lighting), lib=be.lib)), want, "frontend.resolve_shadow_lights, shadow_stack vs M")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. combined
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [2, 5, 32])
def test_combined_against_the_model(backend, n, weighted):
    """COMBINED with and without a weight plane: rows of all-lit and of all-occluded pixels, a row with Lsum = 0, a light with L = 0; outLightingSum as RGBA32_SFLOAT and as
    RGB32_SFLOAT (with the lighting read as RGB32_SFLOAT)"""
    be = Backend(backend)
    w, h = (W0, H0) if n == 32 else (W1, H1)
    lights = lights_of(n)
    ins = scene(n, w, h, seed=10 + n)
    poisoned = dict(ins, dl=ins["dl"].copy())
    for i, l in enumerate(lights):
        if l[0] == LT.DIRECTIONAL:
            poisoned["dl"][i] = np.nan
    p, t, lsum = M.combined(lights, ins["d"], ins["dl"], ins["lighting"], ins["weight"] if weighted else None)
    assert (t[0, :, 0] == 1).all() and (t[1, :, 0] == 0).all() and (p[0] == 65504).all() and (lsum[2] == 0).all() and (t[2, :, 1:] == 0).all()
    assert np.isfinite(p).all() and np.isfinite(t).all()
    for channels in (4, 3):
        got = pack(be, lights, poisoned, SM.COMBINED, weight=weighted, sum_channels=channels, colour_channels=channels)
        what = "COMBINED N = %d%s, %d channels: " % (n, ", weighted" if weighted else "", channels)
        assert_bits(got[R.IN_PENUMBRA], f16(p), what + "IN_PENUMBRA vs M")
        assert_bits(got[R.IN_TRANSLUCENCY], unorm8(t), what + "IN_TRANSLUCENCY vs M")
        want_sum = lsum if channels == 3 else np.concatenate([lsum, np.zeros((h, w, 1), f32)], -1)
        assert_bits(got["lighting_sum"], want_sum, what + "outLightingSum vs M")
    # .x of IN_TRANSLUCENCY is 1 exactly where no light is occluded
    assert np.array_equal(got[R.IN_TRANSLUCENCY][..., 0] == 255, (ins["d"] >= 65504).all(0))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. resolve
def resolve(be, shadow, lighting, mode, channels, n=None):
    """one nrdHipResolveShadowLights launch through the C-ABI into a stamped output"""
    h, w = lighting.shape[-3:-1]
    view, big = be.padded((h, w, channels), "float32", PAD, STAMP32)
    t, desc, keep = frontend.describe_resolve_shadow_lights(shadow, lighting, mode=mode, lights_num=n, out=view, lib=be.lib)
    assert RC(be.lib.nrdHipResolveShadowLights(C.byref(desc), None)) == RC.SUCCESS, be.lib.nrdHipGetLastFrontEndError()
    got = be.down(t).copy()
    assert_whole(be, big, got, np.array(STAMP32, f32), False, "resolve out")
    return got


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3, 6])
def test_resolve_per_light_against_the_model(backend, n):
    """sum( L_i * s_i ) from R8_UNORM and RGBA8_UNORM shadow stacks, lighting as RGBA32_SFLOAT and RGB32_SFLOAT, into RGBA32_SFLOAT and RGB32_SFLOAT: N = 3 and N = 6 (a batch and
    a remainder), every layer gapped and padded (NaN lighting, stamped shadows around the rects)"""
    be = Backend(backend)
    w, h = W1, H1
    rng = np.random.RandomState(20 + n)
    lighting = rng.uniform(0.0, 4.0, (n, h, w, 4)).astype(f32)
    for shadows in (rng.randint(0, 256, (n, h, w)).astype(np.uint8), rng.randint(0, 256, (n, h, w, 4)).astype(np.uint8)):
        want = M.resolve_per_light(shadows, lighting)
        for lc in (4, 3):
            for oc in (4, 3):
                got = resolve(be, up_stack(be, shadows, fill=0xA5), up_stack(be, np.ascontiguousarray(lighting[..., :lc])), SM.PER_LIGHT, oc)
                assert_bits(got, want[..., :oc], "PER_LIGHT resolve, N = %d, %s shadows, lighting x%d -> out x%d vs M" % (n, "R8" if shadows.ndim == 3 else "RGBA8", lc, oc))
    res = frontend.resolve_shadow_lights(be.up(shadows), be.up(lighting), lib=be.lib)
    assert_bits(be.down(res), want, "frontend.resolve_shadow_lights vs M")


@pytest.mark.parametrize("backend", BACKENDS)
def test_resolve_combined_against_the_model(backend):
    """Lsum.rgb * s.yzw, s.x from one RGBA8_UNORM plane: every UNORM8 code occurs"""
    be = Backend(backend)
    w, h = W1, H1
    rng = np.random.RandomState(30)
    lsum = rng.uniform(0.0, 40.0, (h, w, 4)).astype(f32)
    shadow = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    assert len(np.unique(shadow)) == 256
    want = M.resolve_combined(shadow, lsum)
    for lc in (4, 3):
        for oc in (4, 3):
            got = resolve(be, be.up_pitched(shadow, PAD), be.up_pitched(np.ascontiguousarray(lsum[..., :lc]), PAD), SM.COMBINED, oc, n=5)
            assert_bits(got, want[..., :oc], "COMBINED resolve, Lsum x%d -> out x%d vs M" % (lc, oc))
    res = frontend.resolve_shadow_lights(be.up(shadow), be.up(lsum), mode=SM.COMBINED, lib=be.lib)
    assert_bits(be.down(res), want, "frontend.resolve_shadow_lights (COMBINED) vs M")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. validation
def _np_plane(a, fmt, **kw):
    return TPR._plane(a, fmt, **kw)


class HostCase:
    """valid descriptors over host arrays (three lights: local, directional, local; 64 x 32) that a test mutates; the outputs are stamped and compared after every refused call"""

    W, H, N = 64, 32, 3

    def __init__(self):
        n, h, w = self.N, self.H, self.W
        self.table = frontend.shadow_lights(lights_of(n))
        self.d, self.dl, self.wt = np.ones((n, h, w), f32), np.full((n, h, w), 2.0, f32), np.ones((n, h, w), f32)
        self.rgba, self.rgb = np.ones((n, h, w, 4), f32), np.ones((n, h, w, 3), f32)
        self.pen, self.tr = np.full((n, h, w), STAMP16, np.float16), np.full((n, h, w, 4), STAMP8, np.uint8)
        self.sum, self.out = np.full((h, w, 4), STAMP32, f32), np.full((h, w, 4), STAMP32, f32)
        self.sh8, self.sh32 = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w, 4), np.uint8)

    def pack_desc(self, mode):
        d = api.HipShadowLightsPackDesc()
        d.mode, d.lightsNum, d.lights = int(mode), self.N, self.table
        d.distanceToOccluder, d.distanceToOccluderLayerBytes = _np_plane(self.d[0], F.R32_SFLOAT), self.d.strides[0]
        d.distanceToLight, d.distanceToLightLayerBytes = _np_plane(self.dl[0], F.R32_SFLOAT), self.dl.strides[0]
        d.outPenumbra, d.outPenumbraLayerBytes = _np_plane(self.pen[0], F.R16_SFLOAT), self.pen.strides[0]
        d.outTranslucency, d.outTranslucencyLayerBytes = _np_plane(self.tr[0], F.RGBA8_UNORM), self.tr.strides[0]
        if mode == SM.COMBINED:
            d.lighting, d.lightingLayerBytes = _np_plane(self.rgba[0], F.RGBA32_SFLOAT), self.rgba.strides[0]
            d.weight, d.weightLayerBytes = _np_plane(self.wt[0], F.R32_SFLOAT), self.wt.strides[0]
            d.outLightingSum = _np_plane(self.sum, F.RGBA32_SFLOAT)
        else:
            d.translucency, d.translucencyLayerBytes = _np_plane(self.rgba[0], F.RGBA32_SFLOAT), self.rgba.strides[0]
        return d

    def resolve_desc(self, mode):
        d = api.HipShadowLightsResolveDesc()
        d.mode, d.lightsNum = int(mode), self.N
        d.shadow, d.shadowLayerBytes = (_np_plane(self.sh32[0], F.RGBA8_UNORM), self.sh32.strides[0]) if mode == SM.COMBINED else (_np_plane(self.sh8[0], F.R8_UNORM), self.sh8.strides[0])
        d.lighting, d.lightingLayerBytes = _np_plane(self.rgba[0], F.RGBA32_SFLOAT), self.rgba.strides[0]
        d.out = _np_plane(self.out, F.RGBA32_SFLOAT)
        return d

    def untouched(self):
        return (self.pen == np.float16(STAMP16)).all() and (self.tr == STAMP8).all() and (self.sum == f32(STAMP32)).all() and (self.out == f32(STAMP32)).all()


def _set(obj, path, value):
    names = path.split(".")
    for name in names[:-1]:
        obj = getattr(obj, name)
    setattr(obj, names[-1], value)


@pytest.mark.parametrize("which", ["emu", "product"])
def test_validation_rules_name_the_field_and_touch_nothing(which):
    """every rule of the header comment: the stated code, a text that names the field, no output byte touched. On the emulated device code (where an accepted call would write) and
    on the product library with no GPU present (all of it happens in front of the first HIP call)"""
    lib = Backend("emu").lib if which == "emu" else api.load_library()
    case = HostCase()
    layer = case.W * case.H

    def run(kind, mode, mutate, code, *words):
        d = case.pack_desc(mode) if kind == "pack" else case.resolve_desc(mode)
        table = frontend.shadow_lights(lights_of(case.N))
        if kind == "pack":
            d.lights = table
        mutate(d, table) if kind == "pack" else mutate(d)
        fn = lib.nrdHipPackShadowLights if kind == "pack" else lib.nrdHipResolveShadowLights
        got, text = RC(fn(C.byref(d), None)), lib.nrdHipGetLastFrontEndError().decode()
        assert got == code and all(word in text for word in words) and text.startswith("nrdHip%sShadowLights" % ("Pack" if kind == "pack" else "Resolve")), (kind, mode, got, text, words)
        assert case.untouched(), text

    inv, uns = RC.INVALID_ARGUMENT, RC.UNSUPPORTED
    field = lambda path, value: (lambda d, *t: _set(d, path, value))
    light = lambda i, name, value: (lambda d, t: setattr(t[i], name, value))
    for mode in (SM.PER_LIGHT, SM.COMBINED):
        # counts, types, modes, reserved
        run("pack", mode, field("lightsNum", 0), inv, "lightsNum")
        run("pack", mode, field("lightsNum", 33), inv, "lightsNum")
        run("pack", mode, field("mode", 2), inv, "mode")
        run("pack", mode, field("lights", None), inv, "lights")
        run("pack", mode, light(1, "type", 2), inv, "lights[1].type")
        run("pack", mode, light(2, "reserved", 1), inv, "lights[2].reserved")
        # parameters of the type that uses them (light 0 and 2 are LOCAL, light 1 is DIRECTIONAL)
        for bad in (float("nan"), -1.0, float("inf")):
            run("pack", mode, light(1, "tanOfLightAngularRadius", bad), inv, "lights[1].tanOfLightAngularRadius")
            run("pack", mode, light(2, "lightSize", bad), inv, "lights[2].lightSize")
        # required planes
        run("pack", mode, field("distanceToOccluder.data", None), inv, "distanceToOccluder")
        run("pack", mode, field("distanceToLight.data", None), inv, "distanceToLight", "LOCAL")
        run("pack", mode, field("outPenumbra.data", None), inv, "outPenumbra")
        # layer strides
        run("pack", mode, field("distanceToOccluderLayerBytes", layer * 4 - 4), inv, "distanceToOccluderLayerBytes", "rowPitchBytes")
        run("pack", mode, field("distanceToOccluderLayerBytes", layer * 4 + 2), inv, "distanceToOccluderLayerBytes", "multiple of 4")
        run("pack", mode, field("distanceToOccluderLayerBytes", 0), inv, "distanceToOccluderLayerBytes")
        run("pack", mode, field("distanceToLightLayerBytes", layer * 4 - 4), inv, "distanceToLightLayerBytes")
        # sizes, pitches, alignment, formats
        run("pack", mode, field("distanceToLight.width", case.W - 1), inv, "distanceToLight", "size")
        run("pack", mode, field("outPenumbra.rowPitchBytes", case.W * 2 - 2), inv, "outPenumbra", "row pitch")
        run("pack", mode, field("distanceToOccluder.data", case.d.ctypes.data + 2), inv, "distanceToOccluder", "multiple")
        run("pack", mode, field("distanceToOccluder.format", int(F.R16_SFLOAT)), uns, "distanceToOccluder", "format")
        run("pack", mode, field("outPenumbra.format", int(F.R16_UNORM)), uns, "outPenumbra", "format")
        run("pack", mode, field("outTranslucency.format", int(F.RGBA8_SNORM)), uns, "outTranslucency", "format")
    per, com = SM.PER_LIGHT, SM.COMBINED
    plane = lambda a, fmt: _np_plane(a, fmt)
    # the light's unused parameter is not looked at
    ok = lambda d, t: (setattr(t[1], "lightSize", float("nan")), setattr(t[0], "tanOfLightAngularRadius", -1.0))
    if which == "emu":  # (an accepted descriptor launches: over host arrays that is for the emulated device code alone)
        d = case.pack_desc(per)
        table = frontend.shadow_lights(lights_of(case.N))
        ok(d, table)
        d.lights = table
        assert RC(lib.nrdHipPackShadowLights(C.byref(d), None)) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()
        case.pen[:], case.tr[:] = STAMP16, STAMP8  # (the call wrote them)
    # PER_LIGHT: translucency with outTranslucency; the planes it does not take; the output strides
    run("pack", per, field("translucency.data", None), inv, "translucency", "outTranslucency")
    run("pack", per, field("weight", plane(case.wt[0], F.R32_SFLOAT)), inv, "weight")
    run("pack", per, field("lighting", plane(case.rgba[0], F.RGBA32_SFLOAT)), inv, "lighting")

    def translucency_alone(d, *t):
        d.outTranslucency = api.HipPlaneDesc()
    run("pack", per, translucency_alone, inv, "translucency", "outTranslucency")
    run("pack", per, field("outLightingSum", plane(case.sum, F.RGBA32_SFLOAT)), inv, "outLightingSum")
    run("pack", per, field("translucencyLayerBytes", layer * 16 + 8), inv, "translucencyLayerBytes", "16")
    run("pack", per, field("translucencyLayerBytes", layer * 16 - 16), inv, "translucencyLayerBytes", "rowPitchBytes")
    run("pack", per, field("outPenumbraLayerBytes", layer * 2 - 4), inv, "outPenumbraLayerBytes", "rowPitchBytes")
    run("pack", per, field("outPenumbraLayerBytes", layer * 2 + 2), inv, "outPenumbraLayerBytes", "multiple of 4")
    run("pack", per, field("outTranslucencyLayerBytes", layer * 4 - 4), inv, "outTranslucencyLayerBytes")
    run("pack", per, field("translucency.format", int(F.RG32_SFLOAT)), uns, "translucency", "format")
    # COMBINED: its required planes, the plane it does not take
    run("pack", com, field("lighting.data", None), inv, "lighting")
    run("pack", com, field("outTranslucency.data", None), inv, "outTranslucency")
    run("pack", com, field("outLightingSum.data", None), inv, "outLightingSum")
    run("pack", com, field("translucency", plane(case.rgba[0], F.RGBA32_SFLOAT)), inv, "translucency")
    run("pack", com, field("lightingLayerBytes", layer * 16 + 4), inv, "lightingLayerBytes", "16")
    run("pack", com, field("weightLayerBytes", layer * 4 - 4), inv, "weightLayerBytes")
    run("pack", com, field("weight.format", int(F.R16_SFLOAT)), uns, "weight", "format")
    run("pack", com, field("outLightingSum.format", int(F.RGBA16_SFLOAT)), uns, "outLightingSum", "format")
    run("pack", com, field("outLightingSum.height", case.H - 1), inv, "outLightingSum", "size")

    def rgb_lighting(d, *t):  # an RGB32_SFLOAT stack: the stride is held to a multiple of 4, not of 16
        d.lighting, d.lightingLayerBytes = plane(case.rgb[0], F.RGB32_SFLOAT), layer * 12 + 2
    run("pack", com, rgb_lighting, inv, "lightingLayerBytes", "multiple of 4")
    # resolve
    for mode in (per, com):
        run("resolve", mode, field("lightsNum", 0), inv, "lightsNum")
        run("resolve", mode, field("lightsNum", 33), inv, "lightsNum")
        run("resolve", mode, field("mode", 7), inv, "mode")
        for name in ("shadow", "lighting", "out"):
            run("resolve", mode, field(name + ".data", None), inv, name)
        run("resolve", mode, field("out.format", int(F.RGBA16_SFLOAT)), uns, "out", "format")
        run("resolve", mode, field("lighting.format", int(F.RG32_SFLOAT)), uns, "lighting", "format")
        run("resolve", mode, field("lighting.width", case.W + 1), inv, "lighting", "size")
    run("resolve", com, field("shadow", plane(case.sh8[0], F.R8_UNORM)), uns, "shadow", "format")
    run("resolve", per, field("shadowLayerBytes", layer - 4), inv, "shadowLayerBytes", "rowPitchBytes")
    run("resolve", per, field("shadowLayerBytes", layer + 1), inv, "shadowLayerBytes", "multiple of 4")
    run("resolve", per, field("lightingLayerBytes", layer * 16 + 8), inv, "lightingLayerBytes", "16")
    assert RC(lib.nrdHipPackShadowLights(None, None)) == inv and RC(lib.nrdHipResolveShadowLights(None, None)) == inv
    # with one light no stride is looked at, and valid descriptors are accepted (launched on the emulated device code alone: the arrays are host memory)
    if which == "emu":
        for mode in (per, com):
            d = case.pack_desc(mode)
            d.lightsNum, d.distanceToOccluderLayerBytes, d.outPenumbraLayerBytes = 1, 3, 1
            assert RC(lib.nrdHipPackShadowLights(C.byref(d), None)) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()
            assert RC(lib.nrdHipResolveShadowLights(C.byref(case.resolve_desc(mode)), None)) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()


def test_symbols_structs_and_header():
    lib = api.load_library()
    for name in ("nrdHipPackShadowLights", "nrdHipResolveShadowLights"):
        assert name in api.NRD_HIP_SYMBOLS and getattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "NRDHip.h")).read()
    assert "uint32_t nrdHipPackShadowLights(const NrdHipShadowLightsPackDesc* desc, void* hipStream);" in hdr
    assert "uint32_t nrdHipResolveShadowLights(const NrdHipShadowLightsResolveDesc* desc, void* hipStream);" in hdr
    assert "#define NRD_HIP_MAX_SHADOW_LIGHTS 32u" in hdr and api.MAX_SHADOW_LIGHTS == 32
    assert "sizeof(NrdHipShadowLight) == 16 && sizeof(NrdHipShadowLightsPackDesc) == 264 && sizeof(NrdHipShadowLightsResolveDesc) == 96" in hdr
    assert (C.sizeof(api.HipShadowLight), C.sizeof(api.HipShadowLightsPackDesc), C.sizeof(api.HipShadowLightsResolveDesc)) == (16, 264, 96)
    hpp = open(os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")).read()
    assert "PackShadowLights(const NrdHipShadowLightsPackDesc& desc)" in hpp and "ResolveShadowLights(const NrdHipShadowLightsResolveDesc& desc)" in hpp
    # strides supply the layer bytes
    d = np.zeros((3, 9, 16), f32)[:, :8, :12]
    res, desc, keep = frontend.describe_pack_shadow_lights([(LT.DIRECTIONAL, 0.1)] * 3, d, translucency=np.zeros((3, 8, 12, 3), f32))
    assert (desc.lightsNum, desc.distanceToOccluderLayerBytes, desc.distanceToOccluder.rowPitchBytes, desc.translucencyLayerBytes) == (3, 9 * 16 * 4, 64, 8 * 12 * 12)
    assert desc.translucency.format == int(F.RGB32_SFLOAT) and (desc.outPenumbraLayerBytes, desc.outTranslucencyLayerBytes) == (8 * 12 * 2, 8 * 12 * 4)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7. end to end (GPU)
@pytest.mark.gpu
def test_end_to_end_two_local_lights_through_sigma():
    """96 x 64, two local lights. PER_LIGHT: one SIGMA_SHADOW instance with maxStabilizedFrameNum = 0 (no temporal stabilisation: this library's form of the README's
    stabilizationStrength = 0) denoises the two packed layers one after the other, check_inputs() is clean for each, resolve_shadow_lights sums the lit radiance. Every byte
    -- the two OUT_SHADOW_TRANSLUCENCY planes and the resolved radiance -- equals the same flow fed with planes packed by the numpy model. Then once in COMBINED mode through
    SIGMA_SHADOW_TRANSLUCENCY."""
    import parity
    from raytracingdenoiser_amd import synth
    from raytracingdenoiser_amd.executor import HipExecutor

    w, h, n = 96, 64, 2
    be = Backend("hip")
    lights = [(LT.LOCAL, 0.5), (LT.LOCAL, 2.0)]
    frame = synth.render_frame(w, h, 0, want=("sigma",))
    rng = np.random.RandomState(40)
    z = np.abs(frame["viewz"].numpy())
    d = (rng.uniform(0.05, 4.0, (n, h, w)) * (1.0 + 0.05 * z)).astype(f32)
    d[rng.uniform(size=(n, h, w)) < 0.4] = MISS
    d[0, :, : w // 3], d[1, :, 2 * w // 3:] = MISS, 0.0
    ins = dict(d=d, dl=(d + rng.uniform(1.0, 20.0, (n, h, w))).astype(f32), lighting=rng.uniform(0.0, 3.0, (n, h, w, 4)).astype(f32))

    def flow(name, packed_layers, settings_overrides):
        """denoises every (IN_PENUMBRA[, IN_TRANSLUCENCY]) pair of `packed_layers` with ONE instance, returns the stacked OUT_SHADOW_TRANSLUCENCY planes"""
        inst = api.Instance([(0, parity.DENOISERS[name][0])])
        ex = HipExecutor(inst, w, h)
        (rt, dtype, ch, fmt), = parity.output_planes(name, w, h)
        outs = []
        for f, layer in enumerate(packed_layers):
            out = torch.zeros((h, w, ch), dtype=dtype, device="cuda")
            ex.bind(rt, out, fmt)
            for plane_rt, t, plane_fmt in parity.user_planes(name, frame):
                ex.bind(plane_rt, layer[plane_rt] if plane_rt in layer else t.cuda().contiguous(), plane_fmt)
            assert inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame, settings_overrides)) == api.Result.SUCCESS
            assert inst.set_common_settings(parity.common_settings(frame["camera"], frame["camera"], w, h, f)) == api.Result.SUCCESS
            check = ex.check_inputs()
            assert check, check.rules
            ex.denoise()
            torch.cuda.synchronize()
            outs.append(out)
        ex.destroy()
        return torch.stack(outs)

    lighting = torch.from_numpy(ins["lighting"]).cuda()
    # ---- per light
    packed = frontend.pack_shadow_lights(lights, torch.from_numpy(ins["d"]).cuda(), distance_to_light=torch.from_numpy(ins["dl"]).cuda())
    model_p = f16(np.stack([M.penumbra(l, ins["d"][i], ins["dl"][i]) for i, l in enumerate(lights)]))
    assert_bits(packed[R.IN_PENUMBRA][0].cpu().numpy(), model_p, "e2e: packed IN_PENUMBRA layers vs M")
    once = dict(maxStabilizedFrameNum=0)
    got = flow("SIGMA_SHADOW", [{R.IN_PENUMBRA: packed[R.IN_PENUMBRA][0][i]} for i in range(n)], once)
    want = flow("SIGMA_SHADOW", [{R.IN_PENUMBRA: torch.from_numpy(model_p[i]).cuda()} for i in range(n)], once)
    assert_bits(got.cpu().numpy(), want.cpu().numpy(), "e2e PER_LIGHT: OUT_SHADOW_TRANSLUCENCY of both lights, kernel-packed == model-packed")
    assert len(np.unique(got.cpu().numpy())) > 2  # (a denoised shadow, not a constant)
    lit = frontend.resolve_shadow_lights(got[..., 0], lighting)
    torch.cuda.synchronize()
    assert_bits(lit.cpu().numpy(), M.resolve_per_light(want[..., 0].cpu().numpy(), ins["lighting"]), "e2e PER_LIGHT: resolved radiance vs M on the model-fed flow")
    # ---- combined
    packed = frontend.pack_shadow_lights(lights, torch.from_numpy(ins["d"]).cuda(), distance_to_light=torch.from_numpy(ins["dl"]).cuda(), lighting=lighting, mode=SM.COMBINED)
    p, t, lsum = M.combined(lights, ins["d"], ins["dl"], ins["lighting"])
    model = {R.IN_PENUMBRA: torch.from_numpy(f16(p)).cuda(), R.IN_TRANSLUCENCY: torch.from_numpy(unorm8(t)).cuda()}
    got = flow("SIGMA_SHADOW_TRANSLUCENCY", [{rt: packed[rt][0] for rt in model}], once)
    want = flow("SIGMA_SHADOW_TRANSLUCENCY", [model], once)
    assert_bits(got.cpu().numpy(), want.cpu().numpy(), "e2e COMBINED: OUT_SHADOW_TRANSLUCENCY, kernel-packed == model-packed")
    lit = frontend.resolve_shadow_lights(got[0], packed["lighting_sum"][0], mode=SM.COMBINED, lights_num=n)
    torch.cuda.synchronize()
    assert_bits(lit.cpu().numpy(), M.resolve_combined(want[0].cpu().numpy(), lsum), "e2e COMBINED: resolved radiance vs M on the model-fed flow")


@pytest.mark.gpu
def test_captured_calls_replay_the_same_bytes():
    """the contract of the other front-end calls: no allocation, no synchronisation -- both calls are capturable by torch.cuda.graph and replay the same bytes"""
    be = Backend("hip")
    lights = lights_of(5)
    ins = scene(5, W0, H0, seed=50)
    dev = {k: torch.from_numpy(v).cuda() for k, v in ins.items()}
    kw = dict(distance_to_light=dev["dl"], lighting=dev["lighting"], mode=SM.COMBINED)
    packed = frontend.pack_shadow_lights(lights, dev["d"], **kw)
    shadow = torch.from_numpy(np.random.RandomState(51).randint(0, 256, (H0, W0, 4)).astype(np.uint8)).cuda()
    lit = frontend.resolve_shadow_lights(shadow, packed["lighting_sum"][0], mode=SM.COMBINED)
    torch.cuda.synchronize()
    eager = {k: t.cpu().numpy().copy() for k, (t, fmt) in packed.items()}
    eager_lit = lit.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frontend.pack_shadow_lights(lights, dev["d"], out=packed, **kw)
        frontend.resolve_shadow_lights(shadow, packed["lighting_sum"][0], mode=SM.COMBINED, out=lit)
    for t, fmt in packed.values():
        t.zero_()
    lit.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, (t, fmt) in packed.items():
        assert_bits(t.cpu().numpy(), eager[k], "captured nrdHipPackShadowLights == eager: %s" % k)
    assert_bits(lit.cpu().numpy(), eager_lit, "captured nrdHipResolveShadowLights == eager")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 8. C++
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "shadow_lights_integration.cpp")
CPP_EXE = os.path.join(ROOT, "tests", "cpp", "build", "shadow_lights_integration")


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


def test_cpp_integration_compiles_and_validates_on_the_host():
    _build_cpp()
    r = subprocess.run([CPP_EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host-only OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_integration_packs_and_resolves_lights():
    _build_cpp()
    r = subprocess.run([CPP_EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shadow lights integration OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------------- 9. static facts
def test_static_facts_of_the_shadow_light_kernels():
    """what the compiler made of the four kernels for gfx950 (tools/frontend_bench.py shadow_lights_isa(), the `isa_shadow_lights` object of profiles/frontend_bench.json): no
    scratch -- the light table is read from the kernel arguments in place -- and no LDS. VGPRs and waves per SIMD are printed and recorded, not bounded."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import frontend_bench

    facts = frontend_bench.shadow_lights_isa()
    assert set(facts) == {"pack_per_light", "pack_combined", "resolve_per_light", "resolve_combined"}
    for name, k in facts.items():
        print(name, k)
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0, (name, k)
        assert k["vgprs"] > 0 and k["waves_per_simd"] >= 1
        if name.startswith("resolve"):  # k / 255 is the codecs' exact three-operation division: no generic division, no reciprocal
            assert k["transcendental"] == 0 and k["v_div_scale_f32"] == 0, (name, k)
