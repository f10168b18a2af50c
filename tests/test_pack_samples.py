"""nrdHipPackInputsSamples (include/NRDHip.h, raytracingdenoiser_amd/frontend.py): many paths per pixel -- N sample layers per signal, reduced by the reference's rules (the mean of
the packed samples; for the specular hit distance NRD_FrontEnd_SpecHitDistAveraging_*: the smallest non-zero sample) and packed in the same launch.

As in tests/test_pack_resolve.py every comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU). Expected values never come
from the code under test:
  P  the kernels of the parent commit (nrdHipPackInputs / nrdHipPackInputsEx) on single-sample planes
  B  include/NRD.hip.h evaluated on the host by tests/cpp/frontend_check --dump-host (the `dump` fixture of tests/test_pack_resolve.py): the layers are np.rolls of its input
     columns, so the packed value of every sample is a row of the dump and the expectation is their float32 numpy sum in sample order, divided by float32( N )
  C  tests/frontend_model.py (float64) for the normalised hit distance of the diffuse signal (roughness 1), which the dump does not hold
  and float32 numpy restatements of NRD_FrontEnd_SpecHitDistAveraging_{Begin,Add,End} / NRD_FrontEnd_TrimHitDistance from their definitions (NRD.hlsli:693-716).
Bounds: those of check_pack in tests/test_pack_resolve.py -- bit for bit wherever a value is + - * / of fp32 values, one code of the stored format against C."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frontend_model as M
import test_pack_resolve as TPR
from raytracingdenoiser_amd import api, build as native_build, frontend, scene
from test_pack_resolve import BACKENDS, HDP, PACK_CALLS, Backend, assert_bits, assert_codes, f16, img, snorm16, unorm16

dump = TPR.dump  # the host dump of tests/cpp/frontend_check (a module-scoped fixture)

ROOT = TPR.ROOT
F, R, S, CB, RC = api.Format, api.ResourceType, api.SignalMode, api.CheckerboardMode, api.Result
f32 = np.float32
COUNT = TPR.COUNT
W1, H1 = 197, 61  # the ragged size of tests/test_pack_resolve.py: a 5-pixel last workgroup column, a 1-row last row of workgroups
W0, H0 = 67, 23
STAMP = 23130
NRD_INF = f32(1e6)
SHIFT = 1009  # layer k holds the dump's samples rolled by k * SHIFT rows (a prime: no two layers of a pixel hold the same sample)


# ---------------------------------------------------------------------------------------------------------------------------------------------- inputs
def rolled(d, name, k):
    return np.roll(d[name], k * SHIFT, axis=0)


def sample_layers(d, w, h, n, first=0):
    """([n, h, w, 4] radiance + hit distance, [n, h, w, 4] direction): layer s = the dump's input columns rolled by ( first + s ) * SHIFT rows"""
    zeros = np.zeros((COUNT, 1), f32)
    rad = np.stack([img(d, rolled(d, "radiance", first + k), rolled(d, "hitDist", first + k), w=w, h=h) for k in range(n)])
    dirn = np.stack([img(d, rolled(d, "direction", first + k), zeros, w=w, h=h) for k in range(n)])
    return rad, dirn


def mean32(parts):
    """( ( ( P_0 + P_1 ) + P_2 ) + ... ) / float( N ) in float32 numpy"""
    acc = np.asarray(parts[0], f32).copy()
    for p in parts[1:]:
        acc = acc + np.asarray(p, f32)
    out = acc / f32(len(parts))
    assert out.dtype == f32
    return out


def dump_mean(d, name, n, w, h, first=0):
    """the mean over n layers of the dump's fp32 packed rows `name`, as an [h, w, C] image"""
    return mean32([img(d, rolled(d, name, first + k), w=w, h=h) for k in range(n)])


def spec_hit_dist(hits):
    """H of NRDHip.h from the definitions of the three functions (NRD.hlsli:693-716): hits [N, ...] float32"""
    a = np.full(hits.shape[1:], NRD_INF, f32)  # Begin
    for h in hits:  # Add: min( a, h == 0 ? NRD_INF : h ), HLSL's / fminf's min (a NaN operand loses)
        a = np.fmin(a, np.where(h == 0, NRD_INF, h).astype(f32))
    return np.where(a == NRD_INF, f32(0), a).astype(f32)  # End


# ---------------------------------------------------------------------------------------------------------------------------------------------- running the kernels
def up_layers(be, a, pad, gap, fill=np.nan):
    """[N, H, W, 4] on the backend inside a wider allocation: rows `pad` texels longer than the plane, `gap` rows between the layers, everything around the rects = `fill`"""
    if a.ndim == 3:
        return be.up_pitched(a, pad) if pad else be.up(a)
    n, h, w, c = a.shape
    big = np.full((n, h + gap, w + pad, c), fill, dtype=a.dtype)
    big[:, :h, :w] = a
    big = big if be.name == "emu" else torch.from_numpy(big).cuda()
    return big[:, :h, :w]


def _layer_bytes(t):
    return 0 if t is None or t.ndim != 4 else (t.strides[0] if isinstance(t, np.ndarray) else t.stride(0) * t.element_size())


def samples_struct(diff=None, spec=None, trim=0.0):
    """api.HipFrontEndSamples from the uploaded (radiance_hitdist, direction) arrays of each signal, built here from their strides (not by frontend.pack_samples)"""
    s = api.HipFrontEndSamples()
    s.hitDistTrimThreshold = trim
    for arrays, dst in ((diff, s.diffuse), (spec, s.specular)):
        if arrays is not None:
            dst.samplesNum = arrays[0].shape[0] if arrays[0].ndim == 4 else 1
            dst.radianceHitDistLayerBytes, dst.directionLayerBytes = _layer_bytes(arrays[0]), _layer_bytes(arrays[1])
    return s


class Frame:
    """the G-buffer of tests/test_pack_resolve.py's pack tests at one size on one backend, and the calls on it. Outputs always live in wider, stamped allocations."""

    def __init__(self, be, d, w, h, pad=5):
        self.be, self.d, self.w, self.h, self.pad = be, d, w, h, pad
        self.ins = TPR.pack_inputs_of(d, w, h)
        self.dev = {k: be.up_pitched(v, pad) for k, v in self.ins.items()}
        self.rf0 = be.up_pitched(img(d, "Rf0", np.zeros((COUNT, 1), f32), w=w, h=h), pad)
        self.cs = TPR.frame_settings(w, h)

    def up(self, arrays, gap=3):
        """(radiance_hitdist, direction) numpy arrays ([H, W, 4] or [N, H, W, 4]) -> on the backend, padded"""
        return tuple(None if a is None else up_layers(self.be, a, self.pad, gap) for a in arrays)

    def call(self, dm, sm, diff=None, spec=None, entry="samples", samples="auto", cb=CB.OFF, frame_index=0, trim=0.0, demodulate=False, full=False, options="auto"):
        """one launch through the C-ABI. diff / spec: uploaded (radiance_hitdist, direction) pairs (default: the single-sample planes of the frame).
        entry: "plain" nrdHipPackInputs, "ex" nrdHipPackInputsEx, "samples" nrdHipPackInputsSamples; samples: "auto" (from the arrays' strides), None (NULL) or a struct.
        Returns ({ResourceType: plane}, {ResourceType: whole allocation}), downloaded."""
        be, dev, lib = self.be, self.dev, self.be.lib
        single = (dev["rad"], dev["direction"])
        diff, spec = diff or single, spec or single
        kw = dict(hit_dist_params=HDP, lib=lib)
        if dm is not None:
            kw["diffuse"] = dict(mode=dm, radiance_hitdist=diff[0], direction=diff[1])
        if sm is not None:
            kw["specular"] = dict(mode=sm, radiance_hitdist=spec[0], direction=spec[1])
        if full:
            kw.update(material_id=dev["material"], motion=dev["motion"], distance_to_occluder=dev["occluder"], translucency=dev["albedo"], tan_of_light_angular_radius=TPR.TAN_LIGHT)
        if demodulate:
            kw.update(albedo=dev["albedo"], rf0=self.rf0, common_settings=self.cs)
        probe = frontend.describe_pack(dev["nr"], dev["viewz"], **kw)[0]  # (shapes and dtypes of this call's outputs)
        out, bigs = {}, {}
        for rt, (t, fmt) in probe.items():
            name = frontend._dtype_name(t)
            view, bigs[rt] = be.padded(tuple(t.shape), name, self.pad, 0x5A if name == "uint8" else STAMP)
            out[rt] = (view, fmt)
        res, desc, keep = frontend.describe_pack(dev["nr"], dev["viewz"], out=out, **kw)
        opt = api.HipFrontEndOptions(int(cb), frame_index) if options == "auto" else options
        opt_ref = None if opt is None or (options == "auto" and cb == CB.OFF) else C.byref(opt)
        if entry == "plain":
            code = lib.nrdHipPackInputs(C.byref(desc), None)
        elif entry == "ex":
            code = lib.nrdHipPackInputsEx(C.byref(desc), opt_ref, None)
        else:
            if samples == "auto":
                samples = samples_struct(diff if dm is not None else None, spec if sm is not None else None, trim)
            code = lib.nrdHipPackInputsSamples(C.byref(desc), opt_ref, None if samples is None else C.byref(samples), None)
        assert RC(code) == RC.SUCCESS, lib.nrdHipGetLastFrontEndError()
        got = {rt: be.down(t).copy() for rt, (t, fmt) in res.items()}
        whole = {rt: be.down(b).copy() for rt, b in bigs.items()}
        for rt, big in whole.items():  # nothing outside the rect is ever written (checkerboard calls leave texels inside it unwritten: compared by their tests)
            want = np.full(big.shape, 0x5A if big.dtype == np.uint8 else STAMP, dtype=big.dtype)
            want[:self.h, :self.w] = got[rt]
            assert np.array_equal(big.view(np.uint8), want.view(np.uint8)), "bytes outside the rect were written: %s" % rt.name
        return got, whole


def assert_same_planes(a, b, what):
    assert set(a) == set(b)
    for rt in a:
        assert_bits(a[rt], b[rt], "%s: %s" % (what, rt.name))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1. N = 1 is the existing call
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_sample_is_the_existing_call(backend, dump):
    """samples = NULL, a zeroed struct and samplesNum = 1 against nrdHipPackInputsEx on the same planes, every entry of PACK_CALLS, plain, checkerboarded (BLACK) and
    demodulating: every output plane, the whole stamped allocation, bit for bit"""
    fr = Frame(Backend(backend), dump, W1, H1)
    one = api.HipFrontEndSamples()
    one.diffuse.samplesNum = one.specular.samplesNum = 1
    for dm, sm, full in PACK_CALLS:
        for kw in (dict(), dict(cb=CB.BLACK, frame_index=1), dict(demodulate=True)):
            _, old = fr.call(dm, sm, entry="ex", full=full, **kw)
            for what, s in (("NULL", None), ("zeroed", api.HipFrontEndSamples()), ("samplesNum = 1", one)):
                _, new = fr.call(dm, sm, samples=s, full=full, **kw)
                assert_same_planes(new, old, "nrdHipPackInputsSamples(%s) vs nrdHipPackInputsEx, %s / %s %s" % (what, dm.name, sm.name if sm else "-", kw))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2. two equal layers
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_equal_layers_are_the_plain_call(backend, dump):
    """( P + P ) / 2 is exact, and the smallest of two equal non-zero hit distances is that hit distance: N = 2 with both layers equal is nrdHipPackInputs bit for bit, in
    every mode, with and without demodulation (the dump's hit distances are finite and below NRD_INF, where the specular rule is the identity)"""
    fr = Frame(Backend(backend), dump, W1, H1)
    hit = fr.ins["rad"][..., 3]
    assert np.isfinite(hit).all() and hit.max() < NRD_INF
    twice = fr.up((np.stack([fr.ins["rad"]] * 2), np.stack([fr.ins["direction"]] * 2)))
    for dm, sm, full in PACK_CALLS:
        for demodulate in (False, True):
            old, _ = fr.call(dm, sm, entry="plain", full=full, demodulate=demodulate)
            new, _ = fr.call(dm, sm, diff=twice, spec=twice, full=full, demodulate=demodulate)
            assert_same_planes(new, old, "two equal layers vs nrdHipPackInputs, %s / %s%s" % (dm.name, sm.name if sm else "-", ", demodulated" if demodulate else ""))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. the mean
def check_means(be, d, got, n, w, h, which=("DIFF", "SPEC"), first=0, zeroed=None):
    """the planes of the PACK_CALLS calls with n rolled layers per signal ({(call, ResourceType): plane}) against B and C. zeroed: {dump column: [(y, x, layer)]} -- samples whose
    packed contribution is replaced by zeros (test 6)."""
    def mean_of(name, channels=slice(None)):
        parts = [img(d, rolled(d, name, first + k), w=w, h=h)[..., channels].copy() for k in range(n)]
        for y, x, k in (zeroed or {}).get(name, ()):
            parts[k][y, x] = 0
        return mean32(parts)

    xyz = slice(0, 3)
    for sig in which:
        r = lambda name: R["IN_%s_%s" % (sig, name)]
        if (0, r("RADIANCE_HITDIST")) in got:
            assert_bits(got[(0, r("RADIANCE_HITDIST"))][..., :3], f16(mean_of("reblurPacked", xyz)), "N = %d %s REBLUR radiance .xyz vs B" % (n, sig))
        if (1, r("SH0")) in got:
            assert_bits(got[(1, r("SH0"))][..., :3], f16(mean_of("sh0", xyz)), "N = %d %s REBLUR SH0 .xyz vs B" % (n, sig))
            assert_bits(got[(1, r("SH1"))], f16(mean_of("sh1")), "N = %d %s REBLUR SH1 vs B" % (n, sig))
        if (4, r("SH0")) in got:
            assert_bits(got[(4, r("SH0"))][..., :3], f16(mean_of("relaxPacked", xyz)), "N = %d %s RELAX SH0 .xyz vs B" % (n, sig))
            assert_bits(got[(4, r("SH1"))], f16(mean_of("relaxSh1")), "N = %d %s RELAX SH1 vs B" % (n, sig))
    if (3, R.IN_SPEC_RADIANCE_HITDIST) in got and "SPEC" in which:
        assert_bits(got[(3, R.IN_SPEC_RADIANCE_HITDIST)][..., :3], f16(mean_of("relaxPacked", xyz)), "N = %d SPEC RELAX radiance .xyz vs B" % n)
    if "DIFF" not in which or zeroed:
        return
    # RELAX diffuse .w: the mean of the clamped hit distances, float32 numpy
    assert_bits(got[(4, R.IN_DIFF_SH0)][..., 3], f16(mean_of("relaxPacked", 3)), "N = %d DIFF RELAX SH0 .w = the mean of the clamped hit distances" % n)
    assert_bits(got[(5, R.IN_DIFF_RADIANCE_HITDIST)], f16(mean_of("relaxPacked")), "N = %d DIFF RELAX radiance vs B" % n)
    # REBLUR diffuse hit distance: normalised per sample with roughness 1 (C), then the mean
    z = d["viewZ"][:, 0].astype(np.float64)
    nhd = [M.reblur_get_norm_hit_dist(rolled(d, "hitDist", first + k)[:, 0].astype(np.float64), z, HDP, 1.0) for k in range(n)]
    crop = lambda a: img(d, a, w=w, h=h)
    mean_nhd = sum(nhd) / n
    assert_codes(got[(0, R.IN_DIFF_RADIANCE_HITDIST)][..., 3], f16(crop(mean_nhd)), "N = %d IN_DIFF_RADIANCE_HITDIST .w vs C" % n)
    assert_codes(got[(1, R.IN_DIFF_SH0)][..., 3], f16(crop(mean_nhd)), "N = %d IN_DIFF_SH0 .w vs C" % n)
    assert_codes(got[(2, R.IN_DIFF_HITDIST)], unorm16(crop(mean_nhd)), "N = %d IN_DIFF_HITDIST vs C" % n, unorm=True)
    dirocc = sum(M.reblur_pack_directional_occlusion(rolled(d, "direction", first + k).astype(np.float64), nhd[k]) for k in range(n)) / n
    assert_codes(got[(3, R.IN_DIFF_DIRECTION_HITDIST)], snorm16(crop(dirocc)), "N = %d IN_DIFF_DIRECTION_HITDIST vs C" % n)


def run_calls(fr, diff, spec, calls=range(len(PACK_CALLS)), **kw):
    got = {}
    for call in calls:
        dm, sm, full = PACK_CALLS[call]
        planes, _ = fr.call(dm, sm, diff=diff, spec=spec, full=full, **kw)
        got.update({(call, rt): a for rt, a in planes.items()})
    return got


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3, 5])
def test_the_mean_against_the_host_dump(backend, n, dump):
    """N = 3 (fewer samples than a batch of four) and N = 5 (a batch and a remainder), 197 x 61, every mode"""
    be = Backend(backend)
    fr = Frame(be, dump, W1, H1)
    layers = fr.up(sample_layers(dump, W1, H1, n))
    got = run_calls(fr, layers, layers)
    check_means(be, dump, got, n, W1, H1)
    for a in got.values():
        assert np.isfinite(a.astype(f32)).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. the specular hit distance
HIT_MODES = [S.REBLUR_RADIANCE, S.REBLUR_SH, S.REBLUR_OCCLUSION, S.RELAX_RADIANCE, S.RELAX_SH]


def constructed_hits(w, h):
    """[4, h, w] hit distances from a small set with exact zeros, and the cases of the issue at known pixels of row 0"""
    rng = np.random.RandomState(5)
    values = np.array([0.0, 0.0, 0.5, 2.0, 7.25, 30.0], f32)
    hits = values[rng.randint(0, len(values), size=(4, h, w))]
    hits[:, 0, 0] = 0.0                              # all four zero
    hits[:, 0, 1] = (0.0, 0.0, 7.25, 0.0)            # exactly one non-zero
    hits[:, 0, 2] = (0.5, 2.0, 30.0, 7.25)           # the smallest in layer 0
    hits[:, 0, 3] = (30.0, 2.0, 7.25, 0.5)           # ... in layer 3
    hits[:, 0, 4] = (30.0, 2.0, 2.0, 7.25)           # tied across two layers
    hits[:, 0, 5] = (7.25, np.nan, 2.0, 30.0)        # a NaN next to finite samples
    hits[:, 0, 6] = (0.0, 2e6, 0.0, 0.0)             # above NRD_INF, the only non-zero one
    hits[:, 0, 7] = (0.0, 2.0, 0.0, 0.5)             # zeros between the non-zero ones
    return hits


@pytest.mark.parametrize("backend", BACKENDS)
def test_specular_hit_distance_is_the_smallest_non_zero_sample(backend, dump):
    """N = 4: the hit-distance channel of the specular signal is, bit for bit, the one the parent's nrdHipPackInputs writes for a single-sample plane holding H (numpy, from the
    definitions of NRD_FrontEnd_SpecHitDistAveraging_*); the diffuse signal on the same layers does not follow that rule"""
    be = Backend(backend)
    w, h = W0, H0
    fr = Frame(be, dump, w, h)
    rad, dirn = sample_layers(dump, w, h, 4)
    hits = constructed_hits(w, h)
    rad[..., 3] = hits
    H = spec_hit_dist(hits)
    zero, nonzero = (hits == 0).sum(0), np.where(hits == 0, np.inf, hits)
    assert (zero == 4).sum() > 1 and (zero == 3).sum() > 10 and (H[zero == 4] == 0).all() and H[0, 6] == 0 and H[0, 5] == 2.0 and H[0, 7] == 0.5
    for layer in (0, 3):  # pixels whose smallest non-zero sample sits in the first / the last layer alone
        assert ((np.nanargmin(nonzero, 0) == layer) & ((nonzero == np.nanmin(nonzero, 0)).sum(0) == 1) & (zero < 4)).sum() > 50
    assert (((nonzero == np.nanmin(nonzero, 0)).sum(0) == 2) & (zero < 4)).sum() > 50  # ties
    layers = fr.up((rad, dirn))
    single = rad[0].copy()
    single[..., 3] = H
    single = fr.up((single, dirn[0]))
    for mode in HIT_MODES:
        want, _ = fr.call(mode, mode, diff=single, spec=single, entry="plain")
        got, _ = fr.call(mode, mode, diff=layers, spec=layers)
        spec_rt, diff_rt = frontend.signal_slots("specular", mode, "IN")[0], frontend.signal_slots("diffuse", mode, "IN")[0]
        channel = (lambda a: a) if mode == S.REBLUR_OCCLUSION else (lambda a: a[..., 3])
        assert_bits(channel(got[spec_rt]), channel(want[spec_rt]), "%s: specular hit distance == nrdHipPackInputs on H" % mode.name)
        assert np.isfinite(channel(got[spec_rt]).astype(f32)).all()
        differs = channel(got[diff_rt]) != channel(want[diff_rt])
        print("%s: the diffuse hit distance differs from the rule's at %.1f %% of the pixels" % (mode.name, 100.0 * differs.mean()))
        assert differs.mean() > 0.5, "the diffuse signal must be the mean, not the specular rule"


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. trim
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [1, 3])
def test_trim_threshold_is_a_per_sample_pre_trim(backend, n, dump):
    """hitDistTrimThreshold = t == threshold 0 on layers whose hit distances were trimmed with numpy (h < t ? 0 : h): bit for bit, every output plane"""
    be = Backend(backend)
    w, h = W0, H0
    fr = Frame(be, dump, w, h)
    rad, dirn = sample_layers(dump, w, h, n)
    t = f32(np.median(rad[..., 3]))
    trimmed = rad.copy()
    trimmed[..., 3] = np.where(rad[..., 3] < t, f32(0), rad[..., 3])
    share = (trimmed[..., 3] == 0).mean()
    assert 0.3 < share < 0.7 and rad[..., 3].max() < NRD_INF, share
    if n == 1:
        rad, dirn, trimmed = rad[0], dirn[0], trimmed[0]
    a, b = fr.up((rad, dirn)), fr.up((trimmed, dirn))
    for dm, sm in ((S.REBLUR_RADIANCE, S.REBLUR_RADIANCE), (S.RELAX_SH, S.RELAX_SH), (S.REBLUR_OCCLUSION, S.REBLUR_SH)):
        got, _ = fr.call(dm, sm, diff=a, spec=a, trim=float(t))
        want, _ = fr.call(dm, sm, diff=b, spec=b)
        assert_same_planes(got, want, "trim %.3g, N = %d, %s / %s" % (t, n, dm.name, sm.name))
        untrimmed, _ = fr.call(dm, sm, diff=a, spec=a)
        assert any(not np.array_equal(got[rt], untrimmed[rt]) for rt in got), "the threshold changed nothing"


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. per-sample sanitising
@pytest.mark.parametrize("backend", BACKENDS)
def test_invalid_samples_are_sanitised_one_by_one(backend, dump):
    """N = 3: one layer of a pixel holds NaN or +Inf radiance, or a NaN direction. The texel is the mean with that sample's packed contribution replaced by what the packer
    returns for it (zeros) -- not a zero texel, not NaN"""
    be = Backend(backend)
    w, h, n = W0, H0, 3
    fr = Frame(be, dump, w, h)
    rad, dirn = sample_layers(dump, w, h, n)
    rad[1, 1, 1, 0] = np.nan
    rad[0, 2, 2, 1] = np.inf
    rad[2, 3, 66, :3] = np.nan
    dirn[2, 4, 4, 2] = np.nan
    bad_radiance, bad_direction = [(1, 1, 1), (2, 2, 0), (3, 66, 2)], [(4, 4, 2)]
    zeroed = {"reblurPacked": bad_radiance, "sh0": bad_radiance, "relaxPacked": bad_radiance, "sh1": bad_radiance + bad_direction, "relaxSh1": bad_radiance + bad_direction}
    layers = fr.up((rad, dirn))
    got = run_calls(fr, layers, layers, calls=(0, 1, 4))
    check_means(be, dump, got, n, w, h, zeroed=zeroed)
    for (call, rt), a in got.items():
        a = a.astype(f32)
        assert np.isfinite(a).all(), rt.name
        if rt in (R.IN_DIFF_RADIANCE_HITDIST, R.IN_SPEC_RADIANCE_HITDIST, R.IN_DIFF_SH0, R.IN_SPEC_SH0):
            for y, x, k in bad_radiance:
                assert a[y, x, 0] > 0, "%s: one invalid sample zeroed the texel" % rt.name


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7. layout
@pytest.mark.parametrize("backend", BACKENDS)
def test_layer_strides_pitches_and_mixed_sample_counts(backend, dump):
    """layers with gaps between them and rows longer than the plane (everything around the rects is NaN) give the planes of dense layers; diffuse 1 / specular 5 samples in one
    call: the diffuse planes are the plain call's, the specular ones meet the expectation of five layers. (Frame.call holds every output's surroundings against the stamp.)"""
    be = Backend(backend)
    w, h, n = W1, H1, 5
    fr = Frame(be, dump, w, h)
    rad, dirn = sample_layers(dump, w, h, n)
    gapped = fr.up((rad, dirn), gap=3)
    dense = (be.up(rad), be.up(dirn))
    assert _layer_bytes(gapped[0]) == (h + 3) * (w + fr.pad) * 16 and _layer_bytes(dense[0]) == h * w * 16
    for call in (0, 1, 4):
        dm, sm, full = PACK_CALLS[call]
        a, _ = fr.call(dm, sm, diff=gapped, spec=gapped)
        b, _ = fr.call(dm, sm, diff=dense, spec=dense)
        assert_same_planes(a, b, "gapped, pitched layers vs dense ones, %s" % dm.name)
    one = fr.up((rad[0], dirn[0]))
    got = run_calls(fr, one, gapped)
    old = run_calls(fr, one, one, entry="plain")
    for key in got:
        if not key[1].name.startswith("IN_SPEC"):  # the diffuse planes, the G-buffer and the SIGMA planes
            assert_bits(got[key], old[key], "diffuse 1 / specular 5: %s (call %d) == nrdHipPackInputs" % (key[1].name, key[0]))
    check_means(be, dump, got, n, w, h, which=("SPEC",))


@pytest.mark.parametrize("backend", BACKENDS)
def test_sixty_four_layers(backend, dump):
    """samplesNum = 64, the largest count, at 67 x 23: sixteen full batches"""
    be = Backend(backend)
    w, h, n = W0, H0, 64
    fr = Frame(be, dump, w, h)
    layers = fr.up(sample_layers(dump, w, h, n), gap=0)
    got = run_calls(fr, layers, layers)
    check_means(be, dump, got, n, w, h)


@pytest.mark.parametrize("backend", BACKENDS)
def test_checkerboarded_layers(backend, dump):
    """checkerboarding with N = 3: the unselected pixels of every layer hold NaN and no output depends on them; a selected pixel's texel is the texel of the call without
    checkerboarding (held against B and C above), at column x >> 1; the right half and, at this odd width, the sourceless last column of the left half stay stamped"""
    be = Backend(backend)
    w, h, n = W0, H0, 3
    fr = Frame(be, dump, w, h)
    rad, dirn = sample_layers(dump, w, h, n)
    full_layers = fr.up((rad, dirn))
    yy, xx = np.mgrid[0:h, 0:w]
    for cb_mode, frame_index in ((CB.BLACK, 0), (CB.WHITE, 1), (CB.BLACK, 1)):
        cells = {"diffuse": 0, "specular": 1} if cb_mode == CB.BLACK else {"diffuse": 1, "specular": 0}
        sig = {}
        for which, cell in cells.items():
            has = ((((xx ^ yy) ^ frame_index) & 1) == cell)[None, ..., None]
            sig[which] = fr.up((np.where(has, rad, f32(np.nan)).astype(f32), np.where(has, dirn, f32(np.nan)).astype(f32)))
        for mode in HIT_MODES:
            want, _ = fr.call(mode, mode, diff=full_layers, spec=full_layers)
            dev = fr.dev
            kw = dict(diffuse=dict(mode=mode, radiance_hitdist=sig["diffuse"][0], direction=sig["diffuse"][1]), specular=dict(mode=mode, radiance_hitdist=sig["specular"][0],
                      direction=sig["specular"][1]), hit_dist_params=HDP, lib=be.lib)
            probe = frontend.describe_pack(dev["nr"], dev["viewz"], **kw)[0]
            out, bigs = {}, {}
            for rt, (t, fmt) in probe.items():
                view, bigs[rt] = be.padded(tuple(t.shape), frontend._dtype_name(t), fr.pad, STAMP)
                out[rt] = (view, fmt)
            res, desc, keep = frontend.describe_pack(dev["nr"], dev["viewz"], out=out, **kw)
            opt, smp = api.HipFrontEndOptions(int(cb_mode), frame_index), samples_struct(sig["diffuse"], sig["specular"])
            assert RC(be.lib.nrdHipPackInputsSamples(C.byref(desc), C.byref(opt), C.byref(smp), None)) == RC.SUCCESS, be.lib.nrdHipGetLastFrontEndError()
            for rt, (t, fmt) in res.items():
                got, big = be.down(t).copy(), be.down(bigs[rt])
                what = "%s frame %d %s %s" % (cb_mode.name, frame_index, mode.name, rt.name)
                if not rt.name.startswith(("IN_DIFF", "IN_SPEC")):
                    assert_bits(got, want[rt], what + " == the call without checkerboarding")
                    continue
                cell = cells["diffuse" if rt.name.startswith("IN_DIFF") else "specular"]
                moved = scene.checkerboard_pack(torch.from_numpy(want[rt]), cell, frame_index).numpy()
                b = cell ^ (yy[:, :1] & 1) ^ (frame_index & 1)
                k = np.arange(w)[None, :]
                written = (k < (w + 1) // 2) & (2 * k + b < w)
                assert_bits(got[written], moved[written], what)
                assert np.isfinite(got[written].astype(f32)).all(), what
                want_big = np.full(big.shape, STAMP, dtype=big.dtype)
                want_big[:h, :w][written] = got[written]
                assert np.array_equal(big.view(np.uint8), want_big.view(np.uint8)), what + ": a byte without a source pixel was written"


# ---------------------------------------------------------------------------------------------------------------------------------------------- 8. validation
def test_samples_validation_rules_return_their_codes_without_a_device():
    """every new rule of the header comment on the real library with no GPU present: INVALID_ARGUMENT and a text that names the field"""
    lib = api.load_library()
    keep = []
    h, w = 32, 64
    layer = w * h * 16

    def pack(mutate_samples, mutate_desc=lambda d: None):
        d = TPR._front_desc(keep, w, h)
        s = api.HipFrontEndSamples()
        s.specular.samplesNum, s.specular.radianceHitDistLayerBytes, s.specular.directionLayerBytes = 2, layer, layer
        mutate_desc(d)
        mutate_samples(s)
        code = RC(lib.nrdHipPackInputsSamples(C.byref(d), None, C.byref(s), None))
        return code, lib.nrdHipGetLastFrontEndError().decode()

    def expect(result, *words):
        assert result[0] == RC.INVALID_ARGUMENT and all(word in result[1] for word in words), result

    def sh(d):
        d.specular.mode = int(S.REBLUR_SH)
        d.specular.direction = d.specular.radianceHitDist
        d.specular.out1 = d.specular.out0

    expect(pack(lambda s: setattr(s.specular, "samplesNum", 65)), "specular.samplesNum")
    expect(pack(lambda s: setattr(s.diffuse, "samplesNum", 0xFFFFFFFF)), "diffuse.samplesNum")
    expect(pack(lambda s: setattr(s.specular, "reserved", 1)), "specular.reserved")
    expect(pack(lambda s: setattr(s.diffuse, "reserved", 7)), "diffuse.reserved")
    expect(pack(lambda s: setattr(s, "reserved", 1)), "samples: reserved")
    expect(pack(lambda s: setattr(s, "hitDistTrimThreshold", -0.5)), "hitDistTrimThreshold")
    expect(pack(lambda s: setattr(s, "hitDistTrimThreshold", float("nan"))), "hitDistTrimThreshold")
    expect(pack(lambda s: setattr(s.specular, "radianceHitDistLayerBytes", layer + 8)), "specular.radianceHitDistLayerBytes", "16")
    expect(pack(lambda s: setattr(s.specular, "radianceHitDistLayerBytes", layer - 16)), "specular.radianceHitDistLayerBytes", "rowPitchBytes")
    expect(pack(lambda s: setattr(s.specular, "radianceHitDistLayerBytes", 0)), "specular.radianceHitDistLayerBytes")
    expect(pack(lambda s: setattr(s.specular, "directionLayerBytes", layer - 16), sh), "specular.directionLayerBytes", "rowPitchBytes")
    expect(pack(lambda s: setattr(s.specular, "directionLayerBytes", layer + 4), sh), "specular.directionLayerBytes", "16")
    expect(pack(lambda s: setattr(s.diffuse, "samplesNum", 2)), "diffuse.samplesNum", "NONE")  # the descriptor has no diffuse signal
    # the rules of the plain call hold as before, and the strides of a plane the mode does not read, or of a single layer, are not looked at
    expect(pack(lambda s: None, lambda d: setattr(d.viewZ, "data", None)), "viewZ")
    assert RC(lib.nrdHipPackInputsSamples(None, None, None, None)) == RC.INVALID_ARGUMENT
    # (a valid descriptor gets past the validation: without a device the launch itself fails, or with one it succeeds -- never INVALID_ARGUMENT)
    assert pack(lambda s: setattr(s.specular, "directionLayerBytes", 5))[0] != RC.INVALID_ARGUMENT
    assert pack(lambda s: (setattr(s.specular, "samplesNum", 1), setattr(s.specular, "radianceHitDistLayerBytes", 3), setattr(s, "hitDistTrimThreshold", 0.5)))[0] != RC.INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------------------------- 9. surface
class RecordingLib:
    """a library that notes which entry points are called"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nrdHipPack"):
            return fn

        def wrapper(*args):
            self.calls.append(name)
            return fn(*args)
        return wrapper


def test_symbol_header_and_integration_class():
    lib = api.load_library()
    assert "nrdHipPackInputsSamples" in api.NRD_HIP_SYMBOLS and lib.nrdHipPackInputsSamples
    hdr = open(os.path.join(ROOT, "include", "NRDHip.h")).read()
    assert "uint32_t nrdHipPackInputsSamples(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, void* hipStream);" in hdr
    assert "const NrdHipFrontEndSamples& samples" in open(os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")).read()
    assert (C.sizeof(api.HipSignalSamples), C.sizeof(api.HipFrontEndSamples)) == (24, 56)
    s = frontend.pack_samples(dict(radiance_hitdist=np.zeros((3, 4, 8, 4), f32)), dict(radiance_hitdist=(np.zeros((5, 4, 8, 3), f32), np.zeros((5, 4, 8), f32))), 0.25)
    assert (s.diffuse.samplesNum, s.diffuse.radianceHitDistLayerBytes, s.specular.samplesNum, s.specular.radianceHitDistLayerBytes, s.hitDistTrimThreshold) == (3, 512, 5, 512, 0.25)


@pytest.mark.parametrize("backend", BACKENDS)
def test_python_surface_takes_the_new_call_for_layers_only(backend, dump):
    """frontend.pack_inputs with a 4-D signal (also as a ( [N, H, W, 3], [N, H, W] ) pair, and padded) gives the planes of the direct C-ABI call; a 3-D signal makes exactly the call
    it made before -- nrdHipPackInputsSamples is not called -- and hit_dist_trim alone takes the new one"""
    be = Backend(backend)
    w, h, n = W0, H0, 3
    fr = Frame(be, dump, w, h)
    rad, dirn = sample_layers(dump, w, h, n)
    layers = fr.up((rad, dirn))
    lib = RecordingLib(be.lib)
    dev = fr.dev
    for mode in (S.REBLUR_RADIANCE, S.RELAX_SH):
        want, _ = fr.call(mode, mode, diff=layers, spec=layers, trim=0.75)
        sig = lambda a, b: dict(mode=mode, radiance_hitdist=a, direction=b)
        lib.calls.clear()
        got = frontend.pack_inputs(dev["nr"], dev["viewz"], diffuse=sig(*layers), specular=sig(*layers), hit_dist_params=HDP, hit_dist_trim=0.75, lib=lib)
        assert lib.calls == ["nrdHipPackInputsSamples"]
        pair = (be.up(rad[..., :3]), be.up(rad[..., 3]))
        got_pair = frontend.pack_inputs(dev["nr"], dev["viewz"], diffuse=sig(pair, be.up(dirn[..., :3])), specular=sig(pair, be.up(dirn[..., :3])), hit_dist_params=HDP, hit_dist_trim=0.75, lib=lib)
        for rt in want:
            assert_bits(be.down(got[rt][0]), want[rt], "frontend.pack_inputs (4-D, padded) vs the C-ABI: %s %s" % (mode.name, rt.name))
            assert_bits(be.down(got_pair[rt][0]), want[rt], "frontend.pack_inputs (three-channel pair) vs the C-ABI: %s %s" % (mode.name, rt.name))
        # today's paths
        lib.calls.clear()
        single = sig(dev["rad"], dev["direction"])
        frontend.pack_inputs(dev["nr"], dev["viewz"], diffuse=single, specular=single, hit_dist_params=HDP, lib=lib)
        frontend.pack_inputs(dev["nr"], dev["viewz"], diffuse=single, specular=single, hit_dist_params=HDP, lib=lib, checkerboard_mode=CB.WHITE, frame_index=3)
        assert lib.calls == ["nrdHipPackInputs", "nrdHipPackInputsEx"]
        lib.calls.clear()
        trimmed = frontend.pack_inputs(dev["nr"], dev["viewz"], diffuse=single, specular=single, hit_dist_params=HDP, hit_dist_trim=0.75, lib=lib)
        assert lib.calls == ["nrdHipPackInputsSamples"]
        want1, _ = fr.call(mode, mode, trim=0.75)
        for rt in want1:
            assert_bits(be.down(trimmed[rt][0]), want1[rt], "frontend.pack_inputs (hit_dist_trim alone): %s" % rt.name)


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "pack_samples_integration.cpp")
CPP_EXE = os.path.join(ROOT, "tests", "cpp", "build", "pack_samples_integration")


def _build_cpp():
    """as tests/test_integration_cpp.py builds its program: g++, the installed headers, libNRD_hip.so"""
    lib = native_build.build_product()
    os.makedirs(os.path.dirname(CPP_EXE), exist_ok=True)
    hpp = os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")
    if os.path.exists(CPP_EXE) and os.path.getmtime(CPP_EXE) > max(os.path.getmtime(CPP_SRC), os.path.getmtime(lib), os.path.getmtime(hpp)):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-attributes", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", CPP_SRC, "-o", CPP_EXE,
           "-L" + os.path.dirname(lib), "-lNRD_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../../../raytracingdenoiser_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_cpp_overload_compiles_and_validates_on_the_host():
    _build_cpp()
    r = subprocess.run([CPP_EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host-only OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_overload_packs_sample_layers():
    _build_cpp()
    r = subprocess.run([CPP_EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "two equal layers vs one: 0 mismatching values" in r.stdout and "pack samples integration OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_captured_call_replays_the_same_bytes(dump):
    """the contract of the other calls: no allocation, no synchronisation -- the call is capturable by torch.cuda.graph (default queues, nothing else set) and replays the same bytes"""
    be = Backend("hip")
    w, h, n = W0, H0, 5
    fr = Frame(be, dump, w, h)
    layers = fr.up(sample_layers(dump, w, h, n))
    sig = dict(mode=S.REBLUR_SH, radiance_hitdist=layers[0], direction=layers[1])
    kw = dict(diffuse=sig, specular=sig, hit_dist_params=HDP)
    packed = frontend.pack_inputs(fr.dev["nr"], fr.dev["viewz"], **kw)
    torch.cuda.synchronize()
    eager = {rt: t.cpu().numpy().copy() for rt, (t, fmt) in packed.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frontend.pack_inputs(fr.dev["nr"], fr.dev["viewz"], out=packed, **kw)
    for t, fmt in packed.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for rt, (t, fmt) in packed.items():
        assert_bits(t.cpu().numpy(), eager[rt], "captured nrdHipPackInputsSamples == eager: %s" % rt.name)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 10. static facts
def test_static_facts_of_the_samples_kernel():
    """what the compiler made of the two instantiations of the multi-sample kernel for gfx950 (tools/frontend_bench.py samples_isa(), the `isa_samples` object of
    profiles/frontend_samples_bench.json): no scratch, no LDS, and the sample layers are read with 16-byte loads. VGPRs and waves per SIMD are printed and recorded, not bounded."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import frontend_bench

    facts = frontend_bench.samples_isa()
    assert set(facts) == {"pack_samples", "pack_samples_checkerboard"}
    for name, k in facts.items():
        print(name, k)
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0, (name, k)
        assert k["sample_loop_loads"] and set(k["sample_loop_loads"]) == {"global_load_dwordx4"}, (name, k)
        assert k["vgprs"] > 0 and k["waves_per_simd"] >= 1
