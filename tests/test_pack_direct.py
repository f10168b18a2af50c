"""nrdHipPackInputsDirect (include/NRDHip.h, raytracingdenoiser_amd/frontend.py): combined denoising of direct and indirect lighting -- the reference's README rule (radiance
summed, the specular hit distance the indirect one alone, the diffuse hit distance lerp( indirect, direct, min( Ld / ( Ld + Li + EPS ), maxContribution ) )) applied in the
pack launch.

As in tests/test_pack_samples.py / tests/test_pack_lobes.py every comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU),
outputs live in stamped, over-pitched allocations and every byte outside a rect is checked to still hold its stamp. Expected values never come from the code under test:
  B  packed fp32 values of single samples from tests/cpp/frontend_check --dump-host (the `dump` fixture): the indirect layers are the dump's columns rolled as in
     tests/test_pack_samples.py, the direct ones the same rolled by a prime number of rows more; the expectation is their float32 numpy sum, clamp and mean in the header's order
  M  tests/direct_model.py (float32, one numpy operation per fp32 operation of the header's text) for luminance, c and the mix; the normalised diffuse hit distance goes
     through tests/frontend_model.py
  P  the parent's calls, for the identities
Bounds: those of check_pack in tests/test_pack_resolve.py -- bit for bit wherever a value is + - * / of fp32 values, one code of the stored format on the normalised hit distance."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import direct_model as DM
import frontend_model as M
import test_pack_resolve as TPR
import test_pack_samples as TPS
from raytracingdenoiser_amd import api, frontend
from test_pack_resolve import BACKENDS, HDP, Backend, assert_bits, assert_codes, f16, img

dump = TPR.dump  # the host dump of tests/cpp/frontend_check (a module-scoped fixture)

ROOT = TPR.ROOT
F, R, S, CB, RC = api.Format, api.ResourceType, api.SignalMode, api.CheckerboardMode, api.Result
f32 = np.float32
COUNT = TPR.COUNT
W0, H0, W1, H1 = TPS.W0, TPS.H0, TPS.W1, TPS.H1  # 67 x 23 and 197 x 61: ragged in the last 64 x 4 workgroup column and row
STAMP, PAD, GAP = TPS.STAMP, 5, 3
SHIFT = TPS.SHIFT
DIRECT_SHIFT = 4099  # a prime: direct layer t holds the dump's samples rolled by t * SHIFT + DIRECT_SHIFT rows
MODES = [S.REBLUR_RADIANCE, S.REBLUR_SH, S.RELAX_RADIANCE, S.RELAX_SH]  # the modes with a radiance to weigh by
PAIRS = list(itertools.product(MODES, MODES))
SOME_PAIRS = [(S.REBLUR_RADIANCE, S.REBLUR_RADIANCE), (S.REBLUR_SH, S.RELAX_SH), (S.RELAX_SH, S.REBLUR_SH), (S.RELAX_RADIANCE, S.RELAX_RADIANCE)]  # every mode on either side once
# dump columns of the packed texels per mode: (first plane, second plane)
PACKED = {S.REBLUR_RADIANCE: ("reblurPacked", None), S.REBLUR_SH: ("sh0", "sh1"), S.RELAX_RADIANCE: ("relaxPacked", None), S.RELAX_SH: ("relaxPacked", "relaxSh1")}
_CACHE = {}


def needs_direction(mode):
    return mode in (S.REBLUR_SH, S.RELAX_SH)


def is_reblur(mode):
    return mode in (S.REBLUR_RADIANCE, S.REBLUR_SH)


# ---------------------------------------------------------------------------------------------------------------------------------------------- inputs
def shifted(d, name, rows):
    return np.roll(d[name], rows, axis=0)


def layers_of(d, w, h, n, extra=0):
    """([n, h, w, 4] radiance + hit distance, [n, h, w, 4] direction), read-only and computed once: layer s = the dump's input columns rolled by s * SHIFT + extra rows"""
    key = ("layers", w, h, n, extra)
    if key not in _CACHE:
        zeros = np.zeros((COUNT, 1), f32)
        rad = np.stack([img(d, shifted(d, "radiance", k * SHIFT + extra), shifted(d, "hitDist", k * SHIFT + extra), w=w, h=h) for k in range(n)])
        dirn = np.stack([img(d, shifted(d, "direction", k * SHIFT + extra), zeros, w=w, h=h) for k in range(n)])
        rad.setflags(write=False)
        dirn.setflags(write=False)
        _CACHE[key] = (rad, dirn)
    return _CACHE[key]


def packed_of(d, name, w, h, k, extra=0):
    """the dump's fp32 packed rows `name` of layer k, as an [h, w, C] image"""
    return img(d, shifted(d, name, k * SHIFT + extra), w=w, h=h)


def squeeze(a, n):
    return a[0] if n == 1 else a


def up_stack(be, a, fill=np.nan):
    """[H, W(, C)] or [N, H, W(, C)] on the backend inside a wider allocation: rows PAD texels longer than the plane, GAP rows between the layers, `fill` around the rects"""
    a = np.ascontiguousarray(a)
    plane_ndim = 3 if a.shape[-1] in (3, 4) and a.ndim >= 3 else 2
    if a.ndim == plane_ndim:
        return up_stack(be, a[None], fill)[0]
    big = np.full((a.shape[0], a.shape[1] + GAP, a.shape[2] + PAD) + a.shape[3:], fill, dtype=a.dtype)
    big[:, :a.shape[1], :a.shape[2]] = a
    big = big if be.name == "emu" else torch.from_numpy(big).cuda()
    return big[:, :a.shape[1], :a.shape[2]]


# ---------------------------------------------------------------------------------------------------------------------------------------------- running the kernels
class Call:
    """one frame layout on one backend: the G-buffer of tests/test_pack_resolve.py's pack tests (or planes given), and nrdHipPackInputsDirect / nrdHipPackInputsDecimated on it"""

    def __init__(self, be, d, w, h, viewz=None, guide_shift=0):
        self.be, self.w, self.h, self.guide_shift = be, w, h, guide_shift
        gw, gh = (w, h) if not guide_shift else (2 * w - 1, 2 * h - 1)  # ( ( W + 1 ) >> 1, ( H + 1 ) >> 1 ) = ( w, h ) with odd W, H
        ins = TPR.pack_inputs_of(d, gw, gh)
        if viewz is not None:
            ins["viewz"] = viewz
        self.ins = ins
        self.g = {k: be.up_pitched(ins[k], PAD) for k in ("nr", "viewz", "albedo", "material", "motion")}
        self.g["rf0"] = be.up_pitched(img(d, "Rf0", np.zeros((COUNT, 1), f32), w=gw, h=gh), PAD)
        self.cs = TPR.frame_settings(w, h)

    def decimated_copy(self):
        """the same frame with the G-buffer planes replaced by contiguous [ ::2, ::2 ] copies: what the call with guideShift = 0 is fed for the comparison"""
        other = Call.__new__(Call)
        other.be, other.w, other.h, other.guide_shift, other.cs = self.be, self.w, self.h, 0, self.cs
        other.ins = {k: np.ascontiguousarray(v[::2, ::2]) for k, v in self.ins.items()}
        host = dict(other.ins, rf0=np.ascontiguousarray(self.be.down(self.g["rf0"])[::2, ::2]))
        other.g = {k: self.be.up_pitched(host[k], PAD) for k in self.g}
        return other

    def __call__(self, dm, sm, diff, spec, direct=None, maxc=0.5, entry="direct", cb=CB.OFF, frame_index=0, trim=0.0, demodulate=False, full=False, in_place=False, mutate=None,
                 expect=RC.SUCCESS):
        """diff / spec: uploaded (radiance_hitdist, direction) of the INDIRECT signal -- arrays, stacks or (xyz, w) pairs with in_place; direct: None (a NULL pointer), or
        dict(diffuse=, specular=) of frontend.pack_direct's arguments (an empty dict: the zeroed struct). entry "decimated": nrdHipPackInputsDecimated, the parent's call.
        Returns ({ResourceType: plane}, {ResourceType: whole allocation}); with expect != SUCCESS the error text, after checking that every output still holds its stamp."""
        be, g, lib = self.be, self.g, self.be.lib
        sig = lambda mode, planes: dict(mode=mode, radiance_hitdist=planes[0], direction=planes[1] if needs_direction(mode) or mode == S.REBLUR_DIRECTIONAL_OCCLUSION else None)
        kw = dict(hit_dist_params=HDP, lib=lib, diffuse=sig(dm, diff), specular=sig(sm, spec), in_place=in_place, guide_shift=self.guide_shift)
        if full:
            kw.update(material_id=g["material"], motion=g["motion"])
        if demodulate:
            kw.update(albedo=g["albedo"], rf0=g["rf0"], common_settings=self.cs)
        probe = frontend.describe_pack(g["nr"], g["viewz"], **kw)[0]
        out, bigs = {}, {}
        for rt, (a, fmt) in probe.items():
            name = frontend._dtype_name(a)
            view, bigs[rt] = be.padded(tuple(a.shape), name, PAD, 0x5A if name == "uint8" else STAMP)
            out[rt] = (view, fmt)
        res, desc, keep = frontend.describe_pack(g["nr"], g["viewz"], out=out, **kw)
        split = frontend.pack_split(g["nr"], kw["diffuse"], kw["specular"]) if in_place else api.HipFrontEndSplit()
        samples = frontend.pack_samples(kw["diffuse"], kw["specular"], trim, in_place=in_place)
        options = api.HipFrontEndOptions(int(cb), frame_index)
        di = None if direct is None else frontend.pack_direct(direct.get("diffuse"), direct.get("specular"), maxc)[0]
        if mutate:
            mutate(desc, di)
        if entry == "direct":
            code = lib.nrdHipPackInputsDirect(C.byref(desc), C.byref(options), C.byref(samples), C.byref(split), None if di is None else C.byref(di), self.guide_shift, None)
        else:
            code = lib.nrdHipPackInputsDecimated(C.byref(desc), C.byref(options), C.byref(samples), C.byref(split), self.guide_shift, None)
        text = lib.nrdHipGetLastFrontEndError().decode()
        assert RC(code) == expect, (RC(code).name, text)
        got = {rt: be.down(a).copy() for rt, (a, fmt) in res.items()}
        whole = {rt: be.down(b).copy() for rt, b in bigs.items()}
        for rt, big in whole.items():  # (checkerboard calls leave texels inside the rect unwritten: compared by their tests)
            want = np.full(big.shape, 0x5A if big.dtype == np.uint8 else STAMP, dtype=big.dtype)
            if expect == RC.SUCCESS:
                want[:self.h, :self.w] = got[rt]
            assert np.array_equal(big.view(np.uint8), want.view(np.uint8)), "bytes outside the rect were written (or, on an error, any byte at all): %s" % rt.name
        return (got, whole) if expect == RC.SUCCESS else text


def uploaded(be, rad, dirn, n=None):
    """(radiance_hitdist, direction) of a signal on the backend, padded; n = 1 squeezes the stack to one plane"""
    n = rad.shape[0] if n is None and rad.ndim == 4 else n
    if rad.ndim == 4:
        rad, dirn = squeeze(rad, n), squeeze(dirn, n)
    return up_stack(be, rad), up_stack(be, dirn)


def direct_arg(planes, mode):
    return dict(radiance_hitdist=planes[0], direction=planes[1] if needs_direction(mode) else None)


def slots(which, mode):
    return frontend.signal_slots(which, mode, "IN")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1. modes and sample counts
def expected_colour(d, mode, w, h, n, one_direct_layer):
    """(first plane .xyz, second plane or None) of a signal in `mode`: B, summed, clamped and averaged in the header's order"""
    out = []
    for name, channels in zip(PACKED[mode], (slice(0, 3), slice(None))):
        if name is None:
            out.append(None)
            continue
        pi = [packed_of(d, name, w, h, k)[..., channels] for k in range(n)]
        if one_direct_layer:
            out.append(DM.combine_one_direct_layer(pi, packed_of(d, name, w, h, 0, DIRECT_SHIFT)[..., channels]))
        else:
            out.append(DM.combine_per_sample(pi, [packed_of(d, name, w, h, k, DIRECT_SHIFT)[..., channels] for k in range(n)]))
    return out


def mixed_hit_dists(rad_i, rad_d, maxc):
    """per sample: NRD_HIP_MixDiffuseHitDist of the model on ( h_i, h_d, L_i, L_d ); rad_d: [n, ..] or one layer [1, ..] under every sample"""
    n = rad_i.shape[0]
    out = []
    for s in range(n):
        t = s if rad_d.shape[0] == n else 0
        li, ld = DM.luminance(DM.san(rad_i[s][..., :3])), DM.luminance(DM.san(rad_d[t][..., :3]))
        out.append(DM.mix_diffuse_hit_dist(rad_i[s][..., 3], rad_d[t][..., 3], li, ld, maxc))
    return out


def check_diffuse_hit_dist(got, mode, hits, viewz, what):
    """the hit-distance channel of the diffuse signal against M: RELAX bit for bit (the clamp and the mean are fp32 + - * /), REBLUR within one code (the normalisation: C)"""
    if is_reblur(mode):
        # (a NaN hit distance leaves saturate() of the normalisation as 0 -- HLSL's and fminf / fmaxf's NaN rule -- an infinite one as 1: the model's np.clip keeps a NaN, so it is fed 0)
        nhd = [M.reblur_get_norm_hit_dist(np.where(np.isnan(h), 0.0, h.astype(np.float64)).reshape(-1), viewz.astype(np.float64).reshape(-1), HDP, 1.0).reshape(h.shape) for h in hits]
        assert_codes(got, f16(sum(nhd) / len(nhd)), what + " vs M through C")
    else:
        assert_bits(got, f16(DM.mean_of([DM.relax_packed_hit_dist(h) for h in hits])), what + " vs M")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", [(W0, H0), (W1, H1)])
def test_every_mode_pair_and_sample_count_against_the_host_dump(backend, size, dump):
    """67 x 23: every pair of radiance / SH modes; 197 x 61: every mode once on either side. N = 1, 2 and 5 (one batch of four and a remainder), with N direct layers and with one
    direct layer. Colour channels vs B bit for bit; the specular hit distance is the parent call's on the indirect planes, bit for bit; the diffuse one vs M"""
    be = Backend(backend)
    w, h = size
    call = Call(be, dump, w, h)
    viewz = call.ins["viewz"]
    for n in (1, 2, 5):
        rad_i, dir_i = layers_of(dump, w, h, n)
        rad_d, dir_d = layers_of(dump, w, h, n, DIRECT_SHIFT)
        indirect = uploaded(be, rad_i, dir_i)
        parent = {}
        for one_layer in ((False, True) if n > 1 else (True,)):
            dn = 1 if one_layer else n
            direct = uploaded(be, rad_d[:dn], dir_d[:dn], dn)
            hits = mixed_hit_dists(rad_i, rad_d[:dn], 0.5)
            colour = {mode: expected_colour(dump, mode, w, h, n, one_layer) for mode in MODES}
            for dm, sm in (PAIRS if size == (W0, H0) else SOME_PAIRS):
                what = "N = %d, %s, %s / %s" % (n, "one direct layer" if one_layer else "N direct layers", dm.name, sm.name)
                got, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(direct, dm), specular=direct_arg(direct, sm)))
                for which, mode in (("diffuse", dm), ("specular", sm)):
                    s0, s1 = slots(which, mode)
                    assert_bits(got[s0][..., :3], f16(colour[mode][0]), "%s: %s .xyz vs B" % (what, s0.name))
                    if s1 is not None:
                        assert_bits(got[s1], f16(colour[mode][1]), "%s: %s vs B" % (what, s1.name))
                if sm not in parent:
                    parent[sm] = call(S.RELAX_RADIANCE, sm, indirect, indirect, entry="decimated")[0][slots("specular", sm)[0]][..., 3]
                assert_bits(got[slots("specular", sm)[0]][..., 3], parent[sm], what + ": the specular hit distance is the call's without `direct`")
                check_diffuse_hit_dist(got[slots("diffuse", dm)[0]][..., 3], dm, hits, viewz, what + ": the diffuse hit distance")
                for a in got.values():
                    assert np.isfinite(a.astype(f32)).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2. identities
@pytest.mark.parametrize("backend", BACKENDS)
def test_null_and_zeroed_struct_are_the_decimated_call(backend, dump):
    """direct == NULL and the zeroed struct against nrdHipPackInputsDecimated, every output allocation byte for byte: plain, checkerboarded, demodulating, with sample layers and a
    trim threshold, three-channel planes in place, guideShift = 1"""
    be = Backend(backend)
    w, h = W0, H0
    call, low = Call(be, dump, w, h), Call(be, dump, w, h, guide_shift=1)
    rad, dirn = layers_of(dump, w, h, 3)
    one, three = uploaded(be, rad[:1], dirn[:1], 1), uploaded(be, rad, dirn)
    pair = ((up_stack(be, rad[0][..., :3]), up_stack(be, rad[0][..., 3])), up_stack(be, dirn[0][..., :3]))
    cases = [("plain", call, one, dict(full=True)), ("checkerboarded", call, one, dict(cb=CB.BLACK, frame_index=1)), ("demodulating", call, one, dict(demodulate=True)),
             ("three layers, trimmed", call, three, dict(trim=0.75)), ("three-channel planes in place", call, pair, dict(in_place=True)), ("guideShift = 1", low, one, dict(demodulate=True))]
    for what, c, planes, kw in cases:
        for dm, sm in SOME_PAIRS[:2]:
            _, want = c(dm, sm, planes, planes, entry="decimated", **kw)
            for name, direct in (("NULL", None), ("zeroed struct", {})):
                _, got = c(dm, sm, planes, planes, direct=direct, maxc=0.0, **kw)
                TPS.assert_same_planes(got, want, "nrdHipPackInputsDirect(%s) vs nrdHipPackInputsDecimated, %s, %s / %s" % (name, what, dm.name, sm.name))


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_direct_term_of_zero_radiance_is_the_call_without_it(backend, dump):
    """P_d of a zero radiance is zeros and c is 0: where the model says that adding it changes no bit -- the indirect packed value is not -0, which + 0 turns into +0 -- every
    output byte equals the call without `direct`; N = 1 and 3, one direct layer and N, a signal with a direct plane next to one without"""
    be = Backend(backend)
    w, h = W0, H0
    call = Call(be, dump, w, h)
    for n in (1, 3):
        rad, dirn = layers_of(dump, w, h, n)
        planes = uploaded(be, rad, dirn)
        for dn in sorted({1, n}):
            zero_rad = np.zeros((dn, h, w, 4), f32)
            zero_rad[..., 3] = 7.0  # a valid direct hit distance: c = 0 keeps it out
            zero = uploaded(be, zero_rad, np.asarray(layers_of(dump, w, h, dn, DIRECT_SHIFT)[1]), dn)
            for dm, sm in SOME_PAIRS:
                for name in (PACKED[dm][0], PACKED[sm][0]):  # the model: -0 + 0 is the one sum with a zero that changes a bit, and the first planes hold no -0
                    assert not any((np.signbit(packed_of(dump, name, w, h, k)) & (packed_of(dump, name, w, h, k) == 0))[..., :3].any() for k in range(n))
                _, want = call(dm, sm, planes, planes, entry="decimated", demodulate=True)
                for direct in (dict(diffuse=direct_arg(zero, dm), specular=direct_arg(zero, sm)), dict(diffuse=direct_arg(zero, dm)), dict(specular=direct_arg(zero, sm))):
                    _, got = call(dm, sm, planes, planes, direct=direct, demodulate=True)
                    for rt in want:  # (SH1 = direction x luminance may hold -0 where a direction component is -0 / the luminance 0: compared as values there)
                        if rt in (R.IN_DIFF_SH1, R.IN_SPEC_SH1):
                            assert np.array_equal(got[rt].astype(f32), want[rt].astype(f32)), rt.name
                        else:
                            assert_bits(got[rt], want[rt], "zero direct radiance (%s), N = %d, %d direct layer(s), %s / %s: %s" % ("+".join(sorted(direct)), n, dn, dm.name, sm.name, rt.name))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. the diffuse mix
def mix_scene(d, w, h, n):
    """indirect [n, h, w, 4] and direct [1, h, w, 4] planes whose first rows hold the branches of NRD_HIP_MixDiffuseHitDist at known pixels; the rest is the dump's"""
    rad_i, rad_d = np.array(layers_of(d, w, h, n)[0]), np.array(layers_of(d, w, h, 1, DIRECT_SHIFT)[0])
    rad_d[0, 0, 0:8, :3] = 0.0                      # L_d = 0
    rad_d[0, 0, 8:12, :3] = np.nan                  # no light sampled: NaN radiance
    rad_d[0, 0, 12:16, :3] = 50.0                   # a bright light: c above every cap below 1
    rad_i[:, 0, 12:16, :3] = 0.125
    rad_d[0, 0, 16:20, :3] = 0.001                  # a dim one: c below every cap above 0
    rad_i[:, 1, 0:8, 3] = 0.0                       # h_i = 0 with a valid h_d: stays 0
    rad_d[0, 1, 0:8, 3] = 3.0
    rad_d[0, 1, 8:12, 3] = np.nan                   # h_d NaN / 0 / inf / negative
    rad_d[0, 1, 12:16, 3] = 0.0
    rad_d[0, 1, 16:20, 3] = np.inf
    rad_d[0, 1, 20:24, 3] = -2.0
    rad_i[0, 1, 24:28, 3] = np.nan                  # an invalid h_i is kept out of the mix (and sanitised by the packer)
    rad_i[0, 1, 28:32, 3] = np.inf
    return rad_i, rad_d


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("maxc", [0.0, 0.5, 0.65, 1.0])
def test_diffuse_hit_distance_mix_on_every_branch(backend, maxc, dump):
    """N = 1 and 2 under one direct layer, RELAX_RADIANCE (bit for bit) and REBLUR_RADIANCE (one code): c capped by maxHitDistContribution, c below it, L_d = 0, h_i = 0 with a
    valid h_d (stays 0), h_d NaN / 0 / inf; the generator asserts that each branch occurs"""
    be = Backend(backend)
    w, h = W0, H0
    call = Call(be, dump, w, h)
    for n in (1, 2):
        rad_i, rad_d = mix_scene(dump, w, h, n)
        dirn = layers_of(dump, w, h, n)[1]
        li, ld = DM.luminance(DM.san(rad_i[0][..., :3])), DM.luminance(DM.san(rad_d[0][..., :3]))
        raw = ld / ((ld + li) + DM.NRD_EPS)
        c = DM.weight(li, ld, maxc)
        mixed = DM.is_mixed(rad_i[0][..., 3], rad_d[0][..., 3], c)
        hits = mixed_hit_dists(rad_i, rad_d, maxc)
        # every branch occurs
        assert (ld == 0).sum() >= 12 and (c[ld == 0] == 0).all() and not mixed[ld == 0].any()
        assert (rad_i[0][1, 0:8, 3] == 0).all() and (hits[0][1, 0:8] == 0).all() and np.isfinite(rad_d[0][1, 0:8, 3]).all()
        assert not mixed[1, 8:24].any() and (hits[0][1, 8:24] == rad_i[0][1, 8:24, 3]).all() and not mixed[1, 24:32].any()
        if maxc > 0:
            assert ((raw > maxc) & mixed).sum() >= (4 if maxc < 1 else 0) and (c[raw > maxc] == f32(maxc)).all(), "c capped by maxHitDistContribution"
            assert ((raw < maxc) & (raw > 0) & mixed).sum() > 100, "c below the cap"
            assert (hits[0][mixed] != rad_i[0][..., 3][mixed]).mean() > 0.9
        else:
            assert not mixed.any() and all(np.array_equal(hits[s], rad_i[s][..., 3], equal_nan=True) for s in range(n))
        indirect, direct = uploaded(be, rad_i, dirn), uploaded(be, rad_d, np.asarray(layers_of(dump, w, h, 1, DIRECT_SHIFT)[1]), 1)
        for mode in (S.RELAX_RADIANCE, S.REBLUR_RADIANCE):
            got, _ = call(mode, mode, indirect, indirect, direct=dict(diffuse=direct_arg(direct, mode), specular=direct_arg(direct, mode)), maxc=maxc)
            channel = got[slots("diffuse", mode)[0]][..., 3]
            check_diffuse_hit_dist(channel, mode, hits, call.ins["viewz"], "maxHitDistContribution = %g, N = %d, %s: the diffuse hit distance" % (maxc, n, mode.name))
            if n == 1:
                assert (channel.view(np.uint16)[1, 0:8] == 0).all(), "an indirect hit distance of 0 stays 0 under a valid direct one"
            parent, _ = call(mode, mode, indirect, indirect, entry="decimated")
            assert_bits(got[slots("specular", mode)[0]][..., 3], parent[slots("specular", mode)[0]][..., 3], "the specular hit distance is the indirect one")
            if maxc == 0:
                assert_bits(channel, parent[slots("diffuse", mode)[0]][..., 3], "maxHitDistContribution = 0: the diffuse hit distance stays the indirect one")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. poison
@pytest.mark.parametrize("backend", BACKENDS)
def test_values_the_rules_do_not_read_never_reach_an_output(backend, dump):
    """every output byte unchanged when: the specular direct .w is all NaN; the diffuse direct .w is NaN with maxHitDistContribution = 0; the direct planes are NaN at the pixels
    the checkerboard does not select for the signal; the direct planes are NaN where viewZ is sky, with the call demodulating (against zeros there)"""
    be = Backend(backend)
    w, h, n = W0, H0, 2
    rad_i, dir_i = layers_of(dump, w, h, n)
    rad_d, dir_d = layers_of(dump, w, h, n, DIRECT_SHIFT)
    indirect, clean = uploaded(be, rad_i, dir_i), uploaded(be, rad_d, dir_d)
    w_nan = np.array(rad_d)
    w_nan[..., 3] = np.nan
    w_nan = uploaded(be, w_nan, dir_d)
    call = Call(be, dump, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    for dm, sm in SOME_PAIRS:
        want, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(clean, dm), specular=direct_arg(clean, sm)))
        got, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(clean, dm), specular=direct_arg(w_nan, sm)))
        TPS.assert_same_planes(got, want, "the specular direct .w all NaN, %s / %s" % (dm.name, sm.name))
        want, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(clean, dm), specular=direct_arg(clean, sm)), maxc=0.0)
        got, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(w_nan, dm), specular=direct_arg(w_nan, sm)), maxc=0.0)
        TPS.assert_same_planes(got, want, "the diffuse direct .w NaN with maxHitDistContribution = 0, %s / %s" % (dm.name, sm.name))
        for cb, frame_index in ((CB.BLACK, 0), (CB.WHITE, 1), (CB.BLACK, 1)):
            diff_cell = 0 if cb == CB.BLACK else 1
            diff_here = (((xx ^ yy) ^ frame_index) & 1) == diff_cell
            poisoned = []
            for here in (diff_here, ~diff_here):  # the diffuse direct planes are NaN at the specular pixels, the specular ones at the diffuse pixels
                r, dd = np.array(rad_d), np.array(dir_d)
                r[:, ~here], dd[:, ~here] = np.nan, np.nan
                poisoned.append(uploaded(be, r, dd))
            want, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(clean, dm), specular=direct_arg(clean, sm)), cb=cb, frame_index=frame_index)
            got, _ = call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(poisoned[0], dm), specular=direct_arg(poisoned[1], sm)), cb=cb, frame_index=frame_index)
            TPS.assert_same_planes(got, want, "NaN at the pixels %s / frame %d does not select, %s / %s" % (cb.name, frame_index, dm.name, sm.name))
            for rt in got:
                if rt not in (R.IN_NORMAL_ROUGHNESS, R.IN_VIEWZ):
                    stamp = np.full((), STAMP, got[rt].dtype)
                    assert (got[rt][:, : (w + 1) // 2] != stamp).any() and (got[rt][:, (w + 1) // 2:] == stamp).all(), "the left half alone is written: %s" % rt.name
    # sky
    viewz = np.array(TPR.pack_inputs_of(dump, w, h)["viewz"])
    sky = ((xx * 7 + yy * 3) % 11) == 0
    viewz[sky] = 1e7
    sky_call = Call(be, dump, w, h, viewz=viewz)
    r_nan, d_nan, r_zero, d_zero = np.array(rad_d), np.array(dir_d), np.array(rad_d), np.array(dir_d)
    r_nan[:, sky], d_nan[:, sky], r_zero[:, sky], d_zero[:, sky] = np.nan, np.nan, 0.0, 0.0
    nan_planes, zero_planes = uploaded(be, r_nan, d_nan), uploaded(be, r_zero, d_zero)
    for dm, sm in SOME_PAIRS:
        want, _ = sky_call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(zero_planes, dm), specular=direct_arg(zero_planes, sm)), demodulate=True)
        got, _ = sky_call(dm, sm, indirect, indirect, direct=dict(diffuse=direct_arg(nan_planes, dm), specular=direct_arg(nan_planes, sm)), demodulate=True)
        TPS.assert_same_planes(got, want, "NaN direct texels on the sky, demodulating, %s / %s" % (dm.name, sm.name))
        for rt, a in got.items():
            if a.dtype == np.float16:
                assert np.isfinite(a.astype(f32)).all(), rt.name


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. overflow
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_radiances_of_60000_store_65504_not_infinity(backend, dump):
    be = Backend(backend)
    w, h = W0, H0
    call = Call(be, dump, w, h)
    for n in (1, 2):
        for dn in sorted({1, n}):
            rad_i, rad_d = np.full((n, h, w, 4), 60000.0, f32), np.full((dn, h, w, 4), 60000.0, f32)
            rad_i[..., 3], rad_d[..., 3] = 2.0, 3.0
            indirect, direct = uploaded(be, rad_i, layers_of(dump, w, h, n)[1]), uploaded(be, rad_d, layers_of(dump, w, h, dn)[1], dn)
            for mode in MODES:
                got, _ = call(mode, mode, indirect, indirect, direct=dict(diffuse=direct_arg(direct, mode), specular=direct_arg(direct, mode)))
                for which in ("diffuse", "specular"):
                    for rt in slots(which, mode):
                        if rt is not None:
                            assert np.isfinite(got[rt].astype(f32)).all(), (mode.name, rt.name)
                    first = got[slots(which, mode)[0]].astype(f32)
                    if is_reblur(mode):  # Y of ( 60000, 60000, 60000 ) is 60000; Co and Cg are 0
                        assert (first[..., 0] == 65504.0).all() and (first[..., 1:3] == 0).all(), mode.name
                    else:
                        assert (first[..., :3] == 65504.0).all(), mode.name


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. split planes, decimation
@pytest.mark.parametrize("backend", BACKENDS)
def test_three_channel_direct_planes_and_decimated_guides(backend, dump):
    """RGB32_SFLOAT direct planes with the diffuse hitDist companion (maxHitDistContribution > 0) and without it (= 0; the specular signal never has one) against their
    RGBA32_SFLOAT equivalents, byte for byte, N = 1 and 2, the indirect planes four-channel and three-channel in place; guideShift = 1 against the call fed decimated G-buffer copies"""
    be = Backend(backend)
    w, h = W0, H0
    call = Call(be, dump, w, h)
    for n in (1, 2):
        rad_i, dir_i = (squeeze(a, n) for a in layers_of(dump, w, h, n))
        rad_d, dir_d = (squeeze(a, n) for a in layers_of(dump, w, h, n, DIRECT_SHIFT))
        indirect, direct4 = (up_stack(be, rad_i), up_stack(be, dir_i)), (up_stack(be, rad_d), up_stack(be, dir_d))
        indirect3 = ((up_stack(be, rad_i[..., :3]), up_stack(be, rad_i[..., 3])), up_stack(be, dir_i[..., :3]))
        rgb, hit, dir3 = up_stack(be, rad_d[..., :3]), up_stack(be, rad_d[..., 3]), up_stack(be, dir_d[..., :3])
        for dm, sm in SOME_PAIRS:
            four = dict(diffuse=direct_arg(direct4, dm), specular=direct_arg(direct4, sm))
            for maxc in (0.5, 0.0):
                three = dict(diffuse=direct_arg(((rgb, hit) if maxc > 0 else rgb, dir3), dm), specular=direct_arg((rgb, dir3), sm))
                _, want = call(dm, sm, indirect, indirect, direct=four, maxc=maxc)
                _, got = call(dm, sm, indirect, indirect, direct=three, maxc=maxc)
                TPS.assert_same_planes(got, want, "RGB32_SFLOAT direct planes vs RGBA32_SFLOAT, N = %d, maxHitDistContribution = %g, %s / %s" % (n, maxc, dm.name, sm.name))
                _, got = call(dm, sm, indirect3, indirect3, direct=three, maxc=maxc, in_place=True)
                TPS.assert_same_planes(got, want, "... and the indirect planes three-channel in place, N = %d, maxHitDistContribution = %g, %s / %s" % (n, maxc, dm.name, sm.name))
        low = Call(be, dump, w, h, guide_shift=1)
        flat = low.decimated_copy()
        for dm, sm in SOME_PAIRS[:2]:
            four = dict(diffuse=direct_arg(direct4, dm), specular=direct_arg(direct4, sm))
            _, got = low(dm, sm, indirect, indirect, direct=four, demodulate=True, full=True)
            _, want = flat(dm, sm, indirect, indirect, direct=four, demodulate=True, full=True)
            TPS.assert_same_planes(got, want, "guideShift = 1 vs decimated G-buffer copies, N = %d, %s / %s" % (n, dm.name, sm.name))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7. errors
@pytest.mark.parametrize("backend", BACKENDS)
def test_error_table(backend, dump):
    """one case per sentence of the header: the code, the field named in the text, nothing enqueued (every output allocation still holds its stamp)"""
    be = Backend(backend)
    w, h, n = W0, H0, 2
    call = Call(be, dump, w, h)
    rad_i, dir_i = layers_of(dump, w, h, n)
    rad_d, dir_d = layers_of(dump, w, h, n, DIRECT_SHIFT)
    indirect, direct4 = uploaded(be, rad_i, dir_i), uploaded(be, rad_d, dir_d)
    rgb, hit, dir3 = up_stack(be, rad_d[..., :3]), up_stack(be, rad_d[..., 3]), up_stack(be, dir_d[..., :3])
    z = frontend._fp32_plane(call.g["viewz"], 1, "x")
    INV, UNS = RC.INVALID_ARGUMENT, RC.UNSUPPORTED

    def case(expect, field, mutate, dm=S.REBLUR_SH, sm=S.REBLUR_RADIANCE, direct="four", maxc=0.5, planes=indirect, **kw):
        if direct == "four":
            direct = dict(diffuse=direct_arg(direct4, S.REBLUR_SH), specular=direct_arg(direct4, S.REBLUR_RADIANCE))
        text = call(dm, sm, planes, planes, direct=direct, maxc=maxc, mutate=mutate, expect=expect, **kw)
        assert text.startswith("nrdHipPackInputsDirect: ") and field in text, (field, text)

    # a direct plane for a signal without a radiance to weigh by
    case(INV, "direct: diffuse.radianceHitDist", None, dm=S.REBLUR_OCCLUSION, direct=dict(diffuse=dict(radiance_hitdist=direct4[0])))
    case(INV, "direct: diffuse.radianceHitDist", None, dm=S.REBLUR_DIRECTIONAL_OCCLUSION, direct=dict(diffuse=dict(radiance_hitdist=direct4[0], direction=direct4[1])))
    case(INV, "direct: specular.radianceHitDist", None, sm=S.REBLUR_OCCLUSION, direct=dict(specular=dict(radiance_hitdist=direct4[0])))
    one, one_direct = uploaded(be, rad_i[:1], dir_i[:1], 1), uploaded(be, rad_d[:1], dir_d[:1], 1)
    case(INV, "direct: specular.radianceHitDist", lambda d, di: (setattr(d.specular, "mode", 0), setattr(d.specular.out0, "data", None), setattr(d.specular.radianceHitDist, "data", None)),
         planes=one, direct=dict(diffuse=direct_arg(one_direct, S.REBLUR_SH), specular=direct_arg(one_direct, S.REBLUR_RADIANCE)))  # NONE
    # the direction
    case(INV, "direct: diffuse.direction", lambda d, di: setattr(di.diffuse.direction, "data", None))  # REBLUR_SH reads one
    case(INV, "direct: specular.direction", lambda d, di: setattr(di.specular, "direction", di.diffuse.direction))  # REBLUR_RADIANCE reads none
    # the hit-distance companions
    case(INV, "direct: specular.hitDist", lambda d, di: setattr(di.specular, "hitDist", z))
    case(INV, "direct: diffuse.hitDist", lambda d, di: setattr(di.diffuse, "hitDist", z))  # next to an RGBA32_SFLOAT plane: .w would have two sources
    three = dict(diffuse=dict(radiance_hitdist=(rgb, hit), direction=dir3), specular=dict(radiance_hitdist=rgb))
    case(INV, "direct: diffuse.hitDist", lambda d, di: setattr(di.diffuse.hitDist, "data", None), direct=three)  # RGB32_SFLOAT, maxHitDistContribution > 0: missing
    case(INV, "direct: diffuse.hitDist", None, direct=three, maxc=0.0)  # given with maxHitDistContribution == 0
    # the struct
    for bad in (float("nan"), -0.25, 1.5):
        case(INV, "maxHitDistContribution", None, maxc=bad)
    case(INV, "direct: diffuse.samplesNum", lambda d, di: setattr(di.diffuse, "samplesNum", 3))
    case(INV, "direct: specular.samplesNum", lambda d, di: setattr(di.specular, "samplesNum", 64))
    case(INV, "direct: reserved", lambda d, di: setattr(di, "reserved", 1))
    case(INV, "direct: diffuse.reserved", lambda d, di: setattr(di.diffuse, "reserved", 1))
    case(INV, "direct: specular.reserved", lambda d, di: setattr(di.specular, "reserved", 7))
    # layer strides, N = 2: a multiple of 16 for RGBA32_SFLOAT, of 4 for the others, and not below the plane
    case(INV, "direct: diffuse.radianceHitDistLayerBytes", lambda d, di: setattr(di.diffuse, "radianceHitDistLayerBytes", di.diffuse.radianceHitDistLayerBytes + 8))
    case(INV, "direct: specular.radianceHitDistLayerBytes", lambda d, di: setattr(di.specular, "radianceHitDistLayerBytes", 16))
    case(INV, "direct: diffuse.directionLayerBytes", lambda d, di: setattr(di.diffuse, "directionLayerBytes", 16 * (w + PAD) * (h - 1)))  # one row short of the plane
    case(INV, "direct: diffuse.hitDistLayerBytes", lambda d, di: setattr(di.diffuse, "hitDistLayerBytes", di.diffuse.hitDistLayerBytes + 2), direct=three)
    case(INV, "direct: diffuse.radianceHitDistLayerBytes", lambda d, di: setattr(di.diffuse, "radianceHitDistLayerBytes", di.diffuse.radianceHitDistLayerBytes + 2), direct=three)
    # size, pitch, alignment, the 32-bit limits, formats
    case(INV, "direct: diffuse.radianceHitDist", lambda d, di: setattr(di.diffuse.radianceHitDist, "width", w - 1))
    case(INV, "direct: specular.radianceHitDist", lambda d, di: setattr(di.specular.radianceHitDist, "rowPitchBytes", di.specular.radianceHitDist.rowPitchBytes + 4))
    case(INV, "direct: diffuse.direction", lambda d, di: setattr(di.diffuse.direction, "data", di.diffuse.direction.data + 4))
    case(UNS, "direct: diffuse.radianceHitDist", lambda d, di: setattr(di.diffuse.radianceHitDist, "rowPitchBytes", 1 << 24))
    case(UNS, "direct: diffuse.radianceHitDist", lambda d, di: setattr(di.diffuse.radianceHitDist, "format", int(F.RGBA16_SFLOAT)))
    case(UNS, "direct: specular.radianceHitDist", lambda d, di: setattr(di.specular.radianceHitDist, "format", int(F.RG32_SFLOAT)))
    case(UNS, "direct: diffuse.direction", lambda d, di: setattr(di.diffuse.direction, "format", int(F.R32_SFLOAT)))
    case(UNS, "direct: diffuse.hitDist", lambda d, di: setattr(di.diffuse.hitDist, "format", int(F.R16_SFLOAT)), direct=three)
    # the low size under guideShift = 1: a full-size direct plane is refused
    low = Call(be, dump, w, h, guide_shift=1)
    full_size = up_stack(be, np.zeros((2 * h - 1, 2 * w - 1, 4), f32))
    text = low(S.REBLUR_RADIANCE, S.REBLUR_RADIANCE, indirect, indirect, direct=dict(diffuse=dict(radiance_hitdist=full_size)), expect=INV)
    assert "direct: diffuse.radianceHitDist" in text
    text = call(S.REBLUR_RADIANCE, S.REBLUR_RADIANCE, indirect, indirect, direct={}, mutate=lambda d, di: setattr(di.diffuse, "direction", z), expect=INV)
    assert "direct: diffuse.direction" in text  # a direction without a radiance plane
    call(S.REBLUR_SH, S.REBLUR_RADIANCE, indirect, indirect, direct=dict(diffuse=direct_arg(direct4, S.REBLUR_SH), specular=direct_arg(direct4, S.REBLUR_RADIANCE)))  # and the unmutated call succeeds


# ---------------------------------------------------------------------------------------------------------------------------------------------- 8. surface
def test_symbols_structs_and_python_surface():
    """the entry point is exported by the product library and declared by the header, the two structs are mirrored with their sizes, the wrappers are there"""
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "NRDHip.h")).read()
    assert "nrdHipPackInputsDirect" in api.NRD_HIP_SYMBOLS and lib.nrdHipPackInputsDirect and "uint32_t nrdHipPackInputsDirect(" in hdr
    assert "static_assert(sizeof(NrdHipDirectSignal) == 104 && sizeof(NrdHipFrontEndDirect) == 216" in hdr
    assert C.sizeof(api.HipDirectSignal) == 104 and C.sizeof(api.HipFrontEndDirect) == 216
    assert "#define NRD_HIP_DIRECT_MAX_CONTRIBUTION_DEFAULT 0.5f" in hdr and api.DIRECT_MAX_CONTRIBUTION_DEFAULT == 0.5
    assert "NRD_HIP_MixDiffuseHitDist" in open(os.path.join(ROOT, "include", "NRD.hip.h")).read()
    assert "PackInputsDirect" in open(os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")).read()
    assert callable(frontend.pack_direct) and "direct" in frontend.pack_inputs.__kwdefaults__ and "direct" in frontend.describe_pack.__code__.co_varnames
    di, keep = frontend.pack_direct(dict(radiance_hitdist=(np.zeros((3, 4, 8, 3), f32), np.zeros((3, 4, 8), f32)), direction=np.zeros((3, 4, 8, 4), f32)), np.zeros((4, 8, 4), f32), 0.65)
    assert (di.diffuse.samplesNum, di.diffuse.radianceHitDistLayerBytes, di.diffuse.hitDistLayerBytes, di.diffuse.directionLayerBytes) == (3, 384, 128, 512)
    assert (di.diffuse.radianceHitDist.format, di.diffuse.hitDist.format, di.diffuse.direction.format) == (int(F.RGB32_SFLOAT), int(F.R32_SFLOAT), int(F.RGBA32_SFLOAT))
    assert (di.specular.samplesNum, di.specular.radianceHitDist.format, di.specular.hitDist.data, abs(di.maxHitDistContribution - 0.65) < 1e-7) == (1, int(F.RGBA32_SFLOAT), None, True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_pack_inputs_routes_direct(backend, dump):
    """frontend.pack_inputs(direct=...) is the C-ABI call: the same bytes as Call, with a dict and with what pack_direct returned, plain and with guide_shift = 1"""
    be = Backend(backend)
    w, h, n = W0, H0, 2
    rad_i, dir_i = layers_of(dump, w, h, n)
    rad_d, dir_d = layers_of(dump, w, h, 1, DIRECT_SHIFT)
    indirect, direct = uploaded(be, rad_i, dir_i), uploaded(be, rad_d, dir_d, 1)
    for call in (Call(be, dump, w, h), Call(be, dump, w, h, guide_shift=1)):
        arg = dict(diffuse=direct_arg(direct, S.REBLUR_SH), specular=direct[0], max_hit_dist_contribution=0.65)
        want, _ = call(S.REBLUR_SH, S.RELAX_RADIANCE, indirect, indirect, direct=dict(diffuse=arg["diffuse"], specular=dict(radiance_hitdist=direct[0])), maxc=0.65)
        for given in (arg, frontend.pack_direct(**arg)):
            packed = frontend.pack_inputs(call.g["nr"], call.g["viewz"], diffuse=dict(mode=S.REBLUR_SH, radiance_hitdist=indirect[0], direction=indirect[1]),
                                          specular=dict(mode=S.RELAX_RADIANCE, radiance_hitdist=indirect[0]), hit_dist_params=HDP, lib=be.lib, guide_shift=call.guide_shift, direct=given)
            TPS.assert_same_planes({rt: be.down(a) for rt, (a, fmt) in packed.items()}, want, "frontend.pack_inputs(direct=...), guide_shift = %d" % call.guide_shift)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 9. GPU only
@pytest.mark.gpu
def test_captured_call_replays_the_same_bytes(dump):
    """the contract of the other calls: no allocation, no synchronisation -- the call is capturable by torch.cuda.graph (default queues, nothing else set) and replays the same bytes"""
    be = Backend("hip")
    w, h, n = W0, H0, 5
    call = Call(be, dump, w, h)
    rad_i, dir_i = layers_of(dump, w, h, n)
    rad_d, dir_d = layers_of(dump, w, h, n, DIRECT_SHIFT)
    indirect, direct = uploaded(be, rad_i, dir_i), uploaded(be, rad_d, dir_d)
    sig = dict(mode=S.REBLUR_SH, radiance_hitdist=indirect[0], direction=indirect[1])
    kw = dict(diffuse=sig, specular=sig, hit_dist_params=HDP, direct=frontend.pack_direct(direct_arg(direct, S.REBLUR_SH), direct_arg(direct, S.REBLUR_SH)))
    packed = frontend.pack_inputs(call.g["nr"], call.g["viewz"], **kw)
    torch.cuda.synchronize()
    eager = {rt: t.cpu().numpy().copy() for rt, (t, fmt) in packed.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frontend.pack_inputs(call.g["nr"], call.g["viewz"], out=packed, **kw)
    for t, fmt in packed.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for rt, (t, fmt) in packed.items():
        assert_bits(t.cpu().numpy(), eager[rt], "captured nrdHipPackInputsDirect == eager: %s" % rt.name)


@pytest.mark.gpu
def test_fused_packed_planes_meet_the_input_rules(dump):
    """a frame whose direct texels are NaN on the sky, packed by the fused call and bound to a REBLUR_DIFFUSE_SPECULAR executor at 67 x 23: check_inputs() reports no rule broken"""
    import parity
    from raytracingdenoiser_amd.executor import HipExecutor

    be = Backend("hip")
    w, h = W0, H0
    yy, xx = np.mgrid[0:h, 0:w]
    sky = ((xx * 7 + yy * 3) % 11) == 0
    viewz = np.array(TPR.pack_inputs_of(dump, w, h)["viewz"])
    viewz[sky] = 1e7  # beyond the default denoising range
    call = Call(be, dump, w, h, viewz=viewz)
    rad_i, dir_i = layers_of(dump, w, h, 1)
    rad_d, dir_d = (np.array(a) for a in layers_of(dump, w, h, 1, DIRECT_SHIFT))
    rad_d[:, sky], dir_d[:, sky] = np.nan, np.nan
    indirect, direct = uploaded(be, rad_i, dir_i, 1), uploaded(be, rad_d, dir_d, 1)
    motion = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    sig = lambda planes: dict(mode=S.REBLUR_RADIANCE, radiance_hitdist=planes[0])
    packed = frontend.pack_inputs(call.g["nr"], call.g["viewz"], motion=motion, diffuse=sig(indirect), specular=sig(indirect), albedo=call.g["albedo"], rf0=call.g["rf0"],
                                  common_settings=call.cs, hit_dist_params=HDP, direct=dict(diffuse=direct[0], specular=direct[0]))
    torch.cuda.synchronize()
    for rt, (t, fmt) in packed.items():
        if t.dtype == torch.float16:
            assert bool(torch.isfinite(t.float()).all()), rt.name
    name = "REBLUR_DIFFUSE_SPECULAR"
    inst = api.Instance([(0, parity.DENOISERS[name][0])])
    ex = HipExecutor(inst, w, h)
    try:
        outs = {rt: torch.zeros((h, w, ch), dtype=dtype, device="cuda") for rt, dtype, ch, fmt in parity.output_planes(name, w, h)}
        for (rt, dtype, ch, fmt) in parity.output_planes(name, w, h):
            ex.bind(rt, outs[rt], fmt)
        ex.bind_packed({rt: (t.contiguous(), fmt) for rt, (t, fmt) in packed.items()})
        assert inst.set_common_settings(call.cs) == api.Result.SUCCESS
        report = ex.check_inputs()
        assert report, report.rules
    finally:
        ex.destroy()
