"""NRD's input rules for sky and off-rect texels (tests/input_rules.py quotes them): a host may leave garbage, NaN / INF included, in the NOISY inputs wherever viewZ is beyond
the denoising range and wherever the texel is outside the rect, and its guides are finite but not clean on the sky. What this file holds, on the device (the GPU; the CPU
emulation of the device sources with NRD_PARITY_BACKEND=emu):
  a. garbage beyond the denoising range: device == oracle bit for bit, and -- the property no oracle is needed for -- every output texel inside the range equals, bit for bit,
     the run with the renderer's clean sky and is finite;
  b. garbage outside the rect of a larger resource: the same two, and output texels outside the rect keep what was there;
  c. arbitrary finite guides on the sky: device == oracle (no invariance is claimed: the reference's own text lets a sky texel's normal and roughness decide whether a tap of a
     neighbouring geometry texel counts -- tests/test_ref_parity_input_rules.py holds the oracle to that text on the same input);
  d. a sky made by viewZ alone, on texels that keep a geometry normal and a signal, still and moving: device == oracle;
  e. the two tap variants of the REBLUR spatial passes ("full rect" and generic, NRD_HIP_GENERIC_TAPS=1) against each other, byte for byte, in fresh child processes."""
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import input_rules
import parity
from oracle import driver as oracle_driver
from raytracingdenoiser_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = api.ResourceType

# one denoiser per signal family and kernel set
FAMILIES = ["REBLUR_DIFFUSE_SPECULAR", "REBLUR_DIFFUSE_SPECULAR_SH", "REBLUR_DIFFUSE_SPECULAR_OCCLUSION", "REBLUR_DIFFUSE_DIRECTIONAL_OCCLUSION", "RELAX_DIFFUSE_SPECULAR",
            "RELAX_DIFFUSE_SPECULAR_SH", "SIGMA_SHADOW", "SIGMA_SHADOW_TRANSLUCENCY"]
MAIN = ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR_SH", "SIGMA_SHADOW"]
# (rect, resource, frames): 256x160 -- the horizon cuts 16x16 tiles and 32x8 workgroups; 67x45 -- odd, partial tiles; 176x104 inside a 256x160 resource
BIG, ODD, RECT = ((256, 160), None, 4), ((67, 45), None, 3), ((176, 104), (256, 160), 3)
SIZE_OF_KIND = {"finite": ODD, "nan": BIG, "mixed": RECT, "inf": ODD, "neg_inf": BIG}


@pytest.fixture(autouse=True)
def _wall_time(request):
    t = time.perf_counter()
    yield
    print("[wall time] %s: %.2f s" % (request.node.name, time.perf_counter() - t))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fill_outside(plane, w, h, value):
    plane[h:, :] = value
    plane[:h, w:] = value


_clean = {}  # device outputs of the unshaped sequences, computed once per (denoiser, size, settings) and shared by the cases


def device_frames(name, seq, rect, resource=None, overrides=None, cs_kw=None, rect_sizes=None, key=None):
    """the device alone over `seq`: per frame {output: float32 texel values} and, from frame 1 on, whether every output texel outside that frame's rect kept what it held before
    the frame. After frame 0 (the restart frame clears the outputs) the outside of the rect is filled with 5, so that "kept" cannot mean "zero again"."""
    if key is not None and key in _clean:
        return _clean[key]
    rw, rh = resource or rect
    hip = parity.HipRun(name, rw, rh)
    cs_kw = dict(cs_kw or {})
    if resource:
        cs_kw.update(resourceSize=resource, resourceSizePrev=resource)
    outs, kept = [], []
    for f, frame in enumerate(seq):
        w, h = rect_sizes[f % len(rect_sizes)] if rect_sizes else rect
        if rect_sizes:
            cs_kw.update(rectSize=(w, h), rectSizePrev=rect_sizes[max(f - 1, 0) % len(rect_sizes)])
        before = {rt: hip.output(rt).copy() for rt in hip.outs}
        parity.tag_checkerboard(frame, overrides, f)
        hip.step(frame, parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], w, h, f, **cs_kw), parity.denoiser_settings(name, frame, overrides))
        now = {rt: hip.output(rt).copy() for rt in hip.outs}
        if f > 0:
            kept.append(all(np.array_equal(_bits(now[rt][h:]), _bits(before[rt][h:])) and np.array_equal(_bits(now[rt][:h, w:]), _bits(before[rt][:h, w:])) for rt in now))
        else:
            for rt in hip.outs:
                _fill_outside(hip.outs[rt][0], w, h, 5)
        outs.append(now)
    if key is not None:
        _clean[key] = (outs, kept)
    return outs, kept


def _sequence(name, rect, frames, extra_want=(), rect_sizes=None):
    want = tuple(parity.DENOISERS[name][1]) + tuple(extra_want)
    if rect_sizes:
        return [parity.synth.render_frame(*rect_sizes[f % len(rect_sizes)], f, want=want) for f in range(frames)]
    return [parity.synth.render_frame(rect[0], rect[1], f, want=want) for f in range(frames)]  # = scene.generate_sequence (parity.generate_sequence may be patched by the case)


def _assert_invariant(name, dirty, clean, seq, rect, rect_sizes=None, whole_rect=False):
    """every output texel inside the rect and inside the denoising range (whole_rect: every texel of the rect) is bit-identical in the two runs; none inside the range is NaN / INF"""
    for f, (d, c) in enumerate(zip(dirty, clean)):
        w, h = rect_sizes[f % len(rect_sizes)] if rect_sizes else rect
        inside = ~input_rules.sky_mask(seq[f]).numpy()[:h, :w]
        for rt in d:
            a, b = d[rt][:h, :w], c[rt][:h, :w]
            same = np.all(_bits(a) == _bits(b), axis=-1)
            must = np.ones_like(inside) if whole_rect else inside
            bad = np.argwhere(must & ~same)
            print("%s frame %d %s: %d of %d texels differ from the clean run, %d non-finite inside the range" % (name, f, rt.name, len(bad), int(must.sum()), int((~np.isfinite(a).all(-1) & inside).sum())))
            assert not len(bad), (name, f, rt.name, len(bad), bad[:3].tolist())
            assert np.isfinite(a[inside]).all(), (name, f, rt.name)


# ---- a. garbage beyond the denoising range -------------------------------------------------------------------------------------------------------------------------
def _garbage_case(monkeypatch, name, kind, size, overrides=None, extra_want=()):
    rect, resource, frames = size
    input_rules.shaped(monkeypatch, lambda n, frame, f: input_rules.dirty_sky_noisy(frame, kind, f, n))
    worst = parity.run_parity(name, width=rect[0], height=rect[1], frames=frames, resource=resource, settings_overrides=overrides, extra_want=extra_want)
    print("%s %s %s: worst relative error %g" % (name, kind, rect, worst))
    assert worst == 0.0, (name, kind, worst)

    seq = _sequence(name, rect, frames, extra_want)
    embed = (lambda s: [input_rules.embed_in_resource(fr, resource) for fr in s]) if resource else (lambda s: s)
    key = (name, size, repr(overrides), tuple(extra_want))
    clean, _ = device_frames(name, embed([dict(fr) for fr in seq]), rect, resource, overrides, key=key)
    for f, frame in enumerate(seq):
        input_rules.dirty_sky_noisy(frame, kind, f, name)
    seq = embed(seq)
    dirty, _ = device_frames(name, seq, rect, resource, overrides)
    _assert_invariant(name, dirty, clean, seq, rect)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["finite", "nan", "mixed"])
@pytest.mark.parametrize("name", FAMILIES)
def test_garbage_in_the_noisy_inputs_beyond_the_denoising_range_changes_nothing_inside_it(monkeypatch, name, kind):
    _garbage_case(monkeypatch, name, kind, SIZE_OF_KIND[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["inf", "neg_inf"])
@pytest.mark.parametrize("name", ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR"])
def test_infinities_in_the_noisy_inputs_beyond_the_denoising_range_change_nothing_inside_it(monkeypatch, name, kind):
    _garbage_case(monkeypatch, name, kind, SIZE_OF_KIND[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nan", "mixed"])
@pytest.mark.parametrize("overrides, extra_want", [
    (dict(checkerboardMode=1), ()),
    (dict(enableAntiFirefly=True), ()),
    (dict(hitDistanceReconstructionMode=1), ("holes",)),  # 3x3: its taps read the raw noisy neighbours, sky texels among them
    (dict(enablePerformanceMode=True), ()),
], ids=["checkerboard", "anti_firefly", "hit_distance_reconstruction_3x3", "performance_mode"])
def test_garbage_beyond_the_denoising_range_in_the_optional_reblur_passes(monkeypatch, overrides, extra_want, kind):
    _garbage_case(monkeypatch, "REBLUR_DIFFUSE_SPECULAR", kind, BIG, overrides, extra_want)


def _reference_executor(w, h):
    if os.environ.get("NRD_PARITY_BACKEND") == "emu":
        from emu import emu_run

        inst = api.Instance([(0, api.Denoiser.REFERENCE)], lib=emu_run.load())
        return inst, emu_run.EmuExecutor(inst, w, h), (lambda a: a), (lambda a: a)
    import torch

    from raytracingdenoiser_amd.executor import HipExecutor

    inst = api.Instance([(0, api.Denoiser.REFERENCE)])
    return inst, HipExecutor(inst, w, h), (lambda a: torch.from_numpy(a).cuda()), (lambda t: t.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["finite", "nan", "mixed"])
def test_garbage_in_the_signal_of_the_REFERENCE_accumulator_stays_in_its_texel(kind):
    """REFERENCE has no viewZ and no denoising range: it accumulates IN_SIGNAL texel by texel. Garbage on the texels that are sky in the synthetic frame: device == oracle (a NaN
    for a NaN), and every other texel equals the clean run bit for bit and is finite."""
    import torch

    w, h, frames = 67, 45, 3
    sky = input_rules.sky_mask(parity.synth.render_frame(w, h, 0, want=())).numpy()
    rng = np.random.default_rng(5)
    clean = [rng.random((h, w, 4), dtype=np.float32) + 0.25 for _ in range(frames)]
    dirty = []
    for f, sig in enumerate(clean):
        g = input_rules._garbage(torch.from_numpy(sig), kind, f).numpy()
        dirty.append(np.where(sky[..., None], g, sig).astype(np.float32))

    def settings(f):
        cs = api.CommonSettings(resourceSize=(w, h), rectSize=(w, h), resourceSizePrev=(w, h), rectSizePrev=(w, h), timeDeltaBetweenFrames=16.667, frameIndex=f)
        for m in (cs.viewToClipMatrix, cs.viewToClipMatrixPrev, cs.worldToViewMatrix, cs.worldToViewMatrixPrev):
            for k in (0, 5, 10, 15):
                m[k] = 1.0
        return cs

    def run(make, signals):
        inst, ex, to_dev, to_host = make()
        out = to_dev(np.full((h, w, 4), -7.0, dtype=np.float32))
        ex.bind(RT.OUT_SIGNAL, out, api.Format.RGBA32_SFLOAT)
        outs = []
        for f, sig in enumerate(signals):
            ex.bind(RT.IN_SIGNAL, to_dev(np.ascontiguousarray(sig)), api.Format.RGBA32_SFLOAT)
            assert inst.set_common_settings(settings(f)) == api.Result.SUCCESS
            if hasattr(ex, "denoise"):
                ex.denoise()
            else:
                r, ds = inst.get_compute_dispatches()
                assert r == api.Result.SUCCESS
                ex.execute(ds)
            outs.append(np.array(to_host(out), copy=True))
        return outs

    def oracle():
        inst = api.Instance([(0, api.Denoiser.REFERENCE)])
        return inst, oracle_driver.OracleExecutor(inst, w, h, api.FORMAT_BYTES), (lambda a: a), (lambda a: a)

    want, got, got_clean = run(oracle, dirty), run(lambda: _reference_executor(w, h), dirty), run(lambda: _reference_executor(w, h), clean)
    for f in range(frames):
        both_nan = np.isnan(want[f]) & np.isnan(got[f])
        assert np.all(both_nan | (_bits(want[f]) == _bits(got[f]))), "frame %d differs from the oracle" % f
        assert np.array_equal(_bits(got[f][~sky]), _bits(got_clean[f][~sky])) and np.isfinite(got[f][~sky]).all(), "frame %d" % f


# ---- b. garbage outside the rect -----------------------------------------------------------------------------------------------------------------------------------
def _off_rect_case(monkeypatch, name, kind, rect, resource, frames, rect_sizes=None):
    input_rules.shaped(monkeypatch, embed=lambda frame, res, f: input_rules.embed_in_resource_dirty(frame, res, kind, f))
    worst = parity.run_parity(name, width=rect[0], height=rect[1], frames=frames, resource=resource, rect_sizes=rect_sizes)
    print("%s %s %s in %s: worst relative error %g" % (name, kind, rect_sizes or rect, resource, worst))
    assert worst == 0.0, (name, kind, worst)

    seq = _sequence(name, rect, frames, rect_sizes=rect_sizes)
    key = (name, "off_rect", rect, resource, repr(rect_sizes), frames)
    clean, clean_kept = device_frames(name, [input_rules.embed_in_resource(fr, resource) for fr in seq], rect, resource, rect_sizes=rect_sizes, key=key)
    seq = [input_rules.embed_in_resource_dirty(fr, resource, kind, f) for f, fr in enumerate(seq)]
    dirty, kept = device_frames(name, seq, rect, resource, rect_sizes=rect_sizes)
    _assert_invariant(name, dirty, clean, seq, rect, rect_sizes, whole_rect=True)
    assert all(kept) and all(clean_kept), (name, "an output texel outside the rect was written", kept, clean_kept)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nan", "mixed"])
@pytest.mark.parametrize("name", FAMILIES)
def test_garbage_in_the_noisy_inputs_outside_the_rect_changes_nothing_inside_it_and_nothing_is_written_outside(monkeypatch, name, kind):
    _off_rect_case(monkeypatch, name, kind, (176, 104), (256, 160), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_a_rect_that_grows_and_shrinks_over_last_frames_garbage(monkeypatch, name):
    """the rect of frame f + 1 covers texels that were outside the rect, and garbage, on frame f -- inside this frame's history footprint"""
    _off_rect_case(monkeypatch, name, "nan", (176, 104), (256, 160), 4, rect_sizes=[(176, 104), (256, 160), (132, 78), (220, 130)])


# ---- c. arbitrary finite guides on the sky ----------------------------------------------------------------------------------------------------------------------
GUIDE_CASES = [(name, (), None) for name in MAIN] + [
    # the optional guides bound and enabled, screen-space motion vectors (world-space ones are scaled by 0 in the plain sequence: their texels would not matter)
    ("REBLUR_DIFFUSE_SPECULAR", ("mv2d", "confidence", "basecolor"),
     dict(isMotionVectorInWorldSpace=False, motionVectorScale=(1.0 / 256, 1.0 / 160, 1.0), isHistoryConfidenceAvailable=True, isDisocclusionThresholdMixAvailable=True, isBaseColorMetalnessAvailable=True)),
    ("RELAX_DIFFUSE_SPECULAR_SH", ("mv2d", "confidence"),
     dict(isMotionVectorInWorldSpace=False, motionVectorScale=(1.0 / 256, 1.0 / 160, 1.0), isHistoryConfidenceAvailable=True, isDisocclusionThresholdMixAvailable=True)),
    ("SIGMA_SHADOW", ("mv2d",), dict(isMotionVectorInWorldSpace=False, motionVectorScale=(1.0 / 256, 1.0 / 160, 1.0))),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name, extra_want, cs_kw", GUIDE_CASES, ids=["%s-%s" % (c[0], "optional_guides" if c[1] else "plain") for c in GUIDE_CASES])
def test_arbitrary_finite_guides_on_the_sky(monkeypatch, name, extra_want, cs_kw):
    input_rules.shaped(monkeypatch, lambda n, frame, f: input_rules.dirty_sky_guides(frame))
    worst = parity.run_parity(name, width=256, height=160, frames=4, extra_want=extra_want, cs_kw=cs_kw)
    print("%s: worst relative error %g" % (name, worst))
    assert worst == 0.0, (name, worst)


# ---- d. a sky made by viewZ alone ----------------------------------------------------------------------------------------------------------------------------------
PAINTED = [n for n in FAMILIES if n.startswith("REBLUR")] + ["RELAX_DIFFUSE_SPECULAR_SH", "SIGMA_SHADOW"]
NO_TS = dict(maxStabilizedFrameNum=0)  # REBLUR: the *_PostBlur_NoTemporalStabilization pass writes the history copies itself; SIGMA: no stabilization pass; RELAX has none


@pytest.mark.gpu
@pytest.mark.parametrize("moving", [False, True], ids=["still", "moving"])
@pytest.mark.parametrize("name, overrides", [(n, None) for n in PAINTED] + [(n, NO_TS) for n in PAINTED if not n.startswith("RELAX")],
                         ids=PAINTED + [n + "-no_temporal_stabilization" for n in PAINTED if not n.startswith("RELAX")])
def test_a_sky_painted_by_viewz_alone_over_geometry(monkeypatch, name, overrides, moving):
    input_rules.shaped(monkeypatch, lambda n, frame, f: input_rules.paint_sky(frame, f, moving))
    worst = parity.run_parity(name, width=256, height=160, frames=4, settings_overrides=overrides)
    print("%s %s: worst relative error %g" % (name, "moving" if moving else "still", worst))
    assert worst == 0.0, (name, moving, worst)


# ---- e. the two tap variants of the REBLUR spatial passes against each other ------------------------------------------------------------------------------------------
def run_tap_variant_case(name):
    """(runs in a child process of the test below: NRD_HIP_GENERIC_TAPS is read by the library from its environment) prints one digest per scene, frame and plane -- every
    output and every pool plane"""
    w, h, frames = 256, 160, 4
    for scene in ("default", "painted_moving"):
        seq = _sequence(name, (w, h), frames)
        if scene == "painted_moving":
            for f, frame in enumerate(seq):
                input_rules.paint_sky(frame, f, True)
        hip = parity.HipRun(name, w, h)
        for f, frame in enumerate(seq):
            hip.step(frame, parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], w, h, f), parity.denoiser_settings(name, frame, None))
            planes = [(rt.name, hip.output(rt)) for rt in hip.outs]
            for pool in (RT.PERMANENT_POOL, RT.TRANSIENT_POOL):
                for i in range(len(hip.inst.permanent_pool if pool == RT.PERMANENT_POOL else hip.inst.transient_pool)):
                    raw, fmt, pw = hip.ex.read_pool_plane(pool, i)
                    planes.append(("%s[%d]" % (pool.name, i), np.asarray(raw)[:, : pw * api.FORMAT_BYTES[fmt]]))
            for label, a in planes:
                print("digest %s frame %d %s %s" % (scene, f, label, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["REBLUR_DIFFUSE_SPECULAR", "REBLUR_DIFFUSE_SPECULAR_SH", "REBLUR_DIFFUSE_SPECULAR_OCCLUSION"])
def test_full_rect_taps_and_generic_taps_compute_the_same_bytes(name):
    """the "full rect" variant of the spatial passes' taps (kernels_reblur_spatial.hip FetchTapGuidesFullRect: one 16-byte guide load per tap) is an optimisation of the generic
    one, not another filter: all outputs and pool planes of 4 frames are byte-identical, on the default scene and under a moving painted sky (next to whole tiles of sky the
    post-blur's viewZ plane -- the copy the blur pass wrote -- keeps values of earlier frames, which the per-frame guide plane does not hold)"""
    code = "import sys; sys.path[:0] = [%r, %r]; import test_input_rules; test_input_rules.run_tap_variant_case(%r)" % (ROOT, os.path.join(ROOT, "tests"), name)
    env = {k: v for k, v in os.environ.items() if k != "NRD_HIP_GENERIC_TAPS"}
    procs = [subprocess.Popen([sys.executable, "-c", code], env=dict(env, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra in ({}, {"NRD_HIP_GENERIC_TAPS": "1"})]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    full, generic = ([line for line in out.splitlines() if line.startswith("digest ")] for out, _ in outs)
    assert len(full) == len(generic) and len(full) >= 2 * 4 * 10, (len(full), len(generic))
    differing = [a for a, b in zip(full, generic) if a != b]
    print("%s: %d planes compared, %d differ" % (name, len(full), len(differing)))
    assert not differing, [d.rsplit(" ", 1)[0] for d in differing[:8]]
