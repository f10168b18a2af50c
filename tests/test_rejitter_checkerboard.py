"""nrdHipResolveOutputsEx (NRD_SG_ReJitter between the resolve and the remodulation) and nrdHipPackInputsEx (checkerboarded noisy inputs): include/NRDHip.h,
raytracingdenoiser_amd/frontend.py.

As in tests/test_pack_resolve.py every comparison runs on "emu" (the device source compiled for the CPU, part of the CPU suite) and on "hip" (the GPU). Expected values never come
from library code:
  the re-jitter stencil is assembled HERE -- numpy gathers, per pixel, both SH pairs, Rf0, V (the float32 numpy restatement of the view-vector contract), Z and the packed
  IN_NORMAL_ROUGHNESS texel with those of the four edge neighbours (zeros outside the plane) -- and tests/cpp/rejitter_rows.hip evaluates NRD_SG_ReJitter of include/NRD.hip.h on
  these rows, on the host (the expectation of emu) or one thread per row on the device (the expectation of hip): bit for bit. Which pixels are left unscaled is held against
  tests/frontend_model.py (float64) and against causes the test derives itself from the margins of the constructed scene. The colours are float32 products of planes the parent's
  nrdHipResolveOutputs writes. The checkerboard expectation is the expectation of tests/test_pack_resolve.py moved by scene.checkerboard_pack (a torch gather)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frontend_model as M
import parity
import test_frontend_header as TFH
import test_pack_resolve as TPR
from oracle import driver as oracle_driver
from raytracingdenoiser_amd import api, frontend, scene, synth
from test_pack_resolve import Backend, assert_bits, assert_codes, camera_constants, frame_settings, view_vector_numpy

ROOT = TPR.ROOT
F, R, S, RES, CB = api.Format, api.ResourceType, api.SignalMode, api.ResolveMode, api.CheckerboardMode
f32 = np.float32
BACKENDS = TPR.BACKENDS
HDP = TPR.HDP
W0, H0 = 67, 23  # a full and a 3-pixel workgroup column, six rows of 64 x 4 workgroups (three columns, three rows for 32 x 8)
STAMP = 23130
ROWS_SRC = os.path.join(ROOT, "tests", "cpp", "rejitter_rows.hip")
ROWS_EXE = os.path.join(ROOT, "tests", "cpp", "build", "rejitter_rows" + api.ENCODING_SUFFIX)


def _build_rows():
    """tests/cpp/rejitter_rows.hip with the flags of test_frontend_header._build"""
    os.makedirs(os.path.dirname(ROWS_EXE), exist_ok=True)
    hdr = os.path.join(ROOT, "include", "NRD.hip.h")
    if os.path.exists(ROWS_EXE) and os.path.getmtime(ROWS_EXE) > max(os.path.getmtime(ROWS_SRC), os.path.getmtime(hdr)):
        return
    cmd = [TFH.HIPCC, "-std=c++17", "-O2", "-ffp-contract=off", "--offload-arch=gfx950", "-DNRD_NORMAL_ENCODING=%d" % api.NORMAL_ENCODING, "-DNRD_ROUGHNESS_ENCODING=%d" % api.ROUGHNESS_ENCODING,
           "-I" + os.path.join(ROOT, "include"), ROWS_SRC, "-o", ROWS_EXE]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------- the constructed scene
def hsh(a, b, s):
    v = np.sin(12.9898 * a + 78.233 * b + 37.719 * s) * 43758.5453
    return v - np.floor(v)


def _normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _neighbours(a):
    """(e, w, n, s) = the values at (x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1); zeros outside the plane"""
    h, w = a.shape[:2]
    p = np.zeros((h + 2, w + 2) + a.shape[2:], a.dtype)
    p[1:-1, 1:-1] = a
    return p[1:-1, 2:], p[1:-1, :-2], p[2:, 1:-1], p[:-2, 1:-1]


_scenes = {}


def make_scene(w, h):
    """the scene of the issue at size w x h (a crop is the same function of (x, y), with the camera of its own size): float32 planes as the kernels are fed them"""
    if (w, h) in _scenes:
        return _scenes[(w, h)]
    cs = frame_settings(w, h)
    frustum, rot = camera_constants(cs)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    hv = lambda s0: np.stack([hsh(x, y, s0), hsh(x, y, s0 + 1), hsh(x, y, s0 + 2)], -1)
    nv = np.stack([0.3 * np.sin(0.21 * x) + 0.3 * (hsh(x, y, 1) - 0.5), 0.3 * np.cos(0.17 * y) + 0.3 * (hsh(x, y, 2) - 0.5), -np.ones_like(x)], -1)
    band = (y >= 15) & (y <= 17)  # horizontal neighbours face away from each other
    odd = (x.astype(np.int64) & 1) == 1
    nv[band & odd] = (0.9, 0.0, -0.436)
    nv[band & ~odd] = (-0.9, 0.0, -0.436)
    n_world = _normalize(nv) @ rot.astype(np.float64).T  # view space -> world: the rotation of view-to-world
    rough = 0.05 + 0.95 * hsh(x, y, 3)
    z = (5.0 + 0.002 * x + 0.003 * y) * np.where((x >= 40) & (x < 50), 2.5, 1.0)  # a depth step
    sc = {"w": w, "h": h, "cs": cs, "frustum": frustum, "rot": rot}
    sc["viewz"] = z.astype(f32)
    sc["V"] = view_vector_numpy(frustum, rot, sc["viewz"])
    word = synth.pack_normal_roughness(torch.from_numpy(n_world.astype(f32)), torch.from_numpy(rough.astype(f32)), torch.zeros(h, w)).numpy()  # an input like any other
    sc["word"] = np.ascontiguousarray(word)
    for which, seed in (("diff", 10), ("spec", 20)):
        direction = _normalize(n_world + 0.8 * (hv(seed) - 0.5))
        sh0, sh1 = M.reblur_pack_sh(0.05 + 3.0 * hv(seed + 3), hsh(x, y, seed + 6), direction)
        sc[which + "_sh0"], sc[which + "_sh1"] = sh0.astype(f32), sh1.astype(f32)
    grey = 0.04 + 0.8 * hsh(x, y, 30)
    sc["rf0"] = np.stack([grey, grey, grey, np.zeros_like(grey)], -1).astype(f32)
    sc["albedo"] = np.concatenate([0.1 + 0.8 * hv(31), np.zeros((h, w, 1))], -1).astype(f32)
    _scenes[(w, h)] = sc
    return sc


def texel_words(word):
    """the IN_NORMAL_ROUGHNESS texels as uint64 [H, W] (a 32-bit texel zero-extended)"""
    if word.ndim == 2:
        return word.view(np.uint32).astype(np.uint64)
    return np.ascontiguousarray(word).view(np.uint64)[..., 0]


def stencil_rows(sc, sh):
    """one row of tests/cpp/rejitter_rows.hip per pixel, gathered from the planes; sh: the four SH planes as float32 (the values the kernel reads)"""
    h, w = sc["h"], sc["w"]
    z, words = sc["viewz"], texel_words(sc["word"])
    rows = np.zeros((h, w, 38), np.uint32)
    fl = rows.view(f32)
    for k, name in enumerate(("diff_sh0", "diff_sh1", "spec_sh0", "spec_sh1")):
        fl[..., 4 * k:4 * k + 4] = sh[name]
    fl[..., 16:19] = sc["rf0"][..., :3]
    fl[..., 19:22] = sc["V"]
    for k, a in enumerate((z,) + _neighbours(z)):
        fl[..., 22 + k] = a
    for k, a in enumerate((words,) + _neighbours(words)):
        rows[..., 28 + 2 * k] = (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        rows[..., 29 + 2 * k] = (a >> np.uint64(32)).astype(np.uint32)
    return rows.reshape(h * w, 38)


def header_scale(sc, sh, where):
    """NRD_SG_ReJitter of include/NRD.hip.h on the rows: where = "--host" or "--device"; float32 [H, W, 2]"""
    _build_rows()
    base = ROWS_EXE + ".%d" % os.getpid()
    stencil_rows(sc, sh).tofile(base + ".in")
    try:
        r = subprocess.run([ROWS_EXE, where, base + ".in", base + ".out"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "rejitter rows %d" % (sc["w"] * sc["h"]) in r.stdout, r.stdout + r.stderr
        print(r.stdout.strip())
        return np.fromfile(base + ".out", dtype=f32).reshape(sc["h"], sc["w"], 2)
    finally:
        for ext in (".in", ".out"):
            if os.path.exists(base + ext):
                os.remove(base + ext)


def model_decisions(sc, sh, check_counts):
    """which pixels tests/frontend_model.py (float64) leaves at exactly (1, 1), and the premise of the scene: no decision of NRD_SG_ReJitter sits near its threshold.
    The default G-buffer encoding only (the model decodes R10G10B10A2 words)."""
    assert (api.NORMAL_ENCODING, api.ROUGHNESS_ENCODING) == (2, 1)
    h, w = sc["h"], sc["w"]
    nr, _ = M.unpack_normal_and_roughness(M.load_r10g10b10a2(sc["word"].view(np.uint32)))
    zero_n = M.unpack_normal_and_roughness(M.load_r10g10b10a2(np.zeros((1, 1), np.uint32)))[0][0, 0, :3]  # what an all-zero texel decodes to
    N, rough, Z, V = nr[..., :3], nr[..., 3], sc["viewz"].astype(np.float64), sc["V"].astype(np.float64)
    inside = np.ones((h, w), bool)
    ins = _neighbours(inside)
    Zs = _neighbours(Z)
    Ns = [np.where(i[..., None], n, zero_n) for i, n in zip(ins, _neighbours(N))]
    sg = lambda which: M.unpack_sh(sh[which + "_sh0"].astype(np.float64), sh[which + "_sh1"].astype(np.float64))
    scale = M.sg_rejitter(sg("diff"), sg("spec"), sc["rf0"][..., :3].astype(np.float64), V, rough, Z, *Zs, N, *Ns)
    model_ones = np.all(scale == 1.0, axis=-1)
    # the premise, on neighbours inside the plane
    threshold = 0.01 * np.abs(Z) / (np.abs((N * V).sum(-1)) * 0.95 + 0.05)
    z_margin, n_margin = np.inf, np.inf
    z_fail, n_fail = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for i, zn, nn in zip(ins, Zs, Ns):
        dz, dot = np.abs(zn - Z), (nn * N).sum(-1)
        if i.any():
            z_margin = min(z_margin, (np.abs(dz - threshold) / threshold)[i].min())
            n_margin = min(n_margin, np.abs(dot)[i].min())
        z_fail |= i & ~(dz < threshold)
        n_fail |= i & ~(dot > 0.0)
    border = ~(ins[0] & ins[1] & ins[2] & ins[3])
    print("%d x %d: margins %.3g (viewZ, of the threshold) and %.3g (normals); %d of %d pixels scaled; diffuse factor %.3g .. %.3g (1st .. 99th percentile); specular factor on the "
          "1 / pi clamp at %d pixels, on the pi clamp at %d" % (w, h, z_margin, n_margin, int((~model_ones).sum()), w * h, np.percentile(scale[..., 0], 1), np.percentile(scale[..., 0], 99),
                                                                int((scale[..., 1] == 1.0 / M.NRD_PI).sum()), int((scale[..., 1] == M.NRD_PI).sum())))
    assert z_margin >= 0.5 and n_margin >= 0.05, (z_margin, n_margin)
    assert np.array_equal(model_ones, border | z_fail | n_fail), "the model leaves other pixels unscaled than the border, the depth step and the opposed normals"
    if check_counts:  # 67 x 23: the causes, computed from the margins above
        by_z, by_n = z_fail & ~border, n_fail & ~border & ~z_fail
        assert int(border.sum()) == 176 and int(model_ones.sum()) == 443 and int((~model_ones).sum()) == 1098
        assert sorted(set(np.nonzero(by_z)[1])) == [39, 40, 49, 50] and int(by_z.sum()) == 84  # the two sides of both edges of the depth step
        assert set(np.nonzero(by_n)[0]) <= set(range(14, 19)) and int(by_n.sum()) == 183  # the rows whose horizontal neighbours face away from each other
    return model_ones


# ---------------------------------------------------------------------------------------------------------------------------------------------- running the kernels
def sh_planes(sc, half):
    names = ("diff_sh0", "diff_sh1", "spec_sh0", "spec_sh1")
    fed = {n: (TPR.f16(sc[n]) if half else sc[n]) for n in names}
    return fed, {n: fed[n].astype(f32) for n in names}  # (what is uploaded, the float32 values the kernel reads)


class Planes:
    """the scene on a backend: every input plane inside a wider stamped allocation"""

    def __init__(self, be, sc, half=False, pad=5):
        self.be, self.sc, self.pad = be, sc, pad
        fed, self.values = sh_planes(sc, half)
        self.dev = {n: be.up_pitched(a, pad) for n, a in fed.items()}
        for n in ("viewz", "word", "rf0", "albedo"):
            self.dev[n] = be.up_pitched(sc[n], pad)

    def resolve(self, resolve, rejitter, remodulate=False, want=(), stamped=True, mode=S.REBLUR_SH):
        """(downloaded planes, downloaded whole allocations) of one call"""
        h, w, be, d = self.sc["h"], self.sc["w"], self.be, self.dev
        names = ["diffuse", "specular"] + [{"factors": "diff_factor"}.get(n, n) for n in want] + (["spec_factor"] if "factors" in want else [])
        out, bigs = {}, {}
        for n in names:
            out[n], bigs[n] = be.padded((h, w, 2 if n == "rejitter_scale" else 4), "float32", self.pad, STAMP)
        kw = dict(diffuse=dict(mode=mode, resolve=resolve, in0=d["diff_sh0"], in1=d["diff_sh1"]), specular=dict(mode=mode, resolve=resolve, in0=d["spec_sh0"], in1=d["spec_sh1"]),
                  normal_roughness=d["word"], viewz=d["viewz"], rf0=d["rf0"], common_settings=self.sc["cs"], hit_dist_params=HDP, lib=be.lib, want=want, out=out if stamped else None)
        if remodulate or "factors" in want:
            kw.update(albedo=d["albedo"], remodulate=remodulate)
        elif not rejitter:
            kw.pop("rf0")
        res = frontend.resolve_outputs(rejitter=rejitter, **kw)
        assert set(res) == set(names), (sorted(res), names)
        got = {n: be.down(t).copy() for n, t in res.items()}
        whole = {n: be.down(b) for n, b in bigs.items()}
        if stamped:
            for n, big in whole.items():
                want_big = np.full(big.shape, STAMP, dtype=f32)
                want_big[:h, :w] = got[n]
                assert np.array_equal(big.view(np.uint8), want_big.view(np.uint8)), "bytes outside the rect were written: %s" % n
        return got


def check_rejitter(backend, w, h, half=False, check_counts=False):
    """the assertions of the issue's tests 1 and 2 at one size"""
    be, sc = Backend(backend), make_scene(w, h)
    p = Planes(be, sc, half=half)
    want_scale = header_scale(sc, p.values, "--host" if backend == "emu" else "--device")
    model_ones = model_decisions(sc, p.values, check_counts)
    tag = "%d x %d%s" % (w, h, " fp16" if half else "")
    for resolve in (RES.SG, RES.SH):
        plain = p.resolve(resolve, rejitter=False)
        got = p.resolve(resolve, rejitter=True, want=("rejitter_scale",))
        scale = got["rejitter_scale"]
        assert_bits(scale, want_scale, "%s %s: rejitter_scale vs NRD.hip.h on the rows (%s)" % (tag, resolve.name, "host" if backend == "emu" else "device"))
        assert np.array_equal(np.all(scale == 1.0, axis=-1), model_ones), "%s: the pixels left at (1, 1) are not the model's" % tag
        for k, which in enumerate(("diffuse", "specular")):
            assert_bits(got[which][..., :3], plain[which][..., :3] * scale[..., k:k + 1], "%s %s: %s.rgb == plain.rgb * scale" % (tag, resolve.name, which))
            assert_bits(got[which][..., 3], plain[which][..., 3], "%s %s: %s.w" % (tag, resolve.name, which))
        if w == 1 and h == 1:
            for which in ("diffuse", "specular"):
                assert_bits(got[which], plain[which], "1 x 1: %s is the plain resolve" % which)
    # remodulation and composition: ( plain * scale ) * factor, in that order
    plain = p.resolve(RES.SG, rejitter=False)
    got = p.resolve(RES.SG, rejitter=True, remodulate=True, want=("rejitter_scale", "factors", "composed"))
    assert_bits(got["rejitter_scale"], want_scale, "%s remodulated: rejitter_scale" % tag)
    colours = []
    for k, (which, factor) in enumerate((("diffuse", "diff_factor"), ("specular", "spec_factor"))):
        colours.append((plain[which][..., :3] * got["rejitter_scale"][..., k:k + 1]) * got[factor][..., :3])
        assert colours[-1].dtype == f32
        assert_bits(got[which][..., :3], colours[-1], "%s remodulated: %s.rgb == ( plain.rgb * scale ) * factor" % (tag, which))
        assert_bits(got[which][..., 3], plain[which][..., 3], "%s remodulated: %s.w" % (tag, which))
    assert_bits(got["composed"][..., :3], colours[0] + colours[1], "%s composed == diffuse + specular" % tag)
    assert not got["composed"][..., 3].any()
    assert np.isfinite(got["diffuse"]).all() and np.isfinite(got["specular"]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1 / 2. re-jitter
@pytest.mark.parametrize("backend", BACKENDS)
def test_rejitter_constructed_scene_67x23(backend):
    """fp32 SH planes: the expectation has no fp16 rounding of its own. Checked on the CPU when the scene was designed (stand-in camera): margins 0.94 and 0.072; 1098 of 1541 pixels
    scaled, 443 exactly (1, 1) -- 176 on the border, 84 along the depth step (columns 39, 40, 49, 50), 183 in the rows of opposed normals."""
    check_rejitter(backend, W0, H0, check_counts=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejitter_constructed_scene_fp16_planes(backend):
    """the same with RGBA16_SFLOAT signal planes, the expectation built from the rounded values"""
    check_rejitter(backend, W0, H0, half=True, check_counts=True)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", [(1, 1), (64, 4), (65, 5)])
def test_rejitter_edges_of_the_tile(backend, size):
    """1 x 1 (the output is exactly the plain resolve), 64 x 4 (one workgroup, the whole halo outside the plane) and 65 x 5 (one texel of a second workgroup column and row)"""
    check_rejitter(backend, *size)


@pytest.mark.parametrize("backend", BACKENDS)
def test_relax_sh_rejitters_like_reblur_sh(backend):
    """RELAX_SH pairs go through the same unpack: same scale, bit for bit"""
    be, sc = Backend(backend), make_scene(W0, H0)
    p = Planes(be, sc)
    a = p.resolve(RES.SG, rejitter=True, want=("rejitter_scale",), mode=S.REBLUR_SH)
    b = p.resolve(RES.SG, rejitter=True, want=("rejitter_scale",), mode=S.RELAX_SH)
    assert_bits(b["rejitter_scale"], a["rejitter_scale"], "RELAX_SH vs REBLUR_SH scale")
    assert_bits(b["diffuse"], a["diffuse"], "RELAX_SH vs REBLUR_SH diffuse")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3. validation, NULL options
def test_ex_validation_rules_return_their_codes_without_a_device():
    lib = api.load_library()
    RC = api.Result
    for name in ("nrdHipPackInputsEx", "nrdHipResolveOutputsEx"):
        assert name in api.NRD_HIP_SYMBOLS and getattr(lib, name)
    hpp = open(os.path.join(ROOT, "include", "NRDIntegrationHip.hpp")).read()
    assert "const NrdHipFrontEndOptions& options" in hpp and "const NrdHipBackEndOptions& options" in hpp
    w, h = 64, 32
    sh, out, word, z, rf0 = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), np.zeros((h, w), np.int32), np.ones((h, w), f32), np.zeros((h, w, 4), f32)
    if api.NORMAL_ENCODING > 2:
        word = np.zeros((h, w, 4), np.int16)
    scale = np.zeros((h, w, 2), f32)
    persp = parity.common_settings(synth.Camera(w, h, 0), synth.Camera(w, h, 0), w, h, 0)
    pl = TPR._plane

    def resolve(mutate, rejitter=1):
        d, o = api.HipBackEndDesc(), api.HipBackEndOptions()
        d.hitDistParams[:] = HDP
        for s in (d.diffuse, d.specular):
            s.mode, s.resolve = int(S.REBLUR_SH), int(RES.SG)
            s.in0, s.in1, s.out = pl(sh, F.RGBA32_SFLOAT), pl(sh, F.RGBA32_SFLOAT), pl(out, F.RGBA32_SFLOAT)
        d.normalRoughness, d.viewZ, d.rf0 = pl(word, F[api.NORMAL_ROUGHNESS_FORMAT_NAME]), pl(z, F.R32_SFLOAT), pl(rf0, F.RGBA32_SFLOAT)
        d.commonSettings = C.cast(C.byref(persp), C.c_void_p)
        o.reJitter = rejitter
        o.outReJitterScale = pl(scale, F.RG32_SFLOAT)
        mutate(d, o)
        code = RC(lib.nrdHipResolveOutputsEx(C.byref(d), C.byref(o), None))
        text = lib.nrdHipGetLastFrontEndError().decode()
        assert text, "no error text for %s" % code.name
        return code, text

    def expect(result, code, *words):
        assert result[0] == code and all(word_ in result[1] for word_ in words), result

    expect(resolve(lambda d, o: setattr(d.diffuse, "mode", int(S.REBLUR_RADIANCE))), RC.INVALID_ARGUMENT, "reJitter", "SH")
    expect(resolve(lambda d, o: setattr(d.specular, "mode", int(S.NONE))), RC.INVALID_ARGUMENT, "reJitter", "SH")
    expect(resolve(lambda d, o: setattr(d.diffuse, "mode", int(S.REBLUR_DIRECTIONAL_OCCLUSION))), RC.INVALID_ARGUMENT, "reJitter")
    expect(resolve(lambda d, o: setattr(d.specular, "resolve", int(RES.SG_EXTRACT_COLOR))), RC.INVALID_ARGUMENT, "SG_EXTRACT_COLOR")
    expect(resolve(lambda d, o: setattr(d.diffuse, "resolve", int(RES.SG_EXTRACT_COLOR))), RC.INVALID_ARGUMENT, "SG_EXTRACT_COLOR")
    expect(resolve(lambda d, o: setattr(d.normalRoughness, "data", None)), RC.INVALID_ARGUMENT, "normalRoughness")
    expect(resolve(lambda d, o: setattr(d.viewZ, "data", None)), RC.INVALID_ARGUMENT, "viewZ")
    expect(resolve(lambda d, o: setattr(d.rf0, "data", None)), RC.INVALID_ARGUMENT, "rf0")
    expect(resolve(lambda d, o: setattr(d, "commonSettings", None)), RC.INVALID_ARGUMENT, "commonSettings")
    expect(resolve(lambda d, o: setattr(d, "remodulate", 1)), RC.INVALID_ARGUMENT, "albedo")  # albedo is needed with remodulation only
    expect(resolve(lambda d, o: setattr(o.outReJitterScale, "format", int(F.RGBA32_SFLOAT))), RC.UNSUPPORTED, "outReJitterScale")
    expect(resolve(lambda d, o: setattr(o.outReJitterScale, "width", 63)), RC.INVALID_ARGUMENT, "outReJitterScale")
    expect(resolve(lambda d, o: None, rejitter=0), RC.INVALID_ARGUMENT, "outReJitterScale", "without reJitter")
    assert RC(lib.nrdHipResolveOutputsEx(None, None, None)) == RC.INVALID_ARGUMENT

    keep = []

    def pack(mode, mutate=lambda d: None):
        d = TPR._front_desc(keep)
        mutate(d)
        o = api.HipFrontEndOptions(mode, 0)
        code = RC(lib.nrdHipPackInputsEx(C.byref(d), C.byref(o), None))
        return code, lib.nrdHipGetLastFrontEndError().decode()

    expect(pack(3), RC.INVALID_ARGUMENT, "checkerboardMode")
    expect(pack(0xFFFFFFFF), RC.INVALID_ARGUMENT, "checkerboardMode")
    expect(pack(int(CB.BLACK), lambda d: setattr(d.specular, "mode", 0)), RC.INVALID_ARGUMENT, "checkerboardMode", "signal")
    expect(pack(int(CB.WHITE), lambda d: setattr(d.viewZ, "data", None)), RC.INVALID_ARGUMENT, "viewZ")  # the rules of the plain call hold as before
    assert RC(lib.nrdHipPackInputsEx(None, None, None)) == RC.INVALID_ARGUMENT


@pytest.mark.parametrize("backend", BACKENDS)
def test_null_or_zeroed_options_are_the_old_entry_points(backend):
    """options NULL or all zero against nrdHipResolveOutputs / nrdHipPackInputs on the 67 x 23 planes: identical bytes, the whole stamped allocations included"""
    be, sc = Backend(backend), make_scene(W0, H0)
    p, lib, h, w = Planes(be, sc), be.lib, H0, W0
    d = p.dev

    def resolved(call):
        out, bigs = {}, {}
        for n in ("diffuse", "specular", "composed"):
            out[n], bigs[n] = be.padded((h, w, 4), "float32", 5, STAMP)
        res, desc, keep = frontend.describe_resolve(diffuse=dict(mode=S.REBLUR_SH, resolve=RES.SG, in0=d["diff_sh0"], in1=d["diff_sh1"]), specular=dict(mode=S.RELAX_SH, resolve=RES.SH, in0=d["spec_sh0"],
                                                    in1=d["spec_sh1"]), normal_roughness=d["word"], viewz=d["viewz"], rf0=d["rf0"], albedo=d["albedo"], remodulate=True, common_settings=sc["cs"],
                                                    hit_dist_params=HDP, want=("composed",), out=out)
        assert api.Result(call(desc)) == api.Result.SUCCESS, lib.nrdHipGetLastFrontEndError()
        return {n: be.down(b).copy() for n, b in bigs.items()}

    zero_back, zero_front = api.HipBackEndOptions(), api.HipFrontEndOptions()
    old = resolved(lambda desc: lib.nrdHipResolveOutputs(C.byref(desc), None))
    for what, call in (("NULL", lambda desc: lib.nrdHipResolveOutputsEx(C.byref(desc), None, None)), ("zeroed", lambda desc: lib.nrdHipResolveOutputsEx(C.byref(desc), C.byref(zero_back), None))):
        new = resolved(call)
        for n in old:
            assert_bits(new[n], old[n], "nrdHipResolveOutputsEx(%s) vs nrdHipResolveOutputs: %s" % (what, n))

    nr = be.up_pitched(np.concatenate([sc["V"], sc["rf0"][..., :1]], -1), 5)  # (any unit vectors and a roughness)
    probe = None

    def packed(call):
        nonlocal probe
        sig = lambda t: dict(mode=S.REBLUR_SH, radiance_hitdist=t, direction=d["albedo"])
        kw = dict(diffuse=sig(d["diff_sh0"]), specular=sig(d["spec_sh0"]), motion=d["rf0"], hit_dist_params=HDP, lib=lib)
        if probe is None:
            probe = frontend.describe_pack(nr, d["viewz"], **kw)[0]  # (shapes and dtypes)
        out, bigs = {}, {}
        for rt, (t, fmt) in probe.items():
            view, bigs[rt] = be.padded(tuple(t.shape), TPR.frontend._dtype_name(t), 5, STAMP if t.dtype not in (np.uint8, torch.uint8) else 0x5A)
            out[rt] = (view, fmt)
        res, desc, keep = frontend.describe_pack(nr, d["viewz"], out=out, **kw)
        assert api.Result(call(desc)) == api.Result.SUCCESS, lib.nrdHipGetLastFrontEndError()
        return {rt: be.down(b).copy() for rt, b in bigs.items()}

    old = packed(lambda desc: lib.nrdHipPackInputs(C.byref(desc), None))
    for what, call in (("NULL", lambda desc: lib.nrdHipPackInputsEx(C.byref(desc), None, None)), ("zeroed", lambda desc: lib.nrdHipPackInputsEx(C.byref(desc), C.byref(zero_front), None))):
        new = packed(call)
        for rt in old:
            assert_bits(new[rt], old[rt], "nrdHipPackInputsEx(%s) vs nrdHipPackInputs: %s" % (what, rt.name))


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4. another encoding (GPU, child process)
def encoding_case():
    """in a child process whose environment selects encoding (4, 2), as test_pack_resolve.encoding_case: 64-bit texels. The kernel's scale on the 67 x 23 scene against
    rejitter_rows --device built with this encoding's defines, bit for bit."""
    assert (api.NORMAL_ENCODING, api.ROUGHNESS_ENCODING) == TPR.ENCODING
    be, sc = Backend("hip"), make_scene(W0, H0)
    assert sc["word"].dtype == np.int16 and sc["word"].shape == (H0, W0, 4)
    p = Planes(be, sc)
    got = p.resolve(RES.SG, rejitter=True, want=("rejitter_scale",))
    want = header_scale(sc, p.values, "--device")
    assert_bits(got["rejitter_scale"], want, "rejitter_scale (RGBA16_SNORM texels) vs NRD.hip.h on the rows (device)")
    scaled = int((~np.all(want == 1.0, axis=-1)).sum())
    print("scaled pixels: %d" % scaled)
    assert scaled > 1000
    print("encoding_case OK")


@pytest.mark.gpu
def test_rejitter_in_another_g_buffer_encoding():
    env = dict(os.environ, NRD_NORMAL_ENCODING=str(TPR.ENCODING[0]), NRD_ROUGHNESS_ENCODING=str(TPR.ENCODING[1]))
    env.pop("NRD_HIP_LIBRARY", None)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_rejitter_checkerboard as T; T.encoding_case()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "encoding_case OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5. end to end with graph capture (GPU)
@pytest.mark.gpu
def test_end_to_end_rejittered_resolve_with_graph_capture():
    """RELAX_DIFFUSE_SPECULAR_SH, 192 x 128, 3 frames from the raw values of the synthetic sequence: pack -> denoise -> HipExecutor.resolve(rejitter=True, SG, remodulated), and
    the same pack and resolve calls captured by torch.cuda.graph (default queues, nothing else set) and replayed on the same planes: identical bytes. The descriptor's camera is read
    when the call is made, so a captured resolve holds the camera of its capture: the camera of this sequence moves, and the resolve is captured once per frame."""
    from raytracingdenoiser_amd.executor import HipExecutor

    name, mode, w, h, frames = "RELAX_DIFFUSE_SPECULAR_SH", S.RELAX_SH, 192, 128, 3
    seq = [synth.render_frame(w, h, f, want=tuple(parity.DENOISERS[name][1]) + ("raw",)) for f in range(frames)]
    inst = api.Instance([(0, parity.DENOISERS[name][0])])
    ex = HipExecutor(inst, w, h)
    outs = {rt: (torch.zeros((h, w, ch), dtype=dtype, device="cuda"), fmt) for rt, dtype, ch, fmt in parity.output_planes(name, w, h)}
    for rt, (t, fmt) in outs.items():
        ex.bind(rt, t, fmt)
    static = TPR._raw_inputs(seq[0])
    albedo = torch.cat([seq[0]["raw"]["albedo"], torch.zeros(h, w, 1)], -1).cuda().contiguous()
    rf0 = torch.full((h, w, 4), 0.04, device="cuda")
    rf0[..., 0] += 0.5 * albedo[..., 1]
    packed = TPR._pack_frame(static, mode)  # allocates the packed planes (and warms the launch path up) outside the capture
    ex.bind_packed(packed)
    torch.cuda.synchronize()
    g_pack = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_pack):
        TPR._pack_frame(static, mode, out=packed)
    kw = dict(diffuse_mode=mode, specular_mode=mode, resolve=RES.SG, albedo=albedo, rf0=rf0)
    full = dict(kw, rejitter=True, remodulate=True, want=("rejitter_scale", "factors", "composed"))
    replayed = None
    for f, frame in enumerate(seq):
        for k, v in TPR._raw_inputs(frame).items():
            static[k].copy_(v)
        TPR._pack_frame(static, mode, out=packed)
        eager_packed = {rt: t.cpu().numpy().copy() for rt, (t, fmt) in packed.items()}
        for t, fmt in packed.values():
            t.zero_()
        g_pack.replay()
        for rt, (t, fmt) in packed.items():
            assert_bits(t.cpu().numpy(), eager_packed[rt], "frame %d %s: captured pack == eager" % (f, rt.name))
        assert inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame)) == api.Result.SUCCESS
        assert inst.set_common_settings(parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], w, h, f)) == api.Result.SUCCESS
        ex.denoise()
        plain = {k: v.cpu().numpy() for k, v in ex.resolve(**kw).items()}
        got = {k: v.cpu().numpy() for k, v in ex.resolve(**full).items()}
        scale = got["rejitter_scale"]
        assert all(np.isfinite(v).all() for v in got.values()), "frame %d: not finite" % f
        assert scale.min() >= f32(1.0 / M.NRD_PI) and scale.max() <= f32(M.NRD_PI)
        border = np.ones((h, w), bool)
        border[1:-1, 1:-1] = False
        assert np.all(scale[border] == 1.0)
        assert np.any(scale != 1.0)  # (flat surfaces have equal neighbour normals and a scale of 1: only the curved part of the synthetic scene is scaled)
        print("frame %d: %.1f %% of the pixels scaled" % (f, 100.0 * np.mean(np.any(scale != 1.0, axis=-1))))
        colours = []
        for k, (which, factor) in enumerate((("diffuse", "diff_factor"), ("specular", "spec_factor"))):
            colours.append((plain[which][..., :3] * scale[..., k:k + 1]) * got[factor][..., :3])
            assert_bits(got[which][..., :3], colours[-1], "frame %d %s.rgb == ( plain.rgb * scale ) * factor" % (f, which))
            assert_bits(got[which][..., 3], plain[which][..., 3], "frame %d %s.w" % (f, which))
        assert_bits(got["composed"][..., :3], colours[0] + colours[1], "frame %d composed" % f)
        # the same call, captured and replayed on the same planes
        if replayed is None:
            replayed = {k: torch.zeros_like(v) for k, v in ex.resolve(**full).items()}
        for v in replayed.values():
            v.zero_()
        torch.cuda.synchronize()
        g_resolve = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_resolve):
            ex.resolve(out=replayed, stream=torch.cuda.current_stream(), **full)
        g_resolve.replay()
        torch.cuda.synchronize()
        for k, v in replayed.items():
            assert_bits(v.cpu().numpy(), got[k], "frame %d %s: captured resolve == eager" % (f, k))
    ex.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6. checkerboard planes
CB_CALLS = [S.REBLUR_RADIANCE, S.REBLUR_SH, S.REBLUR_OCCLUSION, S.RELAX_RADIANCE, S.RELAX_SH]  # the signal modes whose planes have a left half


def _checkerboard_expectation(d, w, h, exact):
    """{(mode, ResourceType): (expected plane, comparison)} of the NON-checkerboard call, as test_pack_resolve.check_pack builds it from the host dump: the specular side against B
    (bit for bit; the normalised hit distance of the REBLUR modes within one code on the GPU), the diffuse side against C (one code)"""
    crop = lambda a: TPR.img(d, a, w=w, h=h)
    hit, z = d["hitDist"][:, 0].astype(np.float64), d["viewZ"][:, 0].astype(np.float64)
    rad, dirn = d["radiance"].astype(np.float64), d["direction"].astype(np.float64)
    nhd = M.reblur_get_norm_hit_dist(hit, z, HDP, 1.0)
    sh0, sh1 = M.reblur_pack_sh(rad, nhd, dirn)
    r0, r1 = M.relax_pack_sh(rad, hit, dirn)
    f16, unorm16 = TPR.f16, TPR.unorm16
    nhd_w = "bits" if exact else "bits.xyz+codes.w"
    return {
        (S.REBLUR_RADIANCE, R.IN_SPEC_RADIANCE_HITDIST): (f16(crop(d["reblurPacked"])), nhd_w), (S.REBLUR_SH, R.IN_SPEC_SH0): (f16(crop(d["sh0"])), nhd_w),
        (S.REBLUR_SH, R.IN_SPEC_SH1): (f16(crop(d["sh1"])), "bits"), (S.REBLUR_OCCLUSION, R.IN_SPEC_HITDIST): (unorm16(crop(d["normHitDist"])), "bits" if exact else "unorm"),
        (S.RELAX_RADIANCE, R.IN_SPEC_RADIANCE_HITDIST): (f16(crop(d["relaxPacked"])), "bits"), (S.RELAX_SH, R.IN_SPEC_SH0): (f16(crop(d["relaxPacked"])), "bits"),
        (S.RELAX_SH, R.IN_SPEC_SH1): (f16(crop(d["relaxSh1"])), "bits"),
        (S.REBLUR_RADIANCE, R.IN_DIFF_RADIANCE_HITDIST): (f16(crop(M.reblur_pack_radiance_and_norm_hit_dist(rad, nhd))), "codes"), (S.REBLUR_SH, R.IN_DIFF_SH0): (f16(crop(sh0)), "codes"),
        (S.REBLUR_SH, R.IN_DIFF_SH1): (f16(crop(sh1)), "codes"), (S.REBLUR_OCCLUSION, R.IN_DIFF_HITDIST): (unorm16(crop(nhd)), "unorm"),
        (S.RELAX_RADIANCE, R.IN_DIFF_RADIANCE_HITDIST): (f16(crop(r0)), "codes"), (S.RELAX_SH, R.IN_DIFF_SH0): (f16(crop(r0)), "codes"), (S.RELAX_SH, R.IN_DIFF_SH1): (f16(crop(r1)), "codes")}


@pytest.mark.parametrize("backend", BACKENDS)
def test_checkerboard_planes_67x23(backend, dump):
    be, d = Backend(backend), dump
    w, h, pad = W0, H0, 7
    ins = TPR.pack_inputs_of(d, w, h)
    expectation = _checkerboard_expectation(d, w, h, backend == "emu")
    dev = {k: be.up_pitched(v, pad) for k, v in ins.items()}
    yy, xx = np.mgrid[0:h, 0:w]
    seen = set()
    for cb_mode in (CB.BLACK, CB.WHITE):
        cells = {"diffuse": 0, "specular": 1} if cb_mode == CB.BLACK else {"diffuse": 1, "specular": 0}  # as scene.user_planes assigns them
        for frame_index in (0, 1):
            # fp32 inputs of a signal: NaN wherever the pixel carries no data of that signal
            sig_in = {}
            for which, cell in cells.items():
                has = (((xx ^ yy) ^ frame_index) & 1) == cell
                sig_in[which] = tuple(be.up_pitched(np.where(has[..., None], ins[k], f32(np.nan)).astype(f32), pad) for k in ("rad", "direction"))
            for mode in CB_CALLS:
                kw = dict(diffuse=dict(mode=mode, radiance_hitdist=sig_in["diffuse"][0], direction=sig_in["diffuse"][1]),
                          specular=dict(mode=mode, radiance_hitdist=sig_in["specular"][0], direction=sig_in["specular"][1]), material_id=dev["material"], motion=dev["motion"],
                          hit_dist_params=HDP, lib=be.lib)
                plain = frontend.pack_inputs(dev["nr"], dev["viewz"], **dict(kw, diffuse=dict(kw["diffuse"], radiance_hitdist=dev["rad"], direction=dev["direction"]),
                                                                              specular=dict(kw["specular"], radiance_hitdist=dev["rad"], direction=dev["direction"])))
                out, bigs = {}, {}
                for rt, (t, fmt) in plain.items():
                    view, bigs[rt] = be.padded(tuple(t.shape), frontend._dtype_name(t), pad, STAMP)
                    out[rt] = (view, fmt)
                res = frontend.pack_inputs(dev["nr"], dev["viewz"], checkerboard_mode=cb_mode, frame_index=frame_index, out=out, **kw)
                for rt, (t, fmt) in res.items():
                    got, big = be.down(t).copy(), be.down(bigs[rt])
                    what = "%s frame %d %s %s" % (cb_mode.name, frame_index, mode.name, rt.name)
                    if not rt.name.startswith(("IN_DIFF", "IN_SPEC")):  # the G-buffer: the call without options, bit for bit
                        assert_bits(got, be.down(plain[rt][0]), what + " == the call without options")
                        continue
                    cell = cells["diffuse" if rt.name.startswith("IN_DIFF") else "specular"]
                    want, how = expectation[(mode, rt)]
                    seen.add((mode, rt))
                    moved = scene.checkerboard_pack(torch.from_numpy(want), cell, frame_index).numpy()
                    b = (cell ^ (yy[:, :1] & 1) ^ (frame_index & 1))
                    k = np.arange(w)[None, :]
                    written = (k < (w + 1) // 2) & (2 * k + b < w)  # texel (k, y) of the left half has a source pixel
                    assert written.sum() in (h * w // 2, (h * w + 1) // 2)
                    g, m = got[written], moved[written]
                    if how == "bits":
                        assert_bits(g, m, what)
                    elif how == "codes":
                        assert_codes(g, m, what)
                    elif how == "unorm":
                        assert_codes(g, m, what, unorm=True)
                    else:
                        assert_bits(g[..., :3], m[..., :3], what + " .xyz")
                        assert_codes(g[..., 3], m[..., 3], what + " .w")
                    assert np.isfinite(g.astype(f32)).all(), what
                    # every other byte of the allocation still holds the stamp: the right half, the sourceless texel of the left half, the padding
                    want_big = np.full(big.shape, STAMP, dtype=big.dtype)
                    want_big[:h, :w][written] = got[written]
                    assert np.array_equal(big.view(np.uint8), want_big.view(np.uint8)), what + ": a byte without a source pixel was written"
    assert seen == set(expectation)


dump = TPR.dump  # the host dump of tests/cpp/frontend_check, shared with test_pack_resolve (a module-scoped fixture: computed once here)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7. checkerboard end to end (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("name,cb_mode", [("REBLUR_DIFFUSE_SPECULAR", CB.BLACK), ("RELAX_DIFFUSE_SPECULAR", CB.WHITE)])
def test_end_to_end_checkerboarded_planes_from_the_kernel(name, cb_mode):
    """128 x 64, frames 0, 1, 2: the planes the kernel packed in checkerboard mode, downloaded and stepped through the CPU oracle with the same settings, give the outputs the executor
    gives on the device, bit for bit"""
    from raytracingdenoiser_amd.executor import HipExecutor

    w, h, frames = 128, 64, 3
    mode = S.REBLUR_RADIANCE if name.startswith("REBLUR") else S.RELAX_RADIANCE
    keys = {R.IN_DIFF_RADIANCE_HITDIST: "diff" if name.startswith("REBLUR") else "diff_relax", R.IN_SPEC_RADIANCE_HITDIST: "spec" if name.startswith("REBLUR") else "spec_relax"}
    overrides = dict(checkerboardMode=int(cb_mode))
    seq = [synth.render_frame(w, h, f, want=tuple(parity.DENOISERS[name][1]) + ("raw",)) for f in range(frames)]
    prev = oracle_driver.set_ieee_mode(False)
    try:
        ora = parity.OracleRun(name, w, h)
        inst = api.Instance([(0, parity.DENOISERS[name][0])])
        ex = HipExecutor(inst, w, h)
        outs = {rt: (torch.zeros((h, w, ch), dtype=dtype, device="cuda"), fmt) for rt, dtype, ch, fmt in parity.output_planes(name, w, h)}
        for rt, (t, fmt) in outs.items():
            ex.bind(rt, t, fmt)
        packed = None
        for f, frame in enumerate(seq):
            cs = lambda: parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], w, h, f)
            ins = TPR._raw_inputs(frame)
            if packed is None:
                packed = TPR._pack_frame(ins, mode)  # (allocates the planes)
            for rt in keys:
                packed[rt][0].fill_(17.0)  # nothing may read what the checkerboard call leaves unwritten
            frontend.pack_inputs(ins["nr"], ins["viewz"], material_id=ins["material"], motion=ins["motion"], diffuse=dict(mode=mode, radiance_hitdist=ins["diff"]),
                                 specular=dict(mode=mode, radiance_hitdist=ins["spec"]), hit_dist_params=HDP, out=packed, checkerboard_mode=cb_mode, frame_index=f)
            fed = dict(frame, normal_roughness=packed[R.IN_NORMAL_ROUGHNESS][0].cpu(), viewz=packed[R.IN_VIEWZ][0].cpu(), mv=packed[R.IN_MV][0].cpu(), **{key: packed[rt][0].cpu() for rt, key in keys.items()})
            fed["_checkerboard"] = None  # the planes are checkerboarded already
            assert (fed[keys[R.IN_DIFF_RADIANCE_HITDIST]][:, w // 2:] == 17.0).all()
            ora.step(fed, cs(), parity.denoiser_settings(name, frame, overrides))
            ex.bind_packed(packed)
            assert inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame, overrides)) == api.Result.SUCCESS
            assert inst.set_common_settings(cs()) == api.Result.SUCCESS
            ex.denoise()
            torch.cuda.synchronize()
            for rt, (t, fmt) in outs.items():
                assert_bits(t.cpu().numpy(), ora.outs[rt][0], "frame %d %s: executor on kernel-checkerboarded planes == oracle" % (f, rt.name))
        ex.destroy()
    finally:
        oracle_driver.set_ieee_mode(prev)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 8. static facts
def test_static_facts_of_the_new_kernels():
    """what the compiler made of the re-jitter kernel for gfx950 (tools/frontend_bench.py options_isa(), the `isa_options` object of profiles/frontend_bench.json): no scratch, and
    an LDS allocation of exactly the tile the source declares. VGPRs and waves are printed and recorded, not bounded. The checkerboard twin of the pack kernel meets the facts
    asserted of the pack kernel (tests/test_pack_resolve.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import frontend_bench

    facts = frontend_bench.options_isa()
    for name, k in facts.items():
        print(name, k)
    rj, cb = facts["rejitter"], facts["pack_checkerboard"]
    assert rj["scratch_bytes"] == 0
    assert rj["lds_bytes"] == rj["declared_tile_bytes"] == (64 + 2) * (4 + 2) * 16
    assert cb["scratch_bytes"] == 0 and cb["lds_bytes"] == 0 and cb["waves_per_simd"] >= 8 and 0 < cb["vgprs"] <= 64, cb
