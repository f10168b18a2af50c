"""Front end / back end on the device: plumbing over nrdHipPackInputs(Ex) / nrdHipResolveOutputs(Ex), nrdHipPack / ResolveShadowLights and nrdHipPackGuides (include/NRDHip.h).

pack_inputs() turns an application's fp32 buffers into the packed planes HipExecutor.bind accepts, resolve_outputs() turns the denoised OUT_* planes into
linear fp32 radiance -- one kernel launch each, asynchronous on the current stream, usable inside torch.cuda.graph. Buffers may be four-channel, or three-channel with `.w`
(roughness, hit distance) in an array of its own, as a tensor host holds them: those are read and written where they lie (nrdHipPackInputsSplit / nrdHipResolveOutputsSplit). This module allocates and calls the
C-ABI; it computes nothing (no arithmetic on tensors, no fallback). Planes are CUDA tensors; numpy arrays are accepted as well, for a library whose "device
memory" is host memory (the CPU emulation of the device sources that the test-suite builds).
"""
import ctypes as C
import inspect

import numpy as np

from . import api

F, R, SignalMode, ResolveMode = api.Format, api.ResourceType, api.SignalMode, api.ResolveMode
HIT_DIST_PARAMS = (3.0, 0.1, 20.0, -25.0)  # ReblurSettings::hitDistanceParameters defaults

_SH = (SignalMode.REBLUR_SH, SignalMode.RELAX_SH)
_NR_DTYPE = {"RGBA8_UNORM": ("int32", 1), "RGBA8_SNORM": ("int32", 1), "R10_G10_B10_A2_UNORM": ("int32", 1), "RGBA16_UNORM": ("int16", 4), "RGBA16_SNORM": ("int16", 4)}
# (first / second packed plane of a signal, per mode): dtype, channels, Format
_SIGNAL_OUT = {SignalMode.REBLUR_RADIANCE: ("float16", 4, F.RGBA16_SFLOAT), SignalMode.REBLUR_SH: ("float16", 4, F.RGBA16_SFLOAT), SignalMode.REBLUR_OCCLUSION: ("int16", 1, F.R16_UNORM),
               SignalMode.REBLUR_DIRECTIONAL_OCCLUSION: ("int16", 4, F.RGBA16_SNORM), SignalMode.RELAX_RADIANCE: ("float16", 4, F.RGBA16_SFLOAT), SignalMode.RELAX_SH: ("float16", 4, F.RGBA16_SFLOAT)}
_SLOTS = {  # ResourceType of (out0 / in0, out1 / in1) per signal and mode family; "IN" / "OUT" is prepended
    ("diffuse", "radiance"): ("DIFF_RADIANCE_HITDIST", None), ("specular", "radiance"): ("SPEC_RADIANCE_HITDIST", None), ("diffuse", "sh"): ("DIFF_SH0", "DIFF_SH1"),
    ("specular", "sh"): ("SPEC_SH0", "SPEC_SH1"), ("diffuse", "occlusion"): ("DIFF_HITDIST", None), ("specular", "occlusion"): ("SPEC_HITDIST", None),
    ("diffuse", "directional"): ("DIFF_DIRECTION_HITDIST", None)}


def _family(mode):
    mode = SignalMode(mode)
    return "sh" if mode in _SH else "occlusion" if mode == SignalMode.REBLUR_OCCLUSION else "directional" if mode == SignalMode.REBLUR_DIRECTIONAL_OCCLUSION else "radiance"


def signal_slots(which, mode, prefix):
    """(ResourceType of the first plane, of the second or None) of signal `which` ("diffuse" / "specular") in `mode`, for prefix = "IN" or "OUT"."""
    a, b = _SLOTS[(which, _family(mode))]
    return R[prefix + "_" + a], (R[prefix + "_" + b] if b else None)


# ---- array plumbing: torch tensors (CUDA) or numpy arrays ---------------------------------------------------------------------------------------------
def _is_numpy(t):
    return isinstance(t, np.ndarray)


def _ptr_pitch(t):
    if _is_numpy(t):
        assert t.strides[-1] == t.itemsize and (t.ndim == 2 or t.strides[1] == t.shape[2] * t.itemsize), "rows must be dense"
        return t.ctypes.data, t.strides[0]
    assert t[0].is_contiguous(), "rows must be dense"
    return t.data_ptr(), t.stride(0) * t.element_size()


def _dtype_name(t):
    return str(t.dtype).replace("torch.", "")


def _empty(like, shape, dtype):
    if _is_numpy(like):
        return np.empty(shape, dtype=dtype)
    import torch

    return torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)


def _plane(t, fmt):
    ptr, pitch = _ptr_pitch(t)
    return api.HipPlaneDesc(ptr, pitch, int(fmt), t.shape[1], t.shape[0])


def _fp32_plane(t, channels, what):
    """HipPlaneDesc of an fp32 [H, W, channels] ([H, W] for one channel) array"""
    assert _dtype_name(t) == "float32", "%s must be float32" % what
    assert (t.ndim == 2 and channels == 1) or (t.ndim == 3 and t.shape[2] == channels), "%s: expected %d channel(s) per pixel, got shape %s" % (what, channels, tuple(t.shape))
    return _plane(t, {1: F.R32_SFLOAT, 2: F.RG32_SFLOAT, 3: F.RGB32_SFLOAT, 4: F.RGBA32_SFLOAT}[channels])


def rgba(xyz, w=None):
    """[H, W, 3] (+ [H, W]) -> a new [H, W, 4] array, [N, H, W, 3] (+ [N, H, W]) -> a new [N, H, W, 4] one: copies only (the planes of the C-ABI are RGBA32_SFLOAT)"""
    out = _empty(xyz, tuple(xyz.shape[:-1]) + (4,), "float32")
    out[..., :3] = xyz
    if w is None:
        out[..., 3] = 0.0
    else:
        out[..., 3] = w
    return out


def _is_pair(t):
    return isinstance(t, (tuple, list))


def _rgba_arg(t, what, in_place=False, needs_w=False):
    """(array the plane points into, its HipPlaneDesc). Three-channel data -- an (xyz, w) pair or an [H, W, 3] array -- is widened into a new [H, W, 4] copy, or with in_place
    described where it lies as RGB32_SFLOAT (nrdHipPackInputsSplit / nrdHipResolveOutputsSplit; the w of a pair goes into the split struct: pack_split). needs_w: a plane whose .w
    is consumed -- a bare [H, W, 3] array has none to give in place and is widened with zeros as ever."""
    if _stays(t, in_place, needs_w):
        xyz = t[0] if _is_pair(t) else t
        return xyz, _fp32_plane(xyz, 3, what)
    if _is_pair(t):
        t = rgba(*t)
    elif t.ndim == 3 and t.shape[2] == 3:
        t = rgba(t)
    return t, _fp32_plane(t, 4, what)


def _stride0_bytes(t):
    return t.strides[0] if _is_numpy(t) else t.stride(0) * t.element_size()


def _rows_dense(t, channels):
    """are the rows of `t` ([.., W, channels], or [.., W] for channels = 0) dense float32 -- what a plane descriptor can point at"""
    strides = [x // t.itemsize for x in t.strides] if _is_numpy(t) else list(t.stride())
    want = [channels, 1] if channels else [1]
    return _dtype_name(t) == "float32" and (t.shape[-1] == channels or not channels) and strides[-len(want):] == want


def _stays(t, in_place, needs_w):
    """is three-channel data `t` -- an (xyz, w) pair, or an [.., 3] array where .w is not consumed -- described where it lies (see _rgba_arg)? Data whose rows are not dense
    (a [..., :3] view of a wider tensor) is widened as ever."""
    if not in_place:
        return False
    if _is_pair(t):
        return (t[0] is None or _rows_dense(t[0], 3)) and _rows_dense(t[1], 0)
    return not needs_w and t.shape[-1] == 3 and _rows_dense(t, 3)


def _layers(t, in_place=False, needs_w=False):
    """(is it a stack of sample layers, N, bytes from one layer to the next) of a signal argument: [N, H, W, 4], [N, H, W, 3] or an ([N, H, W, 3], [N, H, W]) pair are stacks --
    a three-channel stack is widened into a dense copy, or with in_place described where it lies -- anything else is one layer"""
    first = t[0] if _is_pair(t) else t
    if first is None or first.ndim != 4:
        return False, 1, 0
    if (_is_pair(t) or first.shape[3] == 3) and not _stays(t, in_place, needs_w):
        return True, first.shape[0], first.shape[1] * first.shape[2] * 16
    return True, first.shape[0], _stride0_bytes(first)


def _signal_arg(t, what, in_place=False, needs_w=False):
    """_rgba_arg for a signal plane that may be a stack of sample layers: the plane is that of layer 0"""
    if not _layers(t)[0]:
        return _rgba_arg(t, what, in_place, needs_w)
    if _stays(t, in_place, needs_w):
        xyz = t[0] if _is_pair(t) else t
        return xyz, _fp32_plane(xyz[0], 3, what)
    if _is_pair(t):
        t = rgba(*t)
    elif t.shape[3] == 3:
        t = rgba(t)
    return t, _fp32_plane(t[0], 4, what)


def _stream(like, stream):
    if stream is not None:
        return C.c_void_p(getattr(stream, "cuda_stream", stream))
    if _is_numpy(like):
        return C.c_void_p(0)
    import torch

    return C.c_void_p(torch.cuda.current_stream(like.device).cuda_stream)


class _stream_scope:
    """torch tensors: makes `stream` (a torch.cuda.Stream) the current one for the body, so that what the body allocates -- the output planes, and with in_place=False the widened
    [H, W, 4] copies of three-channel inputs, which die when the call returns while the launch is still in flight -- is allocated, filled and released in the order of the
    stream the kernel runs on (the caching allocator is stream-ordered). A raw stream handle (an int) cannot be made current: such a caller passes `out`, and three-channel
    inputs in place (the default) or four-channel planes."""

    def __init__(self, like, stream):
        self.ctx = None
        if stream is not None and not _is_numpy(like) and hasattr(stream, "cuda_stream"):
            import torch

            self.ctx = torch.cuda.stream(stream)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


def _check(lib, code, what):
    r = api.Result(code)
    if r != api.Result.SUCCESS:
        raise RuntimeError("%s failed: %s (%s)" % (what, r.name, lib.nrdHipGetLastFrontEndError().decode()))


def _settings_ptr(cs):
    return C.cast(C.byref(cs), C.c_void_p) if cs is not None else None


def _reuse(out, key, like, shape, dtype):
    if out is not None and key in out:
        t = out[key][0] if isinstance(out[key], tuple) else out[key]
        assert tuple(t.shape) == tuple(shape) and _dtype_name(t) == dtype, "out[%s] has the wrong shape or dtype" % (key,)
        return t
    return _empty(like, shape, dtype)


# ---- front end -------------------------------------------------------------------------------------------------------------------------------------------
def pack_inputs(normal_roughness, viewz, *args, checkerboard_mode=api.CheckerboardMode.OFF, frame_index=0, lobes=None, direct=None, **kw):
    """see describe_pack; launches on `stream` (a torch.cuda.Stream or a raw handle; default: the current stream) and returns the packed planes. Three-channel arrays, (xyz, w)
    pairs and [N, H, W, 3] stacks are read where they lie through nrdHipPackInputsSplit -- no copy, no allocation (in_place=False: widened into [.., 4] copies first, as before;
    that path allocates, so a raw stream handle suits it with four-channel inputs only); four-channel arguments take the calls they always took.
    checkerboard_mode (api.CheckerboardMode) other than OFF: the noisy signals are traced for every other pixel of frame `frame_index` (CommonSettings::frameIndex) and their
    texels go to the left half of the signal planes, whose other texels are left as they are (NRDHip.h nrdHipPackInputsEx). A signal given as a stack of sample layers
    ([N, H, W, 4]: many paths per pixel) or hit_dist_trim != 0 goes through nrdHipPackInputsSamples, which reduces the layers by the reference's rules in the same launch;
    every other call is the call it was.
    guide_shift=1 (quarter-resolution tracing, NRDHip.h nrdHipPackInputsDecimated): normal_roughness, viewz, material_id, motion, albedo and rf0 are the FULL-size [H, W] G-buffer,
    read at every second texel of every second row; the signals, distance_to_occluder and translucency are traced at the low size [(H + 1) >> 1, (W + 1) >> 1], which is the size
    of every packed plane returned; common_settings (demodulation) is that of the low-size frame.
    lobes= (one traced lobe per pixel: the probabilistic diffuse / specular split, NRDHip.h nrdHipPackInputsLobes): a dict of pack_lobes' arguments, or what pack_lobes returned.
    diffuse and specular are then dict(mode=SignalMode) alone -- both are built from the one traced plane set in the same launch.
    direct= (combined denoising of direct and indirect lighting, NRDHip.h nrdHipPackInputsDirect): a dict of pack_direct's arguments, or what pack_direct returned. The planes of
    diffuse / specular are then the INDIRECT ones; the direct radiance is added to each signal in the same launch and the diffuse hit distance is mixed by the reference's rule."""
    given = inspect.signature(describe_pack).bind(normal_roughness, viewz, *args, **kw).arguments
    in_place = given.get("in_place")
    in_place = PACK_IN_PLACE if in_place is None else bool(in_place)
    kw = dict(kw, in_place=in_place)
    with _stream_scope(viewz, kw.get("stream")):
        res, d, keep = describe_pack(normal_roughness, viewz, *args, **kw)
        lib = kw.get("lib") or api.load_library()
        layered = any(_layers(sig[k])[0] for sig in (given.get("diffuse"), given.get("specular")) if sig for k in ("radiance_hitdist", "direction") if sig.get(k) is not None)
        split = pack_split(normal_roughness, given.get("diffuse"), given.get("specular")) if in_place else None
        if direct is not None:  # one entry point for plain, sampled, split and decimated planes, like nrdHipPackInputsDecimated
            assert lobes is None, "direct: combining with lobes is out of scope"
            di, keep_direct = pack_direct(**direct) if isinstance(direct, dict) else direct
            in_place_here = split is not None and _anything_split(d, split)
            samples = pack_samples(given.get("diffuse"), given.get("specular"), given.get("hit_dist_trim", 0.0), in_place=in_place_here)
            options = pack_options(checkerboard_mode, frame_index)
            split = split if in_place_here else api.HipFrontEndSplit()
            _check(lib, lib.nrdHipPackInputsDirect(C.byref(d), C.byref(options), C.byref(samples), C.byref(split), C.byref(di), int(given.get("guide_shift", 0)),
                                                   _stream(viewz, kw.get("stream"))), "nrdHipPackInputsDirect")
        elif lobes is not None:
            assert int(given.get("guide_shift", 0)) == 0 and given.get("hit_dist_trim", 0.0) == 0.0, "lobes: neither decimation nor a trim threshold"
            lo, keep_lobes = pack_lobes(**lobes) if isinstance(lobes, dict) else lobes
            options = pack_options(checkerboard_mode, frame_index)
            split = split if split is not None else api.HipFrontEndSplit()
            _check(lib, lib.nrdHipPackInputsLobes(C.byref(d), C.byref(options), C.byref(split), C.byref(lo), _stream(viewz, kw.get("stream"))), "nrdHipPackInputsLobes")
        elif int(given.get("guide_shift", 0)) != 0:  # quarter-resolution tracing (NRDHip.h nrdHipPackInputsDecimated): one entry point for plain, sampled and split planes
            in_place_here = split is not None and _anything_split(d, split)
            samples = pack_samples(given.get("diffuse"), given.get("specular"), given.get("hit_dist_trim", 0.0), in_place=in_place_here)
            options = pack_options(checkerboard_mode, frame_index)
            split = split if in_place_here else api.HipFrontEndSplit()
            _check(lib, lib.nrdHipPackInputsDecimated(C.byref(d), C.byref(options), C.byref(samples), C.byref(split), int(given["guide_shift"]), _stream(viewz, kw.get("stream"))),
                   "nrdHipPackInputsDecimated")
        elif split is not None and _anything_split(d, split):  # three-channel planes and (xyz, w) pairs where they lie (NRDHip.h nrdHipPackInputsSplit): no copy, no allocation
            samples = pack_samples(given.get("diffuse"), given.get("specular"), given.get("hit_dist_trim", 0.0), in_place=True)
            options = pack_options(checkerboard_mode, frame_index)
            _check(lib, lib.nrdHipPackInputsSplit(C.byref(d), C.byref(options), C.byref(samples), C.byref(split), _stream(viewz, kw.get("stream"))), "nrdHipPackInputsSplit")
        elif layered or given.get("hit_dist_trim", 0.0) != 0.0:  # many paths per pixel (NRDHip.h nrdHipPackInputsSamples)
            samples = pack_samples(given.get("diffuse"), given.get("specular"), given.get("hit_dist_trim", 0.0))
            options = pack_options(checkerboard_mode, frame_index)
            _check(lib, lib.nrdHipPackInputsSamples(C.byref(d), C.byref(options), C.byref(samples), _stream(viewz, kw.get("stream"))), "nrdHipPackInputsSamples")
        elif int(checkerboard_mode) == 0:
            _check(lib, lib.nrdHipPackInputs(C.byref(d), _stream(viewz, kw.get("stream"))), "nrdHipPackInputs")
        else:
            options = pack_options(checkerboard_mode, frame_index)
            _check(lib, lib.nrdHipPackInputsEx(C.byref(d), C.byref(options), _stream(viewz, kw.get("stream"))), "nrdHipPackInputsEx")
    return res


def pack_options(checkerboard_mode=api.CheckerboardMode.OFF, frame_index=0):
    """api.HipFrontEndOptions for nrdHipPackInputsEx, next to the descriptor of describe_pack"""
    return api.HipFrontEndOptions(int(checkerboard_mode), int(frame_index) & 0xFFFFFFFF)


def pack_samples(diffuse=None, specular=None, hit_dist_trim=0.0, in_place=False):
    """api.HipFrontEndSamples for nrdHipPackInputsSamples, next to the descriptor of describe_pack, from the same diffuse / specular dicts: the sample counts and the layer
    strides (the arrays' stride(0); a three-channel stack or a pair is widened by describe_pack into a dense [N, H, W, 4] copy -- with in_place, as given to describe_pack,
    it stays where it is and the stride is its own). hit_dist_trim > 0: every sample's hit distance goes through NRD_FrontEnd_TrimHitDistance first."""
    samples = api.HipFrontEndSamples()
    samples.hitDistTrimThreshold = float(hit_dist_trim)
    for sig, dst in ((diffuse, samples.diffuse), (specular, samples.specular)):
        if sig is None:
            continue
        rh = sig["radiance_hitdist"]
        if _is_pair(rh) and rh[0] is None:  # the occlusion mode on its hit-distance plane alone (in_place)
            dst.samplesNum = rh[1].shape[0] if rh[1].ndim == 3 else 1
        else:
            _, dst.samplesNum, dst.radianceHitDistLayerBytes = _layers(rh, in_place, True)
        if sig.get("direction") is not None:
            _, n, dst.directionLayerBytes = _layers(sig["direction"], in_place)
            assert n == dst.samplesNum, "direction and radiance_hitdist must have the same number of sample layers"
    return samples


def pack_lobes(radiance_hit_dist, lobe, probability=None, direction=None):
    """(api.HipFrontEndLobes, arrays it points into) for nrdHipPackInputsLobes, next to a descriptor of describe_pack whose diffuse / specular dicts hold a mode alone. Everything
    is read where it lies, [H, W, ..] for one sample per pixel or [N, H, W, ..] stacks the way pack_samples takes them (the layer stride is stride(0)):
    radiance_hit_dist float32 [.., 4], or a (radiance [.., 3], hit_dist [..]) pair, or (None, hit_dist) when both modes read the hit distance alone -- what the ONE traced
    path returned; lobe uint8 [..]: api.Lobe.DIFFUSE / SPECULAR, any other byte = nothing traced; probability float32 [..] or None: the probability with which the SPECULAR lobe
    is chosen (None: the radiance is already divided by it); direction float32 [.., 3] or [.., 4]: needed when a signal's mode reads one."""
    lo, keep = api.HipFrontEndLobes(), [radiance_hit_dist, lobe, probability, direction]
    assert _dtype_name(lobe) == "uint8" and lobe.ndim in (2, 3), "lobe: uint8 [H, W] or [N, H, W]"
    n = lobe.shape[0] if lobe.ndim == 3 else 1

    def stack(t, plane_ndim, what):
        assert t.ndim in (plane_ndim, plane_ndim + 1) and (t.shape[0] if t.ndim > plane_ndim else 1) == n, "%s: %d sample layer(s) expected, got shape %s" % (what, n, tuple(t.shape))
        return (t[0], _stride0_bytes(t)) if t.ndim > plane_ndim else (t, 0)

    layer, lo.lobeLayerBytes = stack(lobe, 2, "lobe")
    lo.lobe, lo.samplesNum = _plane(layer, F.R8_UINT), n
    xyz, w = radiance_hit_dist if _is_pair(radiance_hit_dist) else (radiance_hit_dist, None)
    if xyz is not None:
        layer, lo.radianceHitDistLayerBytes = stack(xyz, 3, "radiance_hit_dist")
        lo.radianceHitDist = _fp32_plane(layer, 4 if w is None else 3, "radiance_hit_dist")
    if w is not None:
        layer, lo.hitDistLayerBytes = stack(w, 2, "hit_dist")
        lo.hitDist = _fp32_plane(layer, 1, "hit_dist")
    if probability is not None:
        layer, lo.probabilityLayerBytes = stack(probability, 2, "probability")
        lo.probability = _fp32_plane(layer, 1, "probability")
    if direction is not None:
        layer, lo.directionLayerBytes = stack(direction, 3, "direction")
        lo.direction = _xyz_plane(layer, "direction")
    return lo, keep


def pack_direct(diffuse=None, specular=None, max_hit_dist_contribution=api.DIRECT_MAX_CONTRIBUTION_DEFAULT):
    """(api.HipFrontEndDirect, arrays it points into) for nrdHipPackInputsDirect, next to a descriptor of describe_pack whose diffuse / specular planes are the INDIRECT ones.
    diffuse / specular: the signal's direct plane, or dict(radiance_hitdist=, direction=) in the SH modes, or None (no direct term). Everything is read where it lies, one layer
    [H, W, ..] under every sample or an [N, H, W, ..] stack with the signal's own N (the layer stride is stride(0)): radiance_hitdist float32 [.., 4] -- direct radiance and the
    distance to the sampled light -- or a (radiance [.., 3], hit_dist [..]) pair, or radiance [.., 3] alone where no direct distance is read (the specular signal always;
    the diffuse one with max_hit_dist_contribution = 0); direction float32 [.., 3] or [.., 4]: the direction to the light.
    max_hit_dist_contribution in [0, 1]: the cap of the weight with which the diffuse hit distance moves from the indirect to the direct one (0.5; the reference's README:
    "0.65 works good as well"); 0 keeps the indirect one."""
    di, keep = api.HipFrontEndDirect(), [diffuse, specular]
    di.maxHitDistContribution = float(max_hit_dist_contribution)

    def stack(t, plane_ndim):
        return (t[0], t.shape[0], _stride0_bytes(t)) if t.ndim > plane_ndim else (t, 1, 0)

    for which, sig, dst in (("diffuse", diffuse, di.diffuse), ("specular", specular, di.specular)):
        if sig is None:
            continue
        sig = sig if isinstance(sig, dict) else dict(radiance_hitdist=sig)
        xyz, w = sig["radiance_hitdist"] if _is_pair(sig["radiance_hitdist"]) else (sig["radiance_hitdist"], None)
        layer, dst.samplesNum, dst.radianceHitDistLayerBytes = stack(xyz, 3)
        dst.radianceHitDist = _xyz_plane(layer, "direct %s radiance_hitdist" % which)
        if w is not None:
            layer, n, dst.hitDistLayerBytes = stack(w, 2)
            assert n == dst.samplesNum, "direct %s: hit_dist and radiance must have the same number of layers" % which
            dst.hitDist = _fp32_plane(layer, 1, "direct %s hit_dist" % which)
        if sig.get("direction") is not None:
            layer, n, dst.directionLayerBytes = stack(sig["direction"], 3)
            assert n == dst.samplesNum, "direct %s: direction and radiance must have the same number of layers" % which
            dst.direction = _xyz_plane(layer, "direct %s direction" % which)
    return di, keep


# Whether pack_inputs takes three-channel input where it lies by default (in_place=None). Decided by tools/frontend_bench.py --split (the `split` object of
# profiles/frontend_bench.json): at 2560 x 1440 the in-place call takes 0.068 ms against 0.119 ms of widening + 0.066 ms of the four-channel call.
PACK_IN_PLACE = True


def pack_split(normal_roughness, diffuse=None, specular=None):
    """api.HipFrontEndSplit for nrdHipPackInputsSplit, next to the descriptor of describe_pack(in_place=True), from the same arguments: the w halves of the (xyz, w) pairs --
    roughness [H, W] of a (normal, roughness) pair, hit_dist [H, W] (or [N, H, W] with its layer stride) of a (radiance, hit_dist) pair; (None, hit_dist) in the occlusion mode.
    The struct points at the caller's arrays: a relaunch sees what they hold then."""
    split = api.HipFrontEndSplit()
    if _stays(normal_roughness, True, True):
        split.roughness = _fp32_plane(normal_roughness[1], 1, "roughness")
    for which, sig in (("diffuse", diffuse), ("specular", specular)):
        if sig is None or sig.get("radiance_hitdist") is None or not _stays(sig["radiance_hitdist"], True, True):  # (None: the traced planes are those of pack_lobes)
            continue
        hit = sig["radiance_hitdist"][1]
        if hit.ndim == 3:
            setattr(split, which + "HitDistLayerBytes", _stride0_bytes(hit))
            hit = hit[0]
        setattr(split, which + "HitDist", _fp32_plane(hit, 1, which + " hit_dist"))
    return split


def _anything_split(d, split):
    planes = [d.normalRoughness, d.motion, d.albedo, d.rf0, d.translucency, d.diffuse.radianceHitDist, d.diffuse.direction, d.specular.radianceHitDist, d.specular.direction]
    return any(p.data and p.format == int(F.RGB32_SFLOAT) for p in planes) or any(p.data for p in (split.roughness, split.diffuseHitDist, split.specularHitDist))


def describe_pack(normal_roughness, viewz, material_id=None, motion=None, diffuse=None, specular=None, albedo=None, rf0=None, distance_to_occluder=None, translucency=None,
                  common_settings=None, hit_dist_params=HIT_DIST_PARAMS, viewz_scale=1.0, tan_of_light_angular_radius=0.0, out=None, stream=None, lib=None, hit_dist_trim=0.0,
                  in_place=None, guide_shift=0, direct=None):
    """The descriptor of one nrdHipPackInputs launch, without launching: (packed planes, api.HipFrontEndDesc, arrays the descriptor points into besides its arguments) -- for a
    caller that launches the same frame layout repeatedly through the C-ABI itself. fp32 inputs: normal_roughness [H, W, 4] (or a (normal [H, W, 3], roughness [H, W]) pair), viewz [H, W], material_id [H, W],
    motion [H, W, 4] or [H, W, 2], albedo / rf0 / translucency [H, W, 4] or [H, W, 3], distance_to_occluder [H, W]; diffuse / specular: dict(mode=SignalMode,
    radiance_hitdist=[H, W, 4] or (radiance [H, W, 3], hit_dist [H, W]), direction=[H, W, 4] or [H, W, 3] for the SH / directional modes). albedo + rf0 +
    common_settings switch demodulation on. Many paths per pixel: a signal's radiance_hitdist may be [N, H, W, 4] or ([N, H, W, 3], [N, H, W]) and its direction
    [N, H, W, 4] or [N, H, W, 3] with the same N (layers may be pitched or padded: the layer stride is stride(0)); the descriptor then holds layer 0 and pack_samples
    the rest, with hit_dist_trim, for nrdHipPackInputsSamples. Returns {ResourceType: (packed array, Format)}, ready for HipExecutor.bind_packed; `out` = a dict returned earlier, whose
    arrays are written again instead of allocating.
    in_place=True (default here: False -- the descriptor then suits nrdHipPackInputs / Ex / Samples): three-channel arrays, (xyz, w) pairs and [N, H, W, 3] stacks are not widened;
    the descriptor points at the caller's own arrays as RGB32_SFLOAT planes and is for nrdHipPackInputsSplit alone, with pack_split(...) for the w halves and
    pack_samples(..., in_place=True): a relaunch after the caller refreshed its tensors packs the new values. (A bare [H, W, 3] normal_roughness / radiance_hitdist, which has
    no w anywhere, is still widened with zeros.) A signal in the occlusion mode may give radiance_hitdist=(None, hit_dist).
    guide_shift=1: the descriptor is for nrdHipPackInputsDecimated( ..., guideShift = 1 ) alone -- the G-buffer arguments are full-size, everything else and every output low-size
    (see pack_inputs).
    direct= (what pack_direct returned, or a dict of its arguments): the descriptor is for nrdHipPackInputsDirect, its diffuse / specular planes are the indirect ones, and the
    third value returned ends with the api.HipFrontEndDirect to pass next to it."""
    in_place = bool(in_place)
    d = api.HipFrontEndDesc()
    keep = []  # widened copies must outlive the launch call
    di = None if direct is None else pack_direct(**direct) if isinstance(direct, dict) else direct
    nr, d.normalRoughness = _rgba_arg(normal_roughness, "normal_roughness", in_place, needs_w=True)
    keep.append(nr)
    h, w = viewz.shape
    assert int(guide_shift) in (0, 1), "guide_shift: 0 or 1"
    if int(guide_shift):  # the outputs have the low size
        h, w = (h + 1) >> 1, (w + 1) >> 1
    d.viewZ = _fp32_plane(viewz, 1, "viewz")
    d.commonSettings = _settings_ptr(common_settings)
    d.hitDistParams[:] = hit_dist_params
    d.viewZScale, d.tanOfLightAngularRadius = viewz_scale, tan_of_light_angular_radius
    res = {}

    def output(slot, shape, dtype, fmt):
        t = _reuse(out, slot, viewz, shape, dtype)
        res[slot] = (t, fmt)
        return _plane(t, fmt)

    nr_dtype, nr_ch = _NR_DTYPE[api.NORMAL_ROUGHNESS_FORMAT_NAME]
    d.outNormalRoughness = output(R.IN_NORMAL_ROUGHNESS, (h, w) if nr_ch == 1 else (h, w, nr_ch), nr_dtype, F[api.NORMAL_ROUGHNESS_FORMAT_NAME])
    d.outViewZ = output(R.IN_VIEWZ, (h, w), "float32", F.R32_SFLOAT)
    if material_id is not None:
        d.materialID = _fp32_plane(material_id, 1, "material_id")
    if motion is not None:
        assert motion.shape[2] != 3 or in_place, "motion [H, W, 3] is read in place only (in_place=True)"
        d.motion = _fp32_plane(motion, motion.shape[2], "motion")
        d.outMv = output(R.IN_MV, (h, w, 4), "float16", F.RGBA16_SFLOAT)
    for name, t in (("albedo", albedo), ("rf0", rf0)):
        if t is not None:
            t, plane = _rgba_arg(t, name, in_place)
            keep.append(t)
            setattr(d, name, plane)
    if distance_to_occluder is not None:
        d.distanceToOccluder = _fp32_plane(distance_to_occluder, 1, "distance_to_occluder")
        d.outPenumbra = output(R.IN_PENUMBRA, (h, w), "float16", F.R16_SFLOAT)
        if translucency is not None:
            t, d.translucency = _rgba_arg(translucency, "translucency", in_place)
            keep.append(t)
            d.outTranslucency = output(R.IN_TRANSLUCENCY, (h, w, 4), "uint8", F.RGBA8_UNORM)
    for which, sig, dst in (("diffuse", diffuse, d.diffuse), ("specular", specular, d.specular)):
        if sig is None:
            continue
        mode = SignalMode(sig["mode"])
        dst.mode = int(mode)
        rh = sig.get("radiance_hitdist")  # (None: a descriptor for nrdHipPackInputsLobes, whose traced planes are those of pack_lobes)
        if rh is not None and not (_stays(rh, in_place, True) and rh[0] is None):
            t, dst.radianceHitDist = _signal_arg(sig["radiance_hitdist"], which + " radiance_hitdist", in_place, needs_w=True)
            keep.append(t)
        if sig.get("direction") is not None:
            t, dst.direction = _signal_arg(sig["direction"], which + " direction", in_place)
            keep.append(t)
        slot0, slot1 = signal_slots(which, mode, "IN")
        dtype, ch, fmt = _SIGNAL_OUT[mode]
        dst.out0 = output(slot0, (h, w) if ch == 1 else (h, w, ch), dtype, fmt)
        if slot1 is not None:
            dst.out1 = output(slot1, (h, w, 4), "float16", F.RGBA16_SFLOAT)
    return res, d, keep + [common_settings] + ([] if di is None else [di[1], di[0]])


# ---- hit-distance coverage of a probabilistic split ----------------------------------------------------------------------------------------------------------
class HitDistCoverage:
    """what nrdHipCheckHitDistCoverage reported: in_range_pixels; per signal ("diffuse", "specular") empty -- in-range pixels whose own hit distance is 0 -- holes -- of those,
    the pixels with no valid sample in the searched area: certainly unreconstructable -- and first_hole, (x, y) of the raster-first one or None"""

    def __init__(self, words, width):
        words = [int(v) & 0xFFFFFFFF for v in words]
        self.in_range_pixels = words[0]
        self.empty = dict(diffuse=words[1], specular=words[2])
        self.holes = dict(diffuse=words[3], specular=words[4])
        self.first_hole = {k: None if v == 0xFFFFFFFF else (v % width, v // width) for k, v in (("diffuse", words[5]), ("specular", words[6]))}

    def __repr__(self):
        return "HitDistCoverage(in_range_pixels=%d, empty=%r, holes=%r, first_hole=%r)" % (self.in_range_pixels, self.empty, self.holes, self.first_hole)


def describe_coverage(viewz, diffuse=None, specular=None, area=api.HitDistanceReconstructionMode.AREA_3X3, viewz_scale=1.0, denoising_range=500000.0):
    """api.HipCoverageDesc of one nrdHipCheckHitDistCoverage launch, without launching. viewz: the packed IN_VIEWZ array; diffuse / specular: the packed plane that carries the
    signal's hit distance, as bound -- IN_*_RADIANCE_HITDIST / IN_*_SH0 (float16 [H, W, 4]), IN_*_HITDIST (int16 [H, W]) or IN_DIFF_DIRECTION_HITDIST (int16 [H, W, 4]);
    area: HitDistanceReconstructionMode of the denoiser (1 = 3x3, 2 = 5x5); viewz_scale and denoising_range: those of its CommonSettings."""
    d = api.HipCoverageDesc()
    d.viewZ = _fp32_plane(viewz, 1, "viewz")
    if diffuse is not None:
        d.diffuse.plane = _packed_plane(diffuse, "diffuse")
    if specular is not None:
        d.specular.plane = _packed_plane(specular, "specular")
    d.viewZScale, d.denoisingRange, d.area = float(viewz_scale), float(denoising_range), int(area)
    return d


def check_hit_dist_coverage(viewz, diffuse=None, specular=None, area=api.HitDistanceReconstructionMode.AREA_3X3, viewz_scale=1.0, denoising_range=500000.0, stream=None, lib=None):
    """see describe_coverage; launches on `stream` (as pack_inputs), waits for it and returns a HitDistCoverage. The dithering that decides which lobe a pixel traces is the
    application's: this is how it learns that a pattern leaves pixels with no valid hit distance within the area the reconstruction searches."""
    d = describe_coverage(viewz, diffuse, specular, area, viewz_scale, denoising_range)
    lib = lib or api.load_library()
    with _stream_scope(viewz, stream):
        report = _empty(viewz, (7,), "int32")
        ptr = report.ctypes.data if _is_numpy(report) else report.data_ptr()
        _check(lib, lib.nrdHipCheckHitDistCoverage(C.byref(d), C.c_void_p(ptr), _stream(viewz, stream)), "nrdHipCheckHitDistCoverage")
        if not _is_numpy(report):
            import torch

            torch.cuda.synchronize(viewz.device)  # (a raw stream handle cannot be waited for through torch: the device is)
            report = report.cpu().numpy()
    return HitDistCoverage(report, viewz.shape[1])


# ---- back end --------------------------------------------------------------------------------------------------------------------------------------------
_IN_FORMAT = {("float16", 4): F.RGBA16_SFLOAT, ("float32", 4): F.RGBA32_SFLOAT, ("int16", 1): F.R16_UNORM, ("uint16", 1): F.R16_UNORM, ("int16", 4): F.RGBA16_SNORM, ("uint8", 1): F.R8_UNORM,
              ("uint8", 4): F.RGBA8_UNORM}


def _packed_plane(t, what):
    key = (_dtype_name(t), 1 if t.ndim == 2 else t.shape[2])
    assert key in _IN_FORMAT, "%s: no plane format for dtype %s with %d channel(s)" % (what, key[0], key[1])
    return _plane(t, _IN_FORMAT[key])


def resolve_outputs(rejitter=False, **kw):
    """see describe_resolve; launches on `stream` (as pack_inputs) and returns the fp32 planes. rejitter=True (both signals in an SH mode, resolve SH or SG; needs rf0): the
    resolved colours are multiplied by NRD_SG_ReJitter before the remodulation (NRDHip.h nrdHipResolveOutputsEx); "rejitter_scale" in `want` adds the two factors, fp32 [H, W, 2].
    channels=3 (describe_resolve) goes through nrdHipResolveOutputsSplit.
    low_viewz= (quarter-resolution denoising, NRDHip.h nrdHipResolveOutputsUpsampled): the signal planes and the shadow are the LOW-size OUT_* planes of the denoiser and low_viewz the
    IN_VIEWZ it ran with; normal_roughness, viewz, albedo and rf0 are full-size and so is every plane returned. Each full pixel takes its signal from the low texel around it that is
    nearest in depth (depth_threshold > 0: and no further than depth_threshold * depth away, else it gets zeros); want_source=True adds "source", uint8 [H, W]: which of the four
    texels (0..3), api.NO_SOURCE where none. common_settings is the denoiser's own (rectSize = the low size)."""
    like = next(t for t in (kw.get("shadow"), kw.get("viewz"), kw.get("normal_roughness"), (kw.get("diffuse") or {}).get("in0"), (kw.get("specular") or {}).get("in0")) if t is not None)
    with _stream_scope(like, kw.get("stream")):
        want = tuple(kw.get("want", ()))
        res, d, keep = describe_resolve(**dict(kw, want=tuple(n for n in want if n != "rejitter_scale")))
        lib = kw.get("lib") or api.load_library()
        if kw.get("low_viewz") is not None:
            options = resolve_options(res, kw["viewz"], rejitter=rejitter, want_scale="rejitter_scale" in want, out=kw.get("out"))
            split, upsample = resolve_split(res), resolve_upsample(res, kw["low_viewz"], kw.get("depth_threshold", 0.0))
            _check(lib, lib.nrdHipResolveOutputsUpsampled(C.byref(d), C.byref(options), C.byref(split), C.byref(upsample), _stream(like, kw.get("stream"))), "nrdHipResolveOutputsUpsampled")
        elif int(kw.get("channels", 4)) == 3:
            options = resolve_options(res, like, rejitter=rejitter, want_scale="rejitter_scale" in want, out=kw.get("out"))
            split = resolve_split(res)
            _check(lib, lib.nrdHipResolveOutputsSplit(C.byref(d), C.byref(options), C.byref(split), _stream(like, kw.get("stream"))), "nrdHipResolveOutputsSplit")
        elif not rejitter and "rejitter_scale" not in want:
            _check(lib, lib.nrdHipResolveOutputs(C.byref(d), _stream(like, kw.get("stream"))), "nrdHipResolveOutputs")
        else:
            options = resolve_options(res, like, rejitter=rejitter, want_scale="rejitter_scale" in want, out=kw.get("out"))
            _check(lib, lib.nrdHipResolveOutputsEx(C.byref(d), C.byref(options), _stream(like, kw.get("stream"))), "nrdHipResolveOutputsEx")
    return res


def resolve_options(res, like, rejitter=True, want_scale=False, out=None):
    """api.HipBackEndOptions for nrdHipResolveOutputsEx, next to the descriptor of describe_resolve: `res` is the dict describe_resolve returned, which gains
    "rejitter_scale" (fp32 [H, W, 2], allocated like `like` or taken from `out`) with want_scale"""
    options = api.HipBackEndOptions()
    options.reJitter = int(bool(rejitter))
    if want_scale:
        h, w = like.shape[:2]
        res["rejitter_scale"] = _reuse(out, "rejitter_scale", like, (h, w, 2), "float32")
        options.outReJitterScale = _plane(res["rejitter_scale"], F.RG32_SFLOAT)
    return options


def resolve_split(res):
    """api.HipBackEndSplit for nrdHipResolveOutputsSplit, next to the descriptor of describe_resolve(channels=3): `res` is the dict it returned, whose "diffuse_hit_dist" /
    "specular_hit_dist" planes (there when asked for in `want`) take the hit distances"""
    split = api.HipBackEndSplit()
    for which in ("diffuse", "specular"):
        if which + "_hit_dist" in res:
            setattr(split, which + "HitDist", _fp32_plane(res[which + "_hit_dist"], 1, which + "_hit_dist"))
    return split


def resolve_upsample(res, low_viewz, depth_threshold=0.0):
    """api.HipBackEndUpsample for nrdHipResolveOutputsUpsampled, next to the descriptor of describe_resolve(low_viewz=...): `res` is the dict it returned, whose "source" plane
    (there with want_source) takes the chosen texel of every pixel"""
    upsample = api.HipBackEndUpsample()
    upsample.lowViewZ = _fp32_plane(low_viewz, 1, "low_viewz")
    upsample.depthThreshold = float(depth_threshold)
    if "source" in res:
        upsample.outSource = _plane(res["source"], F.R8_UINT)
    return upsample


def describe_resolve(diffuse=None, specular=None, shadow=None, normal_roughness=None, viewz=None, albedo=None, rf0=None, common_settings=None, hit_dist_params=HIT_DIST_PARAMS,
                     denormalize_hit_dist=False, remodulate=False, want=(), out=None, stream=None, lib=None, channels=4, low_viewz=None, depth_threshold=0.0, want_source=False):
    """The descriptor of one nrdHipResolveOutputs launch, without launching: (fp32 planes, api.HipBackEndDesc, arrays it points into besides its arguments). diffuse / specular: dict(mode=SignalMode, resolve=ResolveMode, in0=OUT_*_RADIANCE_HITDIST / _SH0 / _HITDIST / DIRECTION_HITDIST array,
    in1=OUT_*_SH1 array) -- the arrays bound as outputs (fp16 / int16) or fp32 [H, W, 4]; shadow: the OUT_SHADOW_TRANSLUCENCY array (uint8 [H, W] or [H, W, 4]);
    normal_roughness / viewz: the packed IN_NORMAL_ROUGHNESS / IN_VIEWZ arrays; want: any of "composed", "view_vector", "factors". Returns fp32 arrays under
    "diffuse", "specular", "shadow", "composed", "view_vector", "diff_factor", "spec_factor".
    channels=3 (default 4): "diffuse", "specular", "composed", "view_vector", "diff_factor" and "spec_factor" are [H, W, 3] (RGB32_SFLOAT planes), the hit distances go to
    "diffuse_hit_dist" / "specular_hit_dist" [H, W] where `want` asks for them and nowhere otherwise, and albedo / rf0 given as [H, W, 3] are read where they lie; the
    descriptor is then for nrdHipResolveOutputsSplit alone, with resolve_split(res).
    low_viewz given (see resolve_outputs): in0 / in1 / shadow and low_viewz are low-size arrays, viewz (required) and the other inputs full-size, and every output has the size of
    viewz; want_source adds "source" (uint8 [H, W]). The descriptor is then for nrdHipResolveOutputsUpsampled alone, with resolve_split(res) and resolve_upsample(res, low_viewz,
    depth_threshold)."""
    assert channels in (3, 4), "channels: 3 or 4"
    colour, colour_format = (3, F.RGB32_SFLOAT) if channels == 3 else (4, F.RGBA32_SFLOAT)
    d = api.HipBackEndDesc()
    like = next(t for t in (shadow, viewz, normal_roughness, (diffuse or {}).get("in0"), (specular or {}).get("in0")) if t is not None)
    h, w = like.shape[:2]
    if low_viewz is not None:
        assert viewz is not None, "the upsampled resolve needs the full-size viewz next to low_viewz"
        h, w = viewz.shape[:2]
    keep, res = [], {}
    d.commonSettings = _settings_ptr(common_settings)
    d.hitDistParams[:] = hit_dist_params
    d.denormalizeHitDist, d.remodulate = int(bool(denormalize_hit_dist)), int(bool(remodulate))

    def output(name, shape, fmt, dtype="float32"):
        t = _reuse(out, name, like, shape, dtype)
        res[name] = t
        return _plane(t, fmt)

    if normal_roughness is not None:
        d.normalRoughness = _plane(normal_roughness, F[api.NORMAL_ROUGHNESS_FORMAT_NAME])
    if viewz is not None:
        d.viewZ = _fp32_plane(viewz, 1, "viewz")
    for name, t in (("albedo", albedo), ("rf0", rf0)):
        if t is not None:
            t, plane = _rgba_arg(t, name, channels == 3)
            keep.append(t)
            setattr(d, name, plane)
    for which, sig, dst in (("diffuse", diffuse, d.diffuse), ("specular", specular, d.specular)):
        if sig is None:
            continue
        mode = SignalMode(sig["mode"])
        dst.mode, dst.resolve = int(mode), int(sig.get("resolve", ResolveMode.SG_EXTRACT_COLOR))
        dst.in0 = _packed_plane(sig["in0"], which + " in0")
        if sig.get("in1") is not None:
            dst.in1 = _packed_plane(sig["in1"], which + " in1")
        dst.out = output(which, (h, w), F.R32_SFLOAT) if mode == SignalMode.REBLUR_OCCLUSION else output(which, (h, w, colour), colour_format)
        if channels == 3 and which + "_hit_dist" in want:
            assert mode != SignalMode.REBLUR_OCCLUSION, "the occlusion mode's output is the hit distance already"
            output(which + "_hit_dist", (h, w), F.R32_SFLOAT)
    if shadow is not None:
        d.shadow = _packed_plane(shadow, "shadow")
        d.outShadow = output("shadow", (h, w) + tuple(shadow.shape[2:]), F.R32_SFLOAT if shadow.ndim == 2 else F.RGBA32_SFLOAT)
    if "composed" in want:
        d.outComposed = output("composed", (h, w, colour), colour_format)
    if "view_vector" in want:
        d.outViewVector = output("view_vector", (h, w, colour), colour_format)
    if "factors" in want:
        d.outDiffFactor = output("diff_factor", (h, w, colour), colour_format)
        d.outSpecFactor = output("spec_factor", (h, w, colour), colour_format)
    if want_source:
        assert low_viewz is not None, "want_source: only the upsampled resolve (low_viewz=) has a source"
        output("source", (h, w), F.R8_UINT, "uint8")
    return res, d, keep + [common_settings]


# ---- SIGMA shadows for local and many lights ------------------------------------------------------------------------------------------------------------------
LightType, ShadowsMode = api.LightType, api.ShadowsMode


def shadow_lights(lights):
    """a ctypes array of api.HipShadowLight from a sequence whose entries are api.HipShadowLight, dicts (type=LightType, tan_of_light_angular_radius=, light_size=) or
    (type, value) pairs -- value is the tangent of the angular radius of a DIRECTIONAL light, the size of a LOCAL one"""
    table = (api.HipShadowLight * len(lights))()
    for dst, l in zip(table, lights):
        if isinstance(l, api.HipShadowLight):
            dst.type, dst.tanOfLightAngularRadius, dst.lightSize, dst.reserved = l.type, l.tanOfLightAngularRadius, l.lightSize, l.reserved
        elif isinstance(l, dict):
            dst.type, dst.tanOfLightAngularRadius, dst.lightSize = int(l["type"]), float(l.get("tan_of_light_angular_radius", 0.0)), float(l.get("light_size", 0.0))
        else:
            dst.type = int(l[0])
            if LightType(l[0]) == LightType.LOCAL:
                dst.lightSize = float(l[1])
            else:
                dst.tanOfLightAngularRadius = float(l[1])
    return table


def _light_stack(t, plane_ndim, what):
    """(layer 0, layers, bytes from one layer to the next) of a stack [N, H, W(, C)] or of one plane [H, W(, C)], read where it lies"""
    if t.ndim == plane_ndim:
        return t, 1, 0
    assert t.ndim == plane_ndim + 1, "%s: expected %d or %d dimensions, got shape %s" % (what, plane_ndim, plane_ndim + 1, tuple(t.shape))
    return t[0], t.shape[0], _stride0_bytes(t)


def light_stack(like, layers, plane_shape, dtype):
    """an uninitialised [layers, *plane_shape] stack, allocated like `like` (a CUDA tensor or a numpy array), whose layer stride meets the rule of NRDHip.h for light layers:
    a multiple of 4 bytes. A dense float16 [N, H, W] or uint8 [N, H, W] stack breaks it when H x W is odd / no multiple of 4, so the layers are padded and the stack is a view of
    them: every layer [i] is dense, the stack as a whole need not be."""
    elems, itemsize = int(np.prod(plane_shape)), np.dtype(dtype).itemsize
    padded = -(-elems * itemsize // 4) * 4 // itemsize
    flat = _empty(like, (layers, padded), dtype)[:, :elems]
    stack = flat.reshape((layers,) + tuple(plane_shape)) if _is_numpy(flat) else flat.view((layers,) + tuple(plane_shape))
    assert layers == 1 or _stride0_bytes(stack) == padded * itemsize  # (a view of the padded layers, not a copy)
    return stack


def shadow_stack(like, layers, height, width, channels=1):
    """the uint8 stack to bind OUT_SHADOW_TRANSLUCENCY layer by layer ([i]: R8_UNORM [H, W], or RGBA8_UNORM [H, W, 4] with channels=4) and to hand to resolve_shadow_lights as
    it is: see light_stack"""
    return light_stack(like, layers, (height, width) if channels == 1 else (height, width, channels), "uint8")


def _colour_stack(t, what):
    layer, n, stride = _light_stack(t, 3, what)
    assert layer.shape[2] in (3, 4), "%s: three or four channels per pixel" % what
    return _fp32_plane(layer, layer.shape[2], what), n, stride


def _scalar_stack(t, what):
    layer, n, stride = _light_stack(t, 2, what)
    return _fp32_plane(layer, 1, what), n, stride


def describe_pack_shadow_lights(lights, distance_to_occluder, distance_to_light=None, translucency=None, lighting=None, weight=None, mode=ShadowsMode.PER_LIGHT, out=None, stream=None,
                                lib=None):
    """The descriptor of one nrdHipPackShadowLights launch, without launching: (packed planes, api.HipShadowLightsPackDesc, what the descriptor points into besides its
    arguments). lights: see shadow_lights (N entries). fp32 inputs, one layer per light, read where they lie (stride(0) is the layer stride; [H, W(, C)] for one light):
    distance_to_occluder [N, H, W]; distance_to_light [N, H, W] (needed with a LOCAL light; the layer of a directional light is not read); translucency [N, H, W, 3 or 4]
    (PER_LIGHT); lighting [N, H, W, 3 or 4] and weight [N, H, W] (COMBINED). Returns {ResourceType: (array, Format)}:
      PER_LIGHT  IN_PENUMBRA [N, H, W] float16 and, with translucency, IN_TRANSLUCENCY [N, H, W, 4] uint8 -- layer i binds as IN_PENUMBRA / IN_TRANSLUCENCY of light i.
                 The stacks come from light_stack: every layer [i] is dense, the layer stride is rounded up to the 4 bytes NRDHip.h asks for
      COMBINED   IN_PENUMBRA [H, W], IN_TRANSLUCENCY [H, W, 4] and "lighting_sum" [H, W, 4] float32 ([H, W, 3] where `out` holds one)
    `out` = a dict returned earlier, whose arrays are written again instead of allocating."""
    mode = ShadowsMode(mode)
    table = shadow_lights(lights)
    d = api.HipShadowLightsPackDesc()
    d.mode, d.lightsNum, d.lights = int(mode), len(table), table
    d.distanceToOccluder, n, d.distanceToOccluderLayerBytes = _scalar_stack(distance_to_occluder, "distance_to_occluder")
    assert n == len(table), "distance_to_occluder holds %d layers for %d lights" % (n, len(table))
    h, w = distance_to_occluder.shape[-2:]
    for t, name, field, stack in ((distance_to_light, "distance_to_light", "distanceToLight", _scalar_stack), (translucency, "translucency", "translucency", _colour_stack),
                                  (lighting, "lighting", "lighting", _colour_stack), (weight, "weight", "weight", _scalar_stack)):
        if t is not None:
            plane, layers, stride = stack(t, name)
            assert layers == n, "%s holds %d layers for %d lights" % (name, layers, n)
            setattr(d, field, plane)
            setattr(d, field + "LayerBytes", stride)
    res = {}

    def output(slot, shape, dtype, fmt):
        if mode == ShadowsMode.PER_LIGHT and not (out is not None and slot in out):
            t = light_stack(distance_to_occluder, shape[0], shape[1:], dtype)  # (a dense [N, H, W] float16 stack of an odd frame would break the layer-stride rule)
        else:
            t = _reuse(out, slot, distance_to_occluder, shape, dtype)
        res[slot] = (t, fmt)
        layer, _, stride = _light_stack(t, len(shape) - (0 if mode == ShadowsMode.COMBINED else 1), str(slot))
        return _plane(layer, fmt), stride

    stack = () if mode == ShadowsMode.COMBINED else (n,)
    d.outPenumbra, d.outPenumbraLayerBytes = output(R.IN_PENUMBRA, stack + (h, w), "float16", F.R16_SFLOAT)
    if mode == ShadowsMode.COMBINED or translucency is not None:
        d.outTranslucency, d.outTranslucencyLayerBytes = output(R.IN_TRANSLUCENCY, stack + (h, w, 4), "uint8", F.RGBA8_UNORM)
    if mode == ShadowsMode.COMBINED:
        given = out["lighting_sum"] if out is not None and "lighting_sum" in out else None
        given = given[0] if isinstance(given, tuple) else given
        channels = 4 if given is None else given.shape[2]
        d.outLightingSum, _ = output("lighting_sum", (h, w, channels), "float32", F.RGB32_SFLOAT if channels == 3 else F.RGBA32_SFLOAT)
    return res, d, [table]


def pack_shadow_lights(lights, distance_to_occluder, *args, **kw):
    """see describe_pack_shadow_lights; launches on `stream` (as pack_inputs) and returns the packed planes: the front end of SIGMA for point, spot, sphere and directional
    lights, many of them per pixel, in one launch -- per light (mode=ShadowsMode.PER_LIGHT: denoise layer by layer with one SIGMA instance whose
    SigmaSettings.maxStabilizedFrameNum is 0, the README's "stabilizationStrength = 0") or combined into one SIGMA_SHADOW_TRANSLUCENCY pass (ShadowsMode.COMBINED)."""
    given = inspect.signature(describe_pack_shadow_lights).bind(lights, distance_to_occluder, *args, **kw).arguments  # (stream and lib wherever they were passed)
    with _stream_scope(distance_to_occluder, given.get("stream")):
        res, d, keep = describe_pack_shadow_lights(lights, distance_to_occluder, *args, **kw)
        lib = given.get("lib") or api.load_library()
        _check(lib, lib.nrdHipPackShadowLights(C.byref(d), _stream(distance_to_occluder, given.get("stream"))), "nrdHipPackShadowLights")
    return res


def describe_resolve_shadow_lights(shadow, lighting, mode=ShadowsMode.PER_LIGHT, lights_num=None, channels=4, out=None, stream=None, lib=None):
    """The descriptor of one nrdHipResolveShadowLights launch, without launching: (fp32 [H, W, channels] array, api.HipShadowLightsResolveDesc, arrays the descriptor points into besides its arguments). shadow: the denoised
    OUT_SHADOW_TRANSLUCENCY -- PER_LIGHT: a stack [N, H, W] or [N, H, W, 4] uint8 with lighting [N, H, W, 3 or 4], the unshadowed L_i; COMBINED: one [H, W, 4] plane with
    lighting = the "lighting_sum" of the pack call. The result is sum( L_i * shadow_i ) in .rgb (and, COMBINED with channels=4, the shadow in .w). `out`: an array to write.
    Layer strides are those of the arrays (stride(0)) and must be multiples of 4 bytes (16 for a four-channel lighting stack): a shadow stack from shadow_stack(...) is; a dense
    [N, H, W] uint8 one is only when H x W is a multiple of 4, and is otherwise copied into an aligned stack first (an allocation and a copy: the third element returned holds it)."""
    mode = ShadowsMode(mode)
    d = api.HipShadowLightsResolveDesc()
    d.mode = int(mode)
    keep = []
    plane_ndim = shadow.ndim - 1 if lighting.ndim == 4 else shadow.ndim  # (a stack where the lighting is one)
    if shadow.ndim > plane_ndim and shadow.shape[0] > 1 and _stride0_bytes(shadow) % 4:
        # a dense [N, H, W] uint8 stack whose H x W is no multiple of 4: the layer-stride rule of NRDHip.h refuses it. Copied into a stack that meets it (shadow_stack
        # allocates one to bind the denoiser's outputs to in the first place: no copy then)
        aligned = light_stack(shadow, shadow.shape[0], tuple(shadow.shape[1:]), "uint8")
        if _is_numpy(aligned):
            aligned[...] = shadow
        else:
            aligned.copy_(shadow)
        shadow = aligned
        keep.append(aligned)
    layer, n, d.shadowLayerBytes = _light_stack(shadow, plane_ndim, "shadow")
    d.shadow = _packed_plane(layer, "shadow")
    d.lighting, layers, d.lightingLayerBytes = _colour_stack(lighting, "lighting")
    assert layers == n, "lighting holds %d layers for %d shadow layers" % (layers, n)
    d.lightsNum = n if mode == ShadowsMode.PER_LIGHT else (lights_num or 1)
    h, w = layer.shape[:2]
    assert channels in (3, 4), "channels: 3 or 4"
    t = out if out is not None else _empty(shadow, (h, w, channels), "float32")
    d.out = _fp32_plane(t, t.shape[2], "out")
    return t, d, keep


def resolve_shadow_lights(shadow, lighting, *args, **kw):
    """see describe_resolve_shadow_lights; launches on `stream` (as pack_inputs) and returns the lit, shadowed radiance: the back end of pack_shadow_lights"""
    given = inspect.signature(describe_resolve_shadow_lights).bind(shadow, lighting, *args, **kw).arguments
    with _stream_scope(shadow, given.get("stream")):
        t, d, keep = describe_resolve_shadow_lights(shadow, lighting, *args, **kw)
        lib = given.get("lib") or api.load_library()
        _check(lib, lib.nrdHipResolveShadowLights(C.byref(d), _stream(shadow, given.get("stream"))), "nrdHipResolveShadowLights")
    return t


# ---- guides from world positions ------------------------------------------------------------------------------------------------------------------------------
MISS_VIEWZ = 1.0e6  # above the default CommonSettings.denoisingRange (5e5): the passes take such a pixel for sky


class PackedGuides(dict):
    """{ResourceType: (array, Format)} as HipExecutor.bind_packed takes it, plus `viewz`: the IN_VIEWZ array once more, the unscaled view depth to hand to pack_inputs"""

    viewz = None


def _xyz_plane(t, what):
    assert t.ndim == 3 and t.shape[2] in (3, 4), "%s: expected [H, W, 3] or [H, W, 4], got shape %s" % (what, tuple(t.shape))
    return _fp32_plane(t, t.shape[2], what)


def describe_pack_guides(position, common_settings=None, position_prev=None, miss_viewz=MISS_VIEWZ, base_color=None, metalness=None, diff_confidence=None, spec_confidence=None,
                         disocclusion_threshold_mix=None, out=None, stream=None, lib=None, want=("viewz", "mv")):
    """The descriptor of one nrdHipPackGuides launch, without launching: (PackedGuides, api.HipGuidesDesc, what the descriptor points into besides its arguments) -- for a caller
    that launches the same frame layout repeatedly through the C-ABI itself (the camera of common_settings is read at every call). fp32 inputs, read where they lie: position
    [H, W, 3] or [H, W, 4], the world-space position of the primary hit, NaN / INF on the sky (None: only the UNORM slots are wanted); position_prev, the same surface point one
    frame back (None: a static scene); base_color [H, W, 3 or 4] with metalness [H, W]; diff_confidence, spec_confidence, disocclusion_threshold_mix [H, W]. With a position:
    IN_VIEWZ [H, W] float32 (miss_viewz on the sky; binds as IN_VIEWZ when CommonSettings.viewZScale is 1) and IN_MV [H, W, 4] float16 in the convention of common_settings
    (motionVectorScale, isMotionVectorInWorldSpace). With their inputs: IN_BASECOLOR_METALNESS [H, W, 4] uint8, IN_DIFF_CONFIDENCE, IN_SPEC_CONFIDENCE,
    IN_DISOCCLUSION_THRESHOLD_MIX [H, W] uint8. want: which of the two position outputs, "viewz" and / or "mv" (default: both; position_prev is read by "mv" alone). `out` = a dict
    returned earlier, whose arrays are written again instead of allocating."""
    like = next(t for t in (position, base_color, diff_confidence, spec_confidence, disocclusion_threshold_mix) if t is not None)
    h, w = like.shape[:2]
    d = api.HipGuidesDesc()
    d.commonSettings = _settings_ptr(common_settings)
    d.missViewZ = float(miss_viewz)
    res = PackedGuides()

    def output(slot, shape, dtype, fmt):
        t = _reuse(out, slot, like, shape, dtype)
        res[slot] = (t, fmt)
        return _plane(t, fmt)

    if position is not None:
        want = tuple(want)
        assert want and set(want) <= {"viewz", "mv"}, "want: \"viewz\" and / or \"mv\""
        d.position = _xyz_plane(position, "position")
        if position_prev is not None:
            d.positionPrev = _xyz_plane(position_prev, "position_prev")
        if "viewz" in want:
            d.outViewZ = output(R.IN_VIEWZ, (h, w), "float32", F.R32_SFLOAT)
            res.viewz = res[R.IN_VIEWZ][0]
        if "mv" in want:
            d.outMv = output(R.IN_MV, (h, w, 4), "float16", F.RGBA16_SFLOAT)
    if base_color is not None or metalness is not None:
        assert base_color is not None and metalness is not None, "IN_BASECOLOR_METALNESS needs base_color and metalness"
        d.baseColor, d.metalness = _xyz_plane(base_color, "base_color"), _fp32_plane(metalness, 1, "metalness")
        d.outBaseColorMetalness = output(R.IN_BASECOLOR_METALNESS, (h, w, 4), "uint8", F.RGBA8_UNORM)
    for t, name, field, slot in ((diff_confidence, "diff_confidence", "DiffConfidence", R.IN_DIFF_CONFIDENCE), (spec_confidence, "spec_confidence", "SpecConfidence", R.IN_SPEC_CONFIDENCE),
                                 (disocclusion_threshold_mix, "disocclusion_threshold_mix", "DisocclusionThresholdMix", R.IN_DISOCCLUSION_THRESHOLD_MIX)):
        if t is not None:
            setattr(d, field[0].lower() + field[1:], _fp32_plane(t, 1, name))
            setattr(d, "out" + field, output(slot, (h, w), "uint8", F.R8_UNORM))
    return res, d, [common_settings]


def pack_guides(position, *args, **kw):
    """see describe_pack_guides; launches on `stream` (as pack_inputs) and returns the PackedGuides: IN_VIEWZ and IN_MV derived on the device from world-space positions and
    the matrices of common_settings, and the optional UNORM guide slots encoded from fp32 planes -- one launch (NRDHip.h nrdHipPackGuides). The dict goes to
    HipExecutor.bind_packed as it is; its `viewz` is the `viewz` argument of pack_inputs."""
    given = inspect.signature(describe_pack_guides).bind(position, *args, **kw).arguments
    like = next(t for t in (position, given.get("base_color"), given.get("diff_confidence"), given.get("spec_confidence"), given.get("disocclusion_threshold_mix")) if t is not None)
    with _stream_scope(like, given.get("stream")):
        res, d, keep = describe_pack_guides(position, *args, **kw)
        lib = given.get("lib") or api.load_library()
        _check(lib, lib.nrdHipPackGuides(C.byref(d), _stream(like, given.get("stream"))), "nrdHipPackGuides")
    return res
