"""TEST INFRASTRUCTURE. The nearest-Z rule of nrdHipResolveOutputsUpsampled and the decimation of nrdHipPackInputsDecimated (include/NRDHip.h), restated in float32 numpy from the
header text alone: multiply, abs, subtract and compare -- every value is the correctly rounded fp32 result, so `select_source` is exact on every backend.

What the model holds is the part the two calls add: WHICH low texel a full pixel takes (select_source), what a plane looks like once every pixel has fetched its texel (gather), and
which texels of a full-size plane a low pixel reads (decimate). What happens to a fetched texel is by the header's own words "the code of the plain call": the expectation of a colour
output is therefore the pre-existing nrdHipResolveOutputs / nrdHipResolveOutputsSplit on the gathered planes (expected_resolve) -- calls the suite holds against the reference text,
the host evaluation of NRD.hip.h and tests/frontend_model.py in tests/test_pack_resolve.py and tests/test_split_planes.py -- with zeros where the source is none."""
import numpy as np

f32 = np.float32
NONE = 255


def low_size(W, H):
    return (W + 1) >> 1, (H + 1) >> 1


def decimate(a):
    """the texels of a full-size plane that the low pixels stand for: ( 2i, 2j ), as a contiguous copy"""
    return np.ascontiguousarray(a[::2, ::2])


def select_source(viewz, low_viewz, viewz_scale, denoising_range, depth_threshold=0.0):
    """uint8 [H, W]: candidate k = a + 2b of every full pixel (0..3), NONE where it has none -- the rule of the header, candidate by candidate in the order k = 0, 1, 2, 3"""
    viewz, low_viewz = np.asarray(viewz, f32), np.asarray(low_viewz, f32)
    H, W = viewz.shape
    h, w = low_viewz.shape
    assert (w, h) == low_size(W, H)
    s, R, t = f32(viewz_scale), f32(denoising_range), f32(depth_threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        Zf = np.abs(viewz * s)
        in_range = ~(np.isnan(Zf) | (Zf > R))
        Y, X = np.mgrid[0:H, 0:W]
        source = np.full((H, W), NONE, np.uint8)
        best = np.zeros((H, W), f32)
        for k in range(4):
            a, b = k & 1, k >> 1
            i, j = (X >> 1) + a, (Y >> 1) + b
            exists = ((a == 0) | ((X & 1) == 1)) & ((b == 0) | ((Y & 1) == 1)) & (i < w) & (j < h)
            Zk = np.abs(low_viewz[np.minimum(j, h - 1), np.minimum(i, w - 1)] * s)
            valid = exists & in_range & ~np.isnan(Zk) & ~(Zk > R)
            dk = np.abs(Zk - Zf)
            assert dk.dtype == f32
            take = valid & ((source == NONE) | (dk < best))  # strictly smaller: a tie stays with the lowest k
            source = np.where(take, np.uint8(k), source)
            best = np.where(take, dk, best)
        if t > 0:
            source = np.where((source != NONE) & (best > t * Zf), np.uint8(NONE), source)
    return source


def source_coordinates(source):
    """(sy, sx, has): the low texel of every full pixel (0, 0 where it has none)"""
    H, W = source.shape
    Y, X = np.mgrid[0:H, 0:W]
    has = source != NONE
    k = np.where(has, source, 0).astype(np.int64)
    return np.where(has, (Y >> 1) + (k >> 1), 0), np.where(has, (X >> 1) + (k & 1), 0), has


def gather(low, source):
    """the full-size plane in which every pixel holds its source texel of `low` ([h, w] or [h, w, C]); zeros where it has none (a NaN of an unchosen texel never gets there)"""
    sy, sx, has = source_coordinates(source)
    out = low[sy, sx].copy()
    out[~has] = 0
    return np.ascontiguousarray(out)


def replicate(low, W, H):
    """plain pixel replication, the yardstick nearest Z is held against: full pixel ( X, Y ) takes low texel ( X >> 1, Y >> 1 )"""
    Y, X = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(low[Y >> 1, X >> 1])


def expected_resolve(frontend, lib, up, down, source, low_signals, **plain_kw):
    """what nrdHipResolveOutputsUpsampled must write, from the PLAIN resolve: low_signals = dict(diffuse=dict(mode=, resolve=, in0=, in1=), specular=..., shadow=array) over low-size
    host arrays; plain_kw: the full-size arguments of frontend.resolve_outputs (device arrays of the backend). Signal outputs, their hit-distance planes, "shadow" and "composed" are
    zero where the source is none; "view_vector" and the factors are the plain call's on every pixel. up / down: host array -> the backend's array and back."""
    kw = dict(plain_kw)
    for which in ("diffuse", "specular"):
        sig = low_signals.get(which)
        if sig is not None:
            kw[which] = dict(sig, in0=up(gather(sig["in0"], source)), **({"in1": up(gather(sig["in1"], source))} if sig.get("in1") is not None else {}))
    if low_signals.get("shadow") is not None:
        kw["shadow"] = up(gather(low_signals["shadow"], source))
    res = {k: np.array(down(v), copy=True) for k, v in frontend.resolve_outputs(lib=lib, **kw).items()}
    none = source == NONE
    for k in res:
        if k not in ("view_vector", "diff_factor", "spec_factor"):
            res[k][none] = 0
    return res
