"""numpy models for tests/test_pack_lobes.py and tests/test_hit_dist_coverage.py (include/NRDHip.h nrdHipPackInputsLobes / nrdHipCheckHitDistCoverage). Nothing here calls the
library: the planes an application would have had to build on the host before the plain pack calls, the one channel in which the lobes call differs from them (the diffuse hit
distance: a mean over the counted samples only), and the coverage stencil. float32 throughout, one numpy operation per fp32 operation of the header's text."""
import numpy as np

import frontend_model as M

f32 = np.float32
DIFFUSE, SPECULAR, NOTHING = 0, 1, 255
BAYER4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int32)
W, H = 67, 21  # odd, three tiles of 32 x 8 both ways, the last tile partly outside
DENOISING_RANGE = 500000.0
SKY_Z = f32(1.0e6)


def bayer_lobes(h, w, p, sample=0):
    """uint8 [h, w]: SPECULAR where the 4 x 4 Bayer threshold of the pixel (rotated per sample) is below p ([h, w] or a scalar: the probability of the specular lobe), else DIFFUSE"""
    y, x = np.mgrid[0:h, 0:w]
    threshold = (((BAYER4[y & 3, x & 3] + 7 * sample) & 15).astype(f32) + f32(0.5)) / f32(16)
    return np.where(threshold < np.asarray(p, f32), SPECULAR, DIFFUSE).astype(np.uint8)


def scene(n=1, w=W, h=H, seed=11):
    """the traced planes of a probabilistic split with n samples per pixel, and the G-buffer under them: a Bayer-dithered lobe plane with bytes of 255 (nothing traced),
    probabilities in [0.05, 0.95] plus exact 0 and 1 (a lobe chosen with probability 0 -- q = 0 -- must be skipped) and one NaN, NaN radiance / direction / hit distance wherever
    the sample does not count, sky pixels, and one pixel none of whose samples is diffuse."""
    rng = np.random.RandomState(seed)
    unit = lambda shape: (lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32))(rng.normal(size=shape + (3,)))
    s = dict(n=n, w=w, h=h)
    s["nr"] = np.concatenate([unit((h, w)), rng.uniform(0.05, 1.0, (h, w, 1)).astype(f32)], -1)
    s["viewz"] = rng.uniform(1.0, 50.0, (h, w)).astype(f32)
    s["viewz"][3, 40:44] = SKY_Z
    s["albedo"] = np.concatenate([rng.uniform(0.05, 1.0, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(f32)
    s["rf0"] = np.concatenate([rng.uniform(0.02, 0.9, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(f32)
    rad = np.concatenate([rng.uniform(0.0, 4.0, (n, h, w, 3)), rng.uniform(0.1, 30.0, (n, h, w, 1))], -1).astype(f32)
    dirn = np.concatenate([unit((n, h, w)), np.zeros((n, h, w, 1), f32)], -1)
    prob = rng.uniform(0.05, 0.95, (n, h, w)).astype(f32)
    lobe = np.stack([bayer_lobes(h, w, prob[k], k) for k in range(n)])
    prob[:, 5, 10:14] = 0.0  # p == 0: a SPECULAR sample there has q = 0 ...
    prob[:, 6, 10:14] = 1.0  # ... and p == 1 a DIFFUSE one
    lobe[:, 5, 10:12] = SPECULAR
    lobe[:, 5, 12:14] = DIFFUSE
    lobe[:, 6, 10:12] = DIFFUSE
    lobe[:, 6, 12:14] = SPECULAR
    prob[:, 7, 10] = np.nan  # a NaN probability: q is NaN for either lobe, nothing counts
    lobe[:, 9, 20:30] = NOTHING
    lobe[:, 12, 33] = SPECULAR  # no sample of this pixel is diffuse: n = 0
    lobe[n - 1, 14, 5] = NOTHING
    for X in (DIFFUSE, SPECULAR):
        assert (counted(lobe, prob, X).sum(0) == 0).any() and (counted(lobe, prob, X).sum(0) == n).any()
    nothing = ~(counted(lobe, prob, DIFFUSE) | counted(lobe, prob, SPECULAR))
    assert nothing.sum() >= 15 * n
    rad[nothing] = np.nan
    dirn[nothing] = np.nan
    s.update(rad=rad, dirn=dirn, prob=prob, lobe=lobe)
    return s


def selection(lobe, prob):
    """q of NRDHip.h: the probability with which the lobe of the sample was chosen; prob None: 1"""
    if prob is None:
        return np.ones(lobe.shape, f32)
    return np.where(lobe == SPECULAR, prob, f32(1.0) - prob).astype(f32)


def counted(lobe, prob, X):
    with np.errstate(invalid="ignore"):
        return (lobe == X) & (selection(lobe, prob) > 0)  # (false for a NaN)


def host_planes(s, X, with_probability=True):
    """what an application builds on the host for signal X before a plain pack call: ([.., 4] rad / q and h where the sample counts, zeros elsewhere; [.., 4] the direction there,
    ( 0, 0, 1 ) elsewhere), [n, h, w, 4] each"""
    prob = s["prob"] if with_probability else None
    keep = counted(s["lobe"], prob, X)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        scaled = np.concatenate([s["rad"][..., :3] / selection(s["lobe"], prob)[..., None], s["rad"][..., 3:]], -1).astype(f32)
    rad = np.where(keep, scaled, f32(0)).astype(f32)
    dirn = np.where(keep, s["dirn"], np.array([0, 0, 1, 0], f32)).astype(f32)
    assert not with_probability or (np.isfinite(rad).all() and np.isfinite(dirn).all())  # (without the plane the samples of a lobe whose q was 0 count, NaN and all)
    return rad, dirn


def packed_diffuse_hit_dist(hit, viewz, mode_is_reblur, directional, hit_dist_params):
    """the fp32 hit-distance output of the mode's packer for the diffuse signal (roughness 1), sanitize = true, hit finite: REBLUR_FrontEnd_GetNormHitDist then the packer's
    saturate (directional occlusion: c0 of the SG, the luma of ( n, n, n )); RELAX: the clamp of its packer. exp2( D x 1 x 1 ) is a power of two for the integer D used."""
    hit, viewz = np.asarray(hit, f32), np.asarray(viewz, f32)
    if not mode_is_reblur:
        return np.minimum(np.maximum(hit, f32(0)), f32(M.NRD_FP16_MAX)).astype(f32)
    A, B, Cc, D = (f32(v) for v in hit_dist_params)
    assert float(D) == int(D)
    e = np.minimum(np.maximum(np.exp2(D * f32(1) * f32(1)), f32(0)), f32(1)).astype(f32)
    f = ((A + np.abs(viewz) * B).astype(f32) * (f32(1) + (Cc - f32(1)) * e).astype(f32)).astype(f32)
    nhd = np.minimum(np.maximum((hit / f).astype(f32), f32(0)), f32(1)).astype(f32)
    if directional:
        return ((nhd * f32(0.25) + nhd * f32(0.5)).astype(f32) + nhd * f32(0.25)).astype(f32)
    return nhd


def diffuse_hit_dist(s, mode_is_reblur, directional, hit_dist_params, viewz_scale=1.0, with_probability=True):
    """the diffuse hit-distance channel of nrdHipPackInputsLobes, fp32 [h, w], before the store codec: the sum, in sample order, of the packer's hit-distance output over the
    counted samples, divided by their number; 0 where there is none"""
    keep = counted(s["lobe"], s["prob"] if with_probability else None, DIFFUSE)
    z = (s["viewz"] * f32(viewz_scale)).astype(f32)
    total, num = np.zeros(z.shape, f32), np.zeros(z.shape, np.int32)
    for k in range(s["n"]):
        hit = np.where(keep[k], s["rad"][k, ..., 3], f32(0)).astype(f32)
        p = packed_diffuse_hit_dist(hit, z, mode_is_reblur, directional, hit_dist_params)
        total = np.where(keep[k], np.where(num == 0, p, (total + p).astype(f32)), total).astype(f32)
        num += keep[k]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(num > 0, (total / num.astype(f32)).astype(f32), f32(0)).astype(f32), num


def spec_hit_dist(hits):
    """NRD_FrontEnd_SpecHitDistAveraging_{Begin,Add,End} from their definitions (NRD.hlsli:693-716): the smallest non-zero sample, 0 if none; hits [n, ...] float32"""
    inf = f32(1e6)
    a = np.full(hits.shape[1:], inf, f32)
    for h in hits:
        a = np.fmin(a, np.where(h == 0, inf, h).astype(f32))
    return np.where(a == inf, f32(0), a).astype(f32)


def coverage_scene(planted=True, w=W, h=H, seed=5):
    """one sample per pixel, no probability plane, every traced hit distance well above 0: the plain 4 x 4 Bayer pattern at p = 0.5 (a checkerboard: both lobes in every 3x3
    area), and with `planted` the cases of tests/test_hit_dist_coverage.py -- (x, y) in PLANTED"""
    rng = np.random.RandomState(seed)
    unit = lambda shape: (lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32))(rng.normal(size=shape + (3,)))
    s = dict(n=1, w=w, h=h)
    s["nr"] = np.concatenate([unit((h, w)), rng.uniform(0.05, 1.0, (h, w, 1)).astype(f32)], -1)
    s["viewz"] = rng.uniform(1.0, 50.0, (h, w)).astype(f32)
    s["albedo"] = np.concatenate([rng.uniform(0.05, 1.0, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(f32)
    s["rf0"] = np.concatenate([rng.uniform(0.02, 0.9, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(f32)
    s["rad"] = np.concatenate([rng.uniform(0.0, 4.0, (1, h, w, 3)), rng.uniform(1.0, 30.0, (1, h, w, 1))], -1).astype(f32)
    s["dirn"] = np.concatenate([unit((1, h, w)), np.zeros((1, h, w, 1), f32)], -1)
    s["prob"] = np.full((1, h, w), 0.5, f32)
    lobe = bayer_lobes(h, w, 0.5)[None]
    if planted:
        P = PLANTED
        block = lambda c, r, v: lobe[0, c[1] - r:c[1] + r + 1, c[0] - r:c[0] + r + 1].__setitem__(Ellipsis, v)
        block(P["3x3 specular"], 1, SPECULAR)
        block(P["5x5 specular"], 2, SPECULAR)
        block(P["tile corner, 5x5 diffuse"], 2, DIFFUSE)
        lobe[0, 0:3, 0:3] = SPECULAR          # P["frame corner"]: the neighbours outside the plane are invalid
        lobe[0, h - 3:, w - 3:] = DIFFUSE     # P["far frame corner"]
        x, y = P["ring beyond the range"]     # a specular pixel whose eight neighbours are diffuse -- non-zero diffuse hit distances -- but beyond the denoising range
        lobe[0, y - 1:y + 2, x - 1:x + 2] = DIFFUSE
        lobe[0, y, x] = SPECULAR
        s["viewz"][y - 1:y + 2, x - 1:x + 2] = SKY_Z
        s["viewz"][y, x] = 10.0
        s["rad"][0, y - 1:y + 2, x - 1:x + 2, 3] = 30.0  # (far enough from 0 to stay non-zero once normalised with a sky depth and stored as UNORM16)
        x, y = P["sky"]                        # a sky pixel for which nothing was traced: hit distance 0 in both signals, and it must not count
        lobe[0, y, x] = NOTHING
        s["viewz"][y, x] = SKY_Z
    s["lobe"] = lobe
    return s


PLANTED = {"3x3 specular": (10, 12), "5x5 specular": (50, 14), "tile corner, 5x5 diffuse": (32, 8), "frame corner": (0, 0), "far frame corner": (W - 1, H - 1),
           "ring beyond the range": (40, 4), "sky": (60, 3)}


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------------------------
def decoded_hit_dist(plane):
    """the hit-distance channel of a packed plane as the passes decode it: .w of float16 / SNORM16 [h, w, 4], the channel of UNORM16 [h, w] (held as int16)"""
    if plane.dtype == np.float16:
        return plane[..., 3].astype(f32)
    if plane.ndim == 3:
        return np.maximum(plane[..., 3].astype(f32) / f32(32767), f32(-1))
    return plane.view(np.uint16).astype(f32) / f32(65535)


def coverage(viewz, diffuse=None, specular=None, area=1, viewz_scale=1.0, denoising_range=DENOISING_RANGE):
    """the report of nrdHipCheckHitDistCoverage as a dict, from a stencil over padded arrays: a neighbour outside the plane is invalid"""
    h, w = viewz.shape
    with np.errstate(invalid="ignore", over="ignore"):
        in_range = np.isfinite(viewz) & ~(np.abs(viewz * f32(viewz_scale)) > f32(denoising_range))
    out = dict(inRangePixels=int(in_range.sum()), empty=[0, 0], holes=[0, 0], firstHole=[0xFFFFFFFF, 0xFFFFFFFF], masks=[None, None])  # masks: [h, w] bool, the holes
    for i, plane in enumerate((diffuse, specular)):
        if plane is None:
            continue
        nonzero = decoded_hit_dist(plane) != 0  # (true for a NaN)
        valid = np.zeros((h + 2 * area, w + 2 * area), bool)
        valid[area:area + h, area:area + w] = in_range & nonzero
        any_valid = np.zeros((h, w), bool)
        for dy in range(2 * area + 1):
            for dx in range(2 * area + 1):
                any_valid |= valid[dy:dy + h, dx:dx + w]
        empty = in_range & ~nonzero
        holes = empty & ~any_valid
        out["empty"][i], out["holes"][i], out["masks"][i] = int(empty.sum()), int(holes.sum()), holes
        if holes.any():
            out["firstHole"][i] = int(np.flatnonzero(holes)[0])
    return out
