"""A float32 numpy restatement of the rules nrdHipPackInputsDirect adds to the front end (include/NRDHip.h, "Combined denoising of direct and indirect lighting"), written from
the text of the header comment and of NRD_HIP_MixDiffuseHitDist and from nothing else: one numpy operation per fp32 operation, in the order the text gives, so that results can be
compared bit for bit. Nothing here calls the code under test."""
import numpy as np

f32 = np.float32
NRD_FP16_MAX = f32(65504.0)
NRD_EPS = f32(1e-6)
LUMA = (f32(0.2126), f32(0.7152), f32(0.0722))


def _f(a):
    a = np.asarray(a, f32)
    assert a.dtype == f32
    return a


def san(radiance):
    """the packers' own first line: _NRD_IsInvalid( r ) ? 0 : clamp( r, 0, NRD_FP16_MAX ) -- one invalid channel zeroes the texel"""
    r = _f(radiance)
    with np.errstate(invalid="ignore"):
        clamped = np.minimum(np.maximum(r, f32(0)), NRD_FP16_MAX)
    return np.where(np.isfinite(r).all(-1, keepdims=True), clamped, f32(0)).astype(f32)


def luminance(radiance):
    """_NRD_Luminance: dot( c, ( 0.2126, 0.7152, 0.0722 ) ) = ( c.x * k.x + c.y * k.y ) + c.z * k.z"""
    r = _f(radiance)
    return ((r[..., 0] * LUMA[0] + r[..., 1] * LUMA[1]) + r[..., 2] * LUMA[2]).astype(f32)


def weight(lum_indirect, lum_direct, max_contribution):
    """c of NRD_HIP_MixDiffuseHitDist: L_d / ( ( L_d + L_i ) + NRD_EPS ), capped; a NaN c, or c <= 0, counts as 0"""
    li, ld = _f(lum_indirect), _f(lum_direct)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (ld / ((ld + li) + NRD_EPS)).astype(f32)
        return np.where(c > 0, np.fmin(c, f32(max_contribution)), f32(0)).astype(f32)


def is_mixed(h_indirect, h_direct, c):
    hi, hd = _f(h_indirect), _f(h_direct)
    with np.errstate(invalid="ignore"):
        return (c > 0) & np.isfinite(hi) & (hi > 0) & np.isfinite(hd) & (hd > 0)


def mix_diffuse_hit_dist(h_indirect, h_direct, lum_indirect, lum_direct, max_contribution):
    """NRD_HIP_MixDiffuseHitDist: lerp( h_i, h_d, c ) = h_i + ( h_d - h_i ) * c where both are finite and above 0 and c > 0, else h_i as it is"""
    hi, hd = _f(h_indirect), _f(h_direct)
    c = weight(lum_indirect, lum_direct, max_contribution)
    with np.errstate(invalid="ignore", over="ignore"):
        lerp = (hi + (hd - hi) * c).astype(f32)
    return np.where(is_mixed(hi, hd, c), lerp, hi).astype(f32)


def clamp_half(a):
    """clamp( v, -NRD_FP16_MAX, NRD_FP16_MAX )"""
    return np.minimum(np.maximum(_f(a), -NRD_FP16_MAX), NRD_FP16_MAX).astype(f32)


def combine_per_sample(packed_indirect, packed_direct):
    """N direct layers: ( ( C_0 + C_1 ) + ... ) / float( N ) with C_s = clamp( P_i,s + P_d,s ) -- lists of N float32 arrays each"""
    assert len(packed_indirect) == len(packed_direct)
    acc = None
    for pi, pd in zip(packed_indirect, packed_direct):
        c = clamp_half(_f(pi) + _f(pd))
        acc = c if acc is None else (acc + c).astype(f32)
    return (acc / f32(len(packed_indirect))).astype(f32)


def combine_one_direct_layer(packed_indirect, packed_direct):
    """one direct layer under N samples: clamp( mean_s( P_i,s ) + P_d ), the mean ( ( P_0 + P_1 ) + ... ) / float( N )"""
    acc = _f(packed_indirect[0])
    for p in packed_indirect[1:]:
        acc = (acc + _f(p)).astype(f32)
    mean = (acc / f32(len(packed_indirect))).astype(f32)
    return clamp_half(mean + _f(packed_direct))


def mean_of(parts):
    """( ( v_0 + v_1 ) + ... ) / float( N ): the diffuse hit-distance channel, the mean of the packed per-sample values"""
    acc = _f(parts[0])
    for p in parts[1:]:
        acc = (acc + _f(p)).astype(f32)
    return (acc / f32(len(parts))).astype(f32)


def relax_packed_hit_dist(h):
    """the hit-distance output of RELAX's packers with sanitize = true: isInvalid( h ) ? 0 : clamp( h, 0, NRD_FP16_MAX )"""
    h = _f(h)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(h), np.minimum(np.maximum(h, f32(0)), NRD_FP16_MAX), f32(0)).astype(f32)


# the edge cases of NRD_HIP_MixDiffuseHitDist ( h_i, h_d, L_i, L_d, maxContribution ): tests/cpp/pack_direct_integration.cpp evaluates the header's function on these very rows
def edge_table():
    nan, inf = np.nan, np.inf
    rows = []
    for maxc in (0.0, 0.5, 0.65, 1.0):
        rows += [
            (2.0, 10.0, 1.0, 1.0, maxc),       # c = 0.5 - eps: below / at the cap
            (2.0, 10.0, 0.25, 4.0, maxc),      # c above 0.5 and 0.65: capped
            (10.0, 2.0, 3.0, 0.125, maxc),     # c small, the direct distance shorter
            (2.0, 10.0, 1.0, 0.0, maxc),       # L_d = 0
            (2.0, 10.0, 0.0, 0.0, maxc),       # both zero: 0 / eps
            (2.0, 10.0, 0.0, 5.0, maxc),       # L_i = 0: c close to 1
            (0.0, 10.0, 1.0, 1.0, maxc),       # h_i = 0 stays 0
            (-0.0, 10.0, 1.0, 1.0, maxc),      # ... and -0 stays -0
            (-1.0, 10.0, 1.0, 1.0, maxc),      # a negative h_i is not valid: kept
            (nan, 10.0, 1.0, 1.0, maxc), (inf, 10.0, 1.0, 1.0, maxc),
            (2.0, nan, 1.0, 1.0, maxc), (2.0, 0.0, 1.0, 1.0, maxc), (2.0, inf, 1.0, 1.0, maxc), (2.0, -3.0, 1.0, 1.0, maxc),
            (2.0, 10.0, nan, 1.0, maxc), (2.0, 10.0, 1.0, nan, maxc), (2.0, 10.0, 1.0, inf, maxc), (2.0, 10.0, inf, 1.0, maxc),  # NaN / inf weights
            (2.0, 10.0, 1.0, -1.0, maxc),      # c < 0
            (3e38, 1.0, 1.0, 3.0, maxc), (1e-40, 1e-38, 65504.0, 65504.0, maxc), (29.999996, 5.00679e-05, 1e-6, 1e-6, maxc)]
    return np.array(rows, f32)
