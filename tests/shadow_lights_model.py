"""float32 numpy restatement of what nrdHipPackShadowLights / nrdHipResolveShadowLights compute (include/NRDHip.h), from the definitions of the three SIGMA front-end
functions and SIGMA_BackEnd_UnpackShadow in NRD.hlsli:828-855, 931 and the README's recipe for several lights. Only + - * / min max and selects, every intermediate np.float32,
in the order the header states: the kernels are held to these values bit for bit. Nothing here calls the library."""
import numpy as np

f32 = np.float32
FP16_MAX, EPS = f32(65504.0), f32(1e-6)
DIRECTIONAL, LOCAL = 0, 1


def _f(a):
    a = np.asarray(a)
    assert a.dtype == f32, a.dtype
    return a


def penumbra(light, d, dl=None):
    """SIGMA_FrontEnd_PackPenumbra of one light = (type, tanOfLightAngularRadius or lightSize): the directional or the local-light overload"""
    kind, value = light
    d = _f(d)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == LOCAL:
            size = _f(_f(f32(value) * d) / np.maximum(_f(_f(dl) - d), EPS))
        else:
            size = _f(d * f32(value))
        radius = _f(size * f32(0.5))
    return np.where(d >= FP16_MAX, FP16_MAX, np.minimum(radius, f32(32768.0))).astype(f32)


def pack_translucency(d, t):
    """SIGMA_FrontEnd_PackTranslucency: [.., 4] = ( d >= NRD_FP16_MAX ? 1 : 0, saturate( t.rgb ) )"""
    t = np.minimum(np.maximum(_f(t)[..., :3], f32(0)), f32(1))
    return np.concatenate([np.where(_f(d) >= FP16_MAX, f32(1), f32(0))[..., None].astype(f32), t], axis=-1).astype(f32)


def luminance(c):
    c = _f(c)
    return _f(_f(_f(c[..., 0] * f32(0.2126)) + _f(c[..., 1] * f32(0.7152))) + _f(c[..., 2] * f32(0.0722)))


def combined(lights, d, dl, lighting, weight=None):
    """the COMBINED pack: (penumbra [H, W], translucency [H, W, 4], Lsum [H, W, 3]) before the store codecs. d, dl, weight: [N, H, W]; lighting: [N, H, W, 3 or 4]"""
    shape = d.shape[1:]
    Lsum, LSsum = np.zeros(shape + (3,), f32), np.zeros(shape + (3,), f32)
    Wsum, Psum, dmin = np.zeros(shape, f32), np.zeros(shape, f32), np.full(shape, np.inf, f32)
    for i, light in enumerate(lights):
        L = _f(lighting[i])[..., :3]
        Lsum = _f(Lsum + L)
        lit = _f(d[i]) >= FP16_MAX
        shadow = np.where(lit, f32(1), f32(0)).astype(f32)
        LSsum = _f(LSsum + _f(L * shadow[..., None]))
        w = _f((np.where(lit, f32(0), f32(1)).astype(f32) if weight is None else _f(weight[i])) * luminance(L))
        Wsum = _f(Wsum + w)
        Psum = _f(Psum + _f(penumbra(light, d[i], None if dl is None else dl[i]) * w))
        dmin = np.minimum(dmin, d[i])
    translucency = _f(LSsum / np.maximum(Lsum, EPS))
    p = np.where(dmin >= FP16_MAX, FP16_MAX, _f(Psum / np.maximum(Wsum, EPS))).astype(f32)
    return p, pack_translucency(dmin, translucency), Lsum


def unpack_shadow(codes):
    """SIGMA_BackEnd_UnpackShadow of UNORM8 texels: ( k / 255 )^2"""
    s = _f(np.asarray(codes, np.uint8).astype(f32) / f32(255))
    return _f(s * s)


def resolve_combined(shadow_rgba8, lsum):
    """[H, W, 4]: Lsum.rgb * s.yzw, s.x"""
    s = unpack_shadow(shadow_rgba8)
    return np.concatenate([_f(_f(lsum)[..., :3] * s[..., 1:]), s[..., :1]], axis=-1).astype(f32)


def resolve_per_light(shadows, lighting):
    """[H, W, 4]: acc = 0; acc = acc + L_i * s_i in order; .w = 0. shadows: [N, H, W] (scalar s_i) or [N, H, W, 4] (s_i = .yzw)"""
    acc = np.zeros(lighting.shape[1:3] + (3,), f32)
    for i in range(lighting.shape[0]):
        s = unpack_shadow(shadows[i])
        s = s[..., None] if s.ndim == 2 else s[..., 1:]
        acc = _f(acc + _f(_f(lighting[i])[..., :3] * s))
    return np.concatenate([acc, np.zeros(acc.shape[:2] + (1,), f32)], axis=-1).astype(f32)
