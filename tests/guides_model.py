"""TEST INFRASTRUCTURE. nrdHipPackGuides (include/NRDHip.h) restated twice, from the header text alone:
  pack()     float32 numpy, every intermediate np.float32, the operations in the header's order: reproduces every byte
  exact()    float64 from the raw matrices (worldToClip = viewToClip . worldToView as 4 x 4 products, no camera-relative step): what the stored values approximate
Matrices are CommonSettings' column-major float[16]."""
import numpy as np

f32 = np.float32
FP16_MAX = f32(65504.0)


def _m(col_major):
    """M[i][j] = row i, column j"""
    return np.asarray(list(col_major), f32).reshape(4, 4).T.copy()


def camera(world_to_view, view_to_clip):
    """(R rows, c, P) as the host side of the call derives them: c = -( ( R[0][i] * t.x + R[1][i] * t.y ) + R[2][i] * t.z )"""
    W, P = _m(world_to_view), _m(view_to_clip)
    R, t = W[:3, :3].copy(), W[:3, 3].copy()
    c = np.array([-f32(f32(f32(R[0, i] * t[0]) + f32(R[1, i] * t[1])) + f32(R[2, i] * t[2])) for i in range(3)], f32)
    return R, c, P


def _dot3(a, x, y, z):
    return ((a[0] * x).astype(f32) + (a[1] * y).astype(f32)).astype(f32) + (a[2] * z).astype(f32)


def to_view(R, c, X):
    dx, dy, dz = (X[..., 0] - c[0]).astype(f32), (X[..., 1] - c[1]).astype(f32), (X[..., 2] - c[2]).astype(f32)
    return [_dot3(R[i], dx, dy, dz).astype(f32) for i in range(3)]


def screen_uv(P, Xv):
    with np.errstate(all="ignore"):
        clip = {k: (_dot3(P[k], Xv[0], Xv[1], Xv[2]).astype(f32) + P[k, 3]).astype(f32) for k in (0, 1, 3)}
        u = ((clip[0] / clip[3]).astype(f32) * f32(0.5)).astype(f32) + f32(0.5)
        v = ((clip[1] / clip[3]).astype(f32) * f32(-0.5)).astype(f32) + f32(0.5)
    behind = clip[3] < 0
    return np.where(behind, f32(99999.0), u).astype(f32), np.where(behind, f32(99999.0), v).astype(f32)


def _div_or_zero(a, s):
    with np.errstate(all="ignore"):
        return (a / f32(s)).astype(f32) if f32(s) != 0 else np.zeros_like(a, f32)


def _store_range(v):
    """what goes into the fp16 conversion: a NaN becomes 0, then the clamp"""
    v = np.where(np.isnan(v), f32(0), v).astype(f32)
    return np.clip(v, -FP16_MAX, FP16_MAX).astype(f32)


def pack(cs, position, position_prev=None, miss_viewz=1e6):
    """(outViewZ float32 [H, W], outMv float32 [H, W, 4] in front of the fp16 store) for an api.CommonSettings and float32 [H, W, >= 3] positions"""
    with np.errstate(all="ignore"):
        X = np.asarray(position, f32)[..., :3]
        R, c, P = camera(cs.worldToViewMatrix, cs.viewToClipMatrix)
        Rp, cp, Pp = camera(cs.worldToViewMatrixPrev, cs.viewToClipMatrixPrev)
        s = [f32(v) for v in cs.motionVectorScale]
        hit = np.isfinite(X).all(-1)
        Xp = X
        if position_prev is not None:
            prev = np.asarray(position_prev, f32)[..., :3]
            Xp = np.where(np.isfinite(prev).all(-1)[..., None], prev, X)
        Xv = to_view(R, c, X)
        if cs.isMotionVectorInWorldSpace:
            mv = [_div_or_zero((Xp[..., i] - X[..., i]).astype(f32), s[i]) for i in range(3)]
        else:
            Xvp = to_view(Rp, cp, Xp)
            (u, v), (up, vp) = screen_uv(P, Xv), screen_uv(Pp, Xvp)
            mv = [((up - u).astype(f32) / s[0]).astype(f32), ((vp - v).astype(f32) / s[1]).astype(f32), _div_or_zero((np.abs(Xvp[2]) - np.abs(Xv[2])).astype(f32), s[2])]
        out_mv = np.stack([_store_range(m) for m in mv] + [np.zeros(hit.shape, f32)], -1)
        out_mv[~hit] = 0
        return np.where(hit, Xv[2], f32(miss_viewz)).astype(f32), out_mv


def exact(cs, position, position_prev=None):
    """float64: (viewZ, mv [H, W, 3] as stored before the fp16 rounding) at finite positions, from worldToClip = viewToClip . worldToView of each frame. The depth the passes
    work with (abs( IN_VIEWZ )) is taken from clip.w here, not from an absolute value of view z: another route than pack()'s to the same number"""
    with np.errstate(all="ignore"):
        X = np.asarray(position, np.float64)[..., :3]
        Xp = X
        if position_prev is not None:
            prev = np.asarray(position_prev, np.float64)[..., :3]
            Xp = np.where(np.isfinite(prev).all(-1)[..., None], prev, X)
        s = [float(v) for v in cs.motionVectorScale]
        out = []
        for w2v, v2c, pts in ((cs.worldToViewMatrix, cs.viewToClipMatrix, X), (cs.worldToViewMatrixPrev, cs.viewToClipMatrixPrev, Xp)):
            W, P = _m(w2v).astype(np.float64), _m(v2c).astype(np.float64)
            h = np.concatenate([pts, np.ones(pts.shape[:-1] + (1,))], -1)
            view = h @ W.T
            clip = h @ (P @ W).T
            uv = np.stack([clip[..., 0] / clip[..., 3] * 0.5 + 0.5, clip[..., 1] / clip[..., 3] * -0.5 + 0.5], -1)
            uv = np.where((clip[..., 3] < 0)[..., None], 99999.0, uv)
            out.append((view[..., 2], uv, clip[..., 3] / abs(P[3, 2])))  # (a perspective projection: clip.w = +-P[3][2] * view z, positive in front of the camera)
        (z, uv, depth), (zp, uvp, depth_p) = out
        if cs.isMotionVectorInWorldSpace:
            mv = np.stack([(Xp[..., i] - X[..., i]) / s[i] if s[i] != 0 else np.zeros(z.shape) for i in range(3)], -1)
        else:
            mv = np.stack([(uvp[..., 0] - uv[..., 0]) / s[0], (uvp[..., 1] - uv[..., 1]) / s[1], (depth_p - depth) / s[2] if s[2] != 0 else np.zeros(z.shape)], -1)
        return z, mv
