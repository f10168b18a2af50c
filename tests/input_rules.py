"""Shapes generated frames into what NRD's input rules ALLOW a host to hand over, and nothing beyond that. The reference's README, "NOISY & NON-NOISY DATA REQUIREMENTS",
gives a host these freedoms (and the helpers below use exactly these):

    Noisy inputs:
     - garbage values are allowed outside of active viewport, i.e. `pixelPos >= CommonSettings::rectSize`
     - garbage values are allowed outside of denoising range, i.e. `abs( viewZ ) >= CommonSettings::denoisingRange`
    Non-noisy inputs (guides):
     - must not contain `NAN/INF` values
    Where "garbage" is `NAN/INF` or undesired value.

Nothing there says that the guides (IN_MV, IN_NORMAL_ROUGHNESS, the confidences, the mix, IN_BASECOLOR_METALNESS) are CLEAN on the sky -- zero motion, a fixed normal --, only
that they are finite.

So: NaN / INF only ever go into NOISY planes, and only beyond the denoising range or outside the rect; guides only ever receive finite values. A case that feeds a NaN guide,
or garbage inside the range and the rect, tests nothing the library promises -- what comes out of it is not a finding.

Every helper works in place on a frame of raytracingdenoiser_amd.synth.render_frame (a dict of planes), in the style of tests/test_tile_exit.py::_shape_sky. This is a helper
module, not a conftest: tests import it."""
import torch

import parity
from raytracingdenoiser_amd import synth
from raytracingdenoiser_amd.scene import embed_in_resource

KINDS = ("finite", "nan", "inf", "neg_inf", "mixed")
# the noisy planes of scene.user_planes by frame key: radiance / SH0 + hit distance, SH1, direction + hit distance, penumbra, translucency, RELAX's packed signals
NOISY = ("diff", "spec", "diff_sh1", "spec_sh1", "diff_direction_hitdist", "penumbra", "translucency", "diff_relax", "spec_relax", "diff_relax_sh1", "spec_relax_sh1")
# every guide but viewZ (which DEFINES the sky and stays as it is)
GUIDES = ("mv", "normal_roughness", "diff_confidence", "spec_confidence", "disocclusion_mix", "basecolor_metalness")
OCCLUSION = ("REBLUR_DIFFUSE_OCCLUSION", "REBLUR_SPECULAR_OCCLUSION", "REBLUR_DIFFUSE_SPECULAR_OCCLUSION")

_FLOAT = {"finite": 3.0, "nan": float("nan"), "inf": float("inf"), "neg_inf": float("-inf")}
_MIXED_FLOAT = (3.0, float("nan"), float("inf"), float("-inf"), synth.FP16_MAX)
# formats that cannot hold a NaN get their extreme codes: SNORM16 0x7FFF (0x8001 for "neg_inf"), UNORM8 0xFF
_SNORM16 = {"finite": 0x7FFF, "nan": 0x7FFF, "inf": 0x7FFF, "neg_inf": -0x7FFF}
_MIXED_SNORM16 = (0x7FFF, -0x8000, -0x7FFF, 0x1234, 0)
_MIXED_UNORM8 = (0xFF, 0x00, 0x80, 0x5D, 0x01)


def sky_mask(frame):
    """texels beyond the denoising range (scene.common_settings leaves CommonSettings::denoisingRange at its default, 5e5 = 0.5 * SKY_VIEWZ)"""
    return frame["viewz"].abs() >= 0.5 * synth.SKY_VIEWZ


def _garbage(plane, kind, salt):
    """a tensor of plane's shape and dtype full of `kind`; "mixed": a hash of (x, y, channel, salt) picks the value of every component"""
    assert kind in KINDS, kind
    if kind != "mixed":
        if plane.dtype.is_floating_point:
            value = _FLOAT[kind]
        elif plane.dtype == torch.int16:
            value = _SNORM16[kind]
        else:
            assert plane.dtype == torch.uint8, plane.dtype
            value = 0xFF
        return torch.full_like(plane, value)
    h, w = plane.shape[:2]
    ch = plane.shape[2] if plane.dim() > 2 else 1
    y, x, c = torch.meshgrid(torch.arange(h, dtype=torch.int64), torch.arange(w, dtype=torch.int64), torch.arange(ch, dtype=torch.int64), indexing="ij")
    pick = (synth._hash_uniform(x, y, c, 101 + salt) * 5.0).to(torch.int64).clamp(0, 4)
    table = _MIXED_FLOAT if plane.dtype.is_floating_point else (_MIXED_SNORM16 if plane.dtype == torch.int16 else _MIXED_UNORM8)
    return torch.tensor(table, dtype=plane.dtype)[pick].reshape(plane.shape).to(plane.device)


def _fill(frame, key, where, kind, salt, name):
    plane = frame[key]
    g = _garbage(plane, kind, salt)
    if name in OCCLUSION and key in ("diff", "spec"):
        # the occlusion family's R16_UNORM input is packed from .w of this plane (scene._hitdist_unorm16): UNORM16 cannot hold a NaN -- it gets 0xFFFF, which +INF packs to
        g[..., 3] = torch.where(torch.isnan(g[..., 3]), torch.full_like(g[..., 3], float("inf")), g[..., 3])
    m = where if plane.dim() == 2 else where.unsqueeze(-1)
    frame[key] = torch.where(m, g, plane).contiguous()


def dirty_sky_noisy(frame, kind, f=0, name=None):
    """garbage of `kind` in every noisy plane wherever viewZ is beyond the denoising range (README: allowed, NaN / INF included). name: the denoiser the frame is for
    (only the occlusion family needs it: see _fill)"""
    sky = sky_mask(frame)
    for k, key in enumerate(NOISY):
        if key in frame:
            _fill(frame, key, sky, kind, 16 * f + k, name)


def dirty_sky_guides(frame):
    """finite arbitrary values in every guide but viewZ on the sky texels: float planes 3.0, integer planes (packed normals, UNORM8 guides) 93. Guides stay finite (README)."""
    sky = sky_mask(frame)
    for key in GUIDES:
        if key in frame:
            plane = frame[key]
            m = sky if plane.dim() == 2 else sky.unsqueeze(-1)
            frame[key] = torch.where(m, torch.full_like(plane, 3.0 if plane.dtype.is_floating_point else 93), plane).contiguous()


def paint_sky(frame, f, moving):
    """a slanted horizon y < 0.3 h + 0.13 x (+ 3 f: three rows lower every frame), made by viewZ ALONE: every other plane keeps what the renderer put there -- a geometry
    normal, roughness, signal and hit distance on texels that are sky now (a renderer that writes the far plane's depth where a ray left the scene and clears nothing else)"""
    viewz = frame["viewz"]
    h, w = viewz.shape
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    now_sky = y < 0.3 * h + 0.13 * x + (3.0 * f if moving else 0.0)
    frame["viewz"] = torch.where(now_sky, torch.full_like(viewz, synth.SKY_VIEWZ), viewz).contiguous()


def embed_in_resource_dirty(frame, resource, kind, f=0):
    """scene.embed_in_resource with the noisy planes' fill outside the rect set to `kind` (README: allowed); the guides keep the finite sentinel 33 / 9"""
    h, w = frame["viewz"].shape
    out = embed_in_resource(frame, resource)
    rw, rh = resource
    y, x = torch.meshgrid(torch.arange(rh), torch.arange(rw), indexing="ij")
    outside = (x >= w) | (y >= h)
    for k, key in enumerate(NOISY):
        if key in out:
            _fill(out, key, outside, kind, 16 * f + k + 7, None)
    return out


def shaped(monkeypatch, shape=None, embed=None):
    """parity.run_parity / ref_parity.run_per_pass then see shaped frames: shape(name, frame, f) works in place on every frame of parity.generate_sequence
    (not on the frames of a rect_sizes sequence, which these functions render themselves); embed(frame, resource, f) replaces scene.embed_in_resource"""
    gen = parity.generate_sequence

    def generate(name, width, height, frames, **kw):
        seq = gen(name, width, height, frames, **kw)
        for f, frame in enumerate(seq):
            shape(name, frame, f)
        return seq

    if shape is not None:
        monkeypatch.setattr(parity, "generate_sequence", generate)
    if embed is not None:
        count = [0]

        def embed_counted(frame, resource):  # (called once per frame, in frame order)
            count[0] += 1
            return embed(frame, resource, count[0] - 1)

        monkeypatch.setattr(parity, "embed_in_resource", embed_counted)
