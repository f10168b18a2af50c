"""The workgroup-uniform tile test (csrc/hip/planes.h LoadTileBytesUniform): every full-frame kernel reads the bytes of the 16x16 tiles under its workgroup through the scalar
cache and leaves, when all of them are sky, before it has issued a vector-memory or LDS instruction; the lanes of a workgroup that stays take their own tile's byte from the
same scalar value. What this file holds:
  * device == oracle, bit for bit, on every output and pool plane, for frames chosen for the tile test (all sky, no sky, a slanted horizon that cuts through 16x16 tiles and
    32x8 workgroups and moves from frame to frame, tile planes that are not a multiple of 4 tiles wide with partial last tiles, 33x9 and 1x1, a dynamic-resolution rect inside
    a larger resource, row strips);
  * the split TemporalAccumulation pass (window kernel + fallback kernel behind a scalar flag scan) with tiles on both paths and a frame on which every tile flagged before is sky;
  * the property the change exists for, on the ISA of the benchmarked kernels: no vector-memory or LDS instruction in front of the sky exit (a CPU test: it only compiles)."""
import os
import re
import subprocess
import sys

import pytest
import torch

import parity
from raytracingdenoiser_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENOISERS = ["REBLUR_DIFFUSE_SPECULAR", "RELAX_DIFFUSE_SPECULAR_SH", "SIGMA_SHADOW"]
SKY_FRAME = 2  # "flash": the frame on which everything is sky


def _shape_sky(frame, mode, f):
    """lays the sky of a rendered frame out for the case, in place. Sky = viewZ beyond the denoising range (all the tile classification looks at). A pixel that BECOMES sky takes
    the values of a rendered sky pixel in every other plane too (zero signal and motion, the renderer's sky normal, ...), and rendered sky that becomes geometry is what
    "no_sky" is for: a far wall that keeps the rendered sky's planes. (Sky pixels that carry a signal, a geometry normal or garbage are another matter than the tile test: tests/test_input_rules.py
    holds the library on them -- a sky painted by viewZ alone, NaN / INF in the noisy inputs beyond the range, arbitrary finite guides.)"""
    viewz = frame["viewz"]
    h, w = viewz.shape
    if mode == "default" or (mode == "flash" and f != SKY_FRAME):
        return
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    was_sky = viewz >= 0.5 * synth.SKY_VIEWZ
    if mode in ("all_sky", "flash"):
        now_sky = torch.ones_like(was_sky)
    elif mode == "no_sky":
        now_sky = torch.zeros_like(was_sky)
    else:
        assert mode in ("horizon", "moving_horizon")
        # slanted: it crosses the tile and workgroup columns at every height of a tile. moving_horizon: 3 rows lower every frame (tiles with geometry, and history, turn into sky)
        now_sky = y < 0.3 * h + 0.13 * x + (3.0 * f if mode == "moving_horizon" else 0.0)
    becomes_sky = now_sky & ~was_sky
    if bool(becomes_sky.any()):
        src = torch.nonzero(was_sky)
        for k, v in frame.items():
            if torch.is_tensor(v) and v.dim() >= 2 and tuple(v.shape[:2]) == (h, w) and k != "viewz":
                v = v.clone()
                v[becomes_sky] = v[src[0, 0], src[0, 1]].clone() if len(src) else torch.zeros_like(v[0, 0])
                frame[k] = v.contiguous()
    solid = 30.0 + 0.05 * x + 0.11 * y  # the far wall in place of rendered sky
    frame["viewz"] = torch.where(now_sky, torch.full_like(viewz, synth.SKY_VIEWZ), torch.where(was_sky, solid, viewz)).contiguous()


def _shaped(monkeypatch, mode):
    orig = parity.generate_sequence

    def generate(name, width, height, frames, **kw):
        seq = orig(name, width, height, frames, **kw)
        for f, frame in enumerate(seq):
            _shape_sky(frame, mode, f)
        return seq

    monkeypatch.setattr(parity, "generate_sequence", generate)


CASES = [
    # tag, sky layout, (width, height), frames, run_parity keywords
    ("all_sky", "all_sky", (192, 128), 3, {}),
    ("no_sky", "no_sky", (192, 128), 3, {}),
    ("horizon", "horizon", (256, 160), 4, {}),
    ("moving_horizon", "moving_horizon", (256, 160), 4, {}),
    ("tiles_63x38_partial", "horizon", (1000, 600), 3, {}),  # 63 tile columns (not a multiple of 4), 32 workgroup columns of which the last covers ONE tile; partial last tiles
    ("33x9", "horizon", (33, 9), 3, {}),
    ("33x9_default_sky", "default", (33, 9), 3, {}),
    ("1x1", "no_sky", (1, 1), 3, {}),
    ("1x1_sky", "all_sky", (1, 1), 3, {}),
    ("rect_in_resource", "horizon", (176, 104), 4, dict(resource=(256, 160))),  # the tiles beyond the rect are classified from the sentinel around it: geometry
]


@pytest.mark.gpu
@pytest.mark.parametrize("name", DENOISERS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_oracle_on_frames_chosen_for_the_tile_test(monkeypatch, name, case):
    tag, mode, (w, h), frames, kw = case
    _shaped(monkeypatch, mode)
    worst = parity.run_parity(name, width=w, height=h, frames=frames, **kw)
    print("%s %s %dx%d: worst relative error %g" % (name, tag, w, h, worst))
    assert worst == 0.0, (name, tag, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,overrides", [
    ("REBLUR_DIFFUSE_SPECULAR", dict(maxBlurRadius=4.0, diffusePrepassBlurRadius=6.0, specularPrepassBlurRadius=6.0)),
    ("RELAX_DIFFUSE_SPECULAR_SH", dict(atrousIterationNum=4)),
    ("SIGMA_SHADOW", None),
])
def test_sharding_into_row_strips_with_a_moving_horizon_reproduces_the_whole_frame(name, overrides):
    """three virtual ranks, each producing its row strip (+ the margins its later passes need) of the horizon frames; after the all-gather every plane equals the uncut run's --
    which the test above holds against the oracle. The workgroups of a strip's first and last tile rows lie partly outside the rows they have to produce."""
    from raytracingdenoiser_amd import sharding
    from raytracingdenoiser_amd.executor import HipExecutor

    W, H, frames, world = 256, 288, 4, 3
    RT = api.ResourceType
    seq = parity.generate_sequence(name, W, H, frames)
    for f, frame in enumerate(seq):
        _shape_sky(frame, "moving_horizon", f)

    def make_run():
        inst = api.Instance([(0, parity.DENOISERS[name][0])])
        ex = HipExecutor(inst, W, H)
        outs = []
        for rt, dtype, ch, fmt in parity.output_planes(name, W, H):
            outs.append(torch.zeros((H, W, ch), dtype=dtype, device="cuda"))
            ex.bind(rt, outs[-1], fmt)
        return inst, ex, outs

    ref_inst, ref_ex, ref_outs = make_run()
    ranks = []
    for r in range(world):
        inst, ex, outs = make_run()
        ranks.append((inst, ex, outs, sharding.FrameSharder(ex, inst, W, H, r, world, outs)))
    assert all(s.rows is not None for *_, s in ranks)
    for f, frame in enumerate(seq):
        def step(inst, ex):
            for rt, t, fmt in parity.user_planes(name, frame):
                ex.bind(rt, t.cuda().contiguous(), fmt)
            inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame, overrides))
            assert inst.set_common_settings(parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], W, H, f)) == api.Result.SUCCESS
            ex.denoise()

        step(ref_inst, ref_ex)
        for inst, ex, outs, s in ranks:
            step(inst, ex)
        for _, _, _, src in ranks:  # the all-gather: every rank's owned strip goes to all the others
            rb, re_ = src.rows
            for _, _, _, dst in ranks:
                if dst is not src:
                    for ps, pd in zip(src.planes, dst.planes):
                        pd[rb:re_].copy_(ps[rb:re_])
        torch.cuda.synchronize()
        ref_planes = ([ref_ex.pool_plane_tensor(RT.PERMANENT_POOL, i) for i, (_, ds) in enumerate(ref_inst.permanent_pool) if ds == 1]
                      + [o.view(-1).view(dtype=torch.uint8).view(H, -1) for o in ref_outs]
                      + [ref_ex.pool_plane_tensor(RT.TRANSIENT_POOL, i) for i, (_, ds) in enumerate(ref_inst.transient_pool) if ds == 1])
        assert len(ref_planes) == len(ranks[0][3].planes)
        for r, (_, _, _, s) in enumerate(ranks):
            for k, (a, b) in enumerate(zip(s.planes, ref_planes)):
                assert torch.equal(a, b), "frame %d rank %d plane %d differs from the uncut run" % (f, r, k)


def run_flash_case(name, width, height, frames):
    """(runs in a subprocess of the test below: NRD_HIP_TA_WINDOW_LIMIT is read once per process) -- prints run_parity's per-frame fallback statistics and the worst error"""
    orig = parity.generate_sequence

    def generate(n, w, h, fr, **kw):
        seq = orig(n, w, h, fr, **kw)
        for f, frame in enumerate(seq):
            _shape_sky(frame, "flash", f)
        return seq

    parity.generate_sequence = generate
    print("worst", parity.run_parity(name, width=width, height=height, frames=frames, verbose=True))


@pytest.mark.gpu
def test_window_and_fallback_kernels_with_flagged_tiles_that_turn_into_sky():
    """NRD_HIP_TA_WINDOW_LIMIT=35x11 leaves a good part of the tiles of every frame to the fallback kernel (both TA kernels have tiles). On frame SKY_FRAME every pixel is sky:
    each tile flagged on the frame before is sky now -- it must neither be run nor be counted, and the frame after it (history restarts over the whole frame) is back on
    both paths. All outputs and pool planes equal the oracle's on every frame."""
    name, w, h, frames = "REBLUR_DIFFUSE_SPECULAR", 256, 160, 5
    code = "import sys; sys.path[:0] = [%r, %r]; import test_tile_exit; test_tile_exit.run_flash_case(%r, %d, %d, %d)" % (ROOT, os.path.join(ROOT, "tests"), name, w, h, frames)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NRD_HIP_TA_WINDOW_LIMIT="35x11"), capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    assert float(re.search(r"worst ([0-9.eE+-]+)", out.stdout).group(1)) == 0.0, out.stdout[-2000:]
    stats = [(int(a), int(b)) for a, b in re.findall(r"tiles left to a fallback kernel: (\d+) of (\d+)", out.stdout)]
    print("tiles left to the fallback kernel per frame:", stats)
    assert len(stats) == frames
    total = ((w + 31) // 32) * ((h + 7) // 8)
    assert all(t == total for _, t in stats), stats
    for f, (flagged, _) in enumerate(stats):
        if f == SKY_FRAME:
            assert flagged == 0, stats  # flagged on the frame before, sky now: not counted
        else:
            assert 0 < flagged < total, stats  # both kernels had tiles


# ---- the ISA of the benchmarked kernels ------------------------------------------------------------------------------------------------------------------------------
def test_no_vector_memory_or_lds_instruction_in_front_of_the_sky_exit():
    """compiles the kernels of the benchmarked frame (REBLUR_DIFFUSE_SPECULAR at 1440p, RELAX_DIFFUSE_SPECULAR_SH at 4K) to gfx950 assembly with the product's flags and walks
    each from its entry to the first point at which a workgroup can end (tools/isa_sky_exit.py): no global_ / buffer_ / flat_ / scratch_ / ds_ instruction on the way, except
    the window kernel's store of its flag byte (lane 0) on the exit path itself"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_sky_exit

    report = isa_sky_exit.check_all(verbose=True)
    bad = {k: v for k, v in report.items() if not v["ok"]}
    assert report and not bad, bad
