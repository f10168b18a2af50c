"""REBLUR HistoryFix requests the texels of its reconstruction taps in groups (kernels_reblur_history.hip hf::TAP_BATCH) and sums them in the reference's order:
no value may change. Every case is held against the oracle bit for bit -- every user output and every pool plane of every frame -- on the paths the grouping touches:
all pixels young (frames 0-1), young and old lanes mixed in one wave (later frames of a moving camera), taps clamped at every edge (stride 14 reaches +-28 px),
partial tiles, every settings field the loop reads, every instantiation of the kernel, and a camera cut in mid-sequence."""
import numpy as np
import pytest

import parity
from raytracingdenoiser_amd import api

RT = api.ResourceType
SMALL = (96, 72)  # +-28 px of taps: nearly every pixel has taps clamped at some edge


@pytest.mark.gpu
@pytest.mark.parametrize("size", [SMALL, (200, 104)])  # 200x104: partial tiles in x (200 = 6 x 32 + 8)
def test_diffuse_specular_moving_camera(size):
    worst = parity.run_parity("REBLUR_DIFFUSE_SPECULAR", width=size[0], height=size[1], frames=6)
    assert worst == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("overrides", [dict(historyFixFrameNum=1), dict(historyFixFrameNum=6), dict(historyFixBasePixelStride=3), dict(historyFixBasePixelStride=30),
                                       dict(enableAntiFirefly=True)], ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_settings_the_loop_reads(overrides):
    """historyFixFrameNum: which lanes are young; historyFixBasePixelStride: 3 floors to a stride of 0 once a pixel has history (the loop is skipped), 30 clamps most taps"""
    worst = parity.run_parity("REBLUR_DIFFUSE_SPECULAR", width=SMALL[0], height=SMALL[1], frames=6, settings_overrides=overrides)
    assert worst == 0.0


@pytest.mark.gpu
def test_material_test_is_live():
    """minMaterialFor* = 0 with the scene's four material IDs: every tap decodes and compares its material (the default, 4, skips both on a uniform test)"""
    worst = parity.run_parity("REBLUR_DIFFUSE_SPECULAR", width=SMALL[0], height=SMALL[1], frames=6, extra_want=("materials",),
                              settings_overrides=dict(minMaterialForDiffuse=0.0, minMaterialForSpecular=0.0))
    assert worst == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,overrides", [("REBLUR_DIFFUSE", None), ("REBLUR_SPECULAR", None), ("REBLUR_DIFFUSE_SPECULAR_OCCLUSION", None), ("REBLUR_DIFFUSE_SPECULAR_SH", None),
                                            ("REBLUR_DIFFUSE_SPECULAR", dict(enablePerformanceMode=True))],
                         ids=["diffuse", "specular", "occlusion", "sh", "performance_mode"])
def test_other_instantiations(name, overrides):
    worst = parity.run_parity(name, width=SMALL[0], height=SMALL[1], frames=4, settings_overrides=overrides)
    assert worst == 0.0


def _assert_same_state(ora, hip, frame):
    for rt in ora.outs:
        assert np.array_equal(hip.output(rt), ora.output(rt), equal_nan=True), "frame %d %s" % (frame, rt.name)
    for pool in (RT.PERMANENT_POOL, RT.TRANSIENT_POOL):
        descs = ora.inst.permanent_pool if pool == RT.PERMANENT_POOL else ora.inst.transient_pool
        for i in range(len(descs)):
            o_raw, fmt, w = ora.ex.pool_plane(pool, i)
            h_raw, hfmt, hw = hip.ex.read_pool_plane(pool, i)
            assert fmt == hfmt and w == hw
            row_bytes = w * api.FORMAT_BYTES[fmt]
            assert np.array_equal(o_raw[:, :row_bytes], h_raw[:, :row_bytes]), "frame %d %s[%d] %s" % (frame, pool.name, i, fmt.name)


@pytest.mark.gpu
def test_camera_cut():
    """three frames of history, then a CLEAR_AND_RESTART frame (every pixel of both signals is reconstructed again) and two frames behind it"""
    name, (w, h), frames, cut = "REBLUR_DIFFUSE_SPECULAR", SMALL, 6, 3
    seq = parity.generate_sequence(name, w, h, frames)
    ora, hip = parity.OracleRun(name, w, h), parity.HipRun(name, w, h)
    for f, frame in enumerate(seq):
        cam, cam_prev = frame["camera"], seq[max(f - 1, 0)]["camera"]
        kw = dict(accumulationMode=int(api.AccumulationMode.CLEAR_AND_RESTART)) if f == cut else {}
        ora.step(frame, parity.common_settings(cam, cam_prev, w, h, f, **kw), parity.denoiser_settings(name, frame, None))
        hip.step(frame, parity.common_settings(cam, cam_prev, w, h, f, **kw), parity.denoiser_settings(name, frame, None))
        _assert_same_state(ora, hip, f)
