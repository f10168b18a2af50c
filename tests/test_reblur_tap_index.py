"""The one-index tap of the REBLUR spatial passes (kernels_reblur_spatial.hip, FR == 3) is another way to form the same byte offsets: REBLUR_DIFFUSE_SPECULAR, 4 frames,
moving camera, every output and every pool plane against the oracle with error 0, at
  96 x 72    three tile columns, XCD stripes off, the rect edge inside every tap's reach; the pool's 256-byte row padding gives the 4-byte planes another pitch in texels than
             the 8- and 16-byte ones, so PrePass and Blur take the indexed tap and PostBlur (which reads its own R32F viewZ per tap) does not;
  200 x 104  a width that is no multiple of 32: partial tiles on the right, the clamp and in-screen path on both axes; no two texel sizes share a pitch in texels, so every
             pass must fall back to the per-plane offsets;
  128 x 72   a multiple of 64: all planes share the pitch in texels, every pass takes the indexed tap (as at 1440p and 4K).
Then the same frames byte for byte between child processes that take the indexed tap, the per-plane offsets (NRD_HIP_TAP_INDEX=0) and the generic tap (NRD_HIP_GENERIC_TAPS=1),
user planes with a padded pitch (the launcher must fall back, not mis-address), and the two small sizes once more with a shrunken TemporalAccumulation window, so that
window and fallback tiles both occur in front of the spatial passes. tests/test_tap_index_host.py holds the launcher's predicate on the CPU."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity
from raytracingdenoiser_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = api.ResourceType
NAME = "REBLUR_DIFFUSE_SPECULAR"
FRAMES = 4
SIZES = [(96, 72), (200, 104), (128, 72)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_output_and_pool_plane_equals_the_oracle(size):
    worst = parity.run_parity(NAME, width=size[0], height=size[1], frames=FRAMES)
    print("%s %dx%d: worst relative error %g" % (NAME, size[0], size[1], worst))
    assert worst == 0.0, (size, worst)


@pytest.mark.gpu
def test_a_padded_pitch_of_the_user_planes_falls_back_to_per_plane_offsets():
    """128 x 72 is a size at which every pass takes the indexed tap; with the user's planes living in wider allocations (24 texels more per row, first texel one row in) the
    pre-pass's signal inputs no longer share the guide plane's pitch in texels -- error 0 says the launcher noticed"""
    worst = parity.run_parity(NAME, width=128, height=72, frames=FRAMES, pad=24)
    print("padded user planes: worst relative error %g" % worst)
    assert worst == 0.0, worst


def run_digest_case():
    """(child process: the switches are read by the library from its environment) one digest per size, frame and plane -- every output and every pool plane"""
    for w, h in SIZES[1:]:
        seq = parity.generate_sequence(NAME, w, h, FRAMES)
        hip = parity.HipRun(NAME, w, h)
        for f, frame in enumerate(seq):
            hip.step(frame, parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], w, h, f), parity.denoiser_settings(NAME, frame, None))
            planes = [(rt.name, hip.output(rt)) for rt in hip.outs]
            for pool in (RT.PERMANENT_POOL, RT.TRANSIENT_POOL):
                for i in range(len(hip.inst.permanent_pool if pool == RT.PERMANENT_POOL else hip.inst.transient_pool)):
                    raw, fmt, pw = hip.ex.read_pool_plane(pool, i)
                    planes.append(("%s[%d]" % (pool.name, i), np.asarray(raw)[:, : pw * api.FORMAT_BYTES[fmt]]))
            for label, a in planes:
                print("digest %dx%d frame %d %s %s" % (w, h, f, label, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()))


def _child(code, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("NRD_HIP_GENERIC_TAPS", "NRD_HIP_TAP_INDEX", "NRD_HIP_TA_WINDOW_LIMIT")}
    return subprocess.Popen([sys.executable, "-c", code], env=dict(env, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.gpu
def test_indexed_taps_per_plane_offsets_and_generic_taps_compute_the_same_bytes():
    code = "import sys; sys.path[:0] = [%r, %r]; import test_reblur_tap_index; test_reblur_tap_index.run_digest_case()" % (ROOT, os.path.join(ROOT, "tests"))
    procs = [_child(code, extra) for extra in ({}, {"NRD_HIP_TAP_INDEX": "0"}, {"NRD_HIP_GENERIC_TAPS": "1"})]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    indexed, per_plane, generic = ([line for line in out.splitlines() if line.startswith("digest ")] for out, _ in outs)
    assert len(indexed) == len(per_plane) == len(generic) and len(indexed) >= 2 * FRAMES * 10, (len(indexed), len(per_plane), len(generic))
    differing = [a for a, b, c in zip(indexed, per_plane, generic) if not a == b == c]
    print("%d planes compared, %d differ" % (len(indexed), len(differing)))
    assert not differing, [d.rsplit(" ", 1)[0] for d in differing[:8]]


@pytest.mark.gpu
def test_shrunken_temporal_accumulation_window_at_the_small_sizes():
    """NRD_HIP_TA_WINDOW_LIMIT (read once per process, hence the child) shrinks the rectangle the window kernel accepts until both TemporalAccumulation kernels have tiles, as
    tests/test_executor.py does at 256 x 160: error 0 at both sizes"""
    code = ("import sys; sys.path[:0] = [%r, %r]; import parity\n"
            "for w, h in ((96, 72), (200, 104)):\n"
            "    print('worst', parity.run_parity(%r, width=w, height=h, frames=%d, verbose=True))\n") % (ROOT, os.path.join(ROOT, "tests"), NAME, FRAMES)
    p = _child(code, {"NRD_HIP_TA_WINDOW_LIMIT": "35x11"})
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0, err[-2000:]
    worst = [float(m) for m in re.findall(r"worst ([0-9.eE+-]+|inf|nan)", out)]
    assert worst == [0.0, 0.0], (worst, out[-2000:])
    tiles = [(int(a), int(b)) for a, b in re.findall(r"tiles left to a fallback kernel: (\d+) of (\d+)", out)]
    print("tiles left to the fallback kernel per frame:", tiles)
    assert len(tiles) == 2 * FRAMES and any(0 < a < b for a, b in tiles[:FRAMES]) and any(0 < a < b for a, b in tiles[FRAMES:]), tiles
