"""The launcher's predicate for the one-index tap of the REBLUR spatial passes (csrc/host/tap_index.h; kernels_reblur_spatial.hip, FR == 3) is host-only code:
tests/cpp/tap_index_host.cpp builds from that header alone -- no HIP runtime, nothing loaded into python -- under AddressSanitizer + UndefinedBehaviorSanitizer. The predicate
must hold only where every plane a tap reads has the same pitch in texels and fewer than 2^24 of them; where it holds, the program forms the index as the kernel does (one fp32
fma, one conversion) and compares the byte offsets it gives with y * pitch + x * bytesPerTexel in every plane."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tap_index_host.cpp")
HEADER = os.path.join(ROOT, "raytracingdenoiser_amd", "csrc", "host", "tap_index.h")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "tap_index_host")
CLANG = os.environ.get("NRD_EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]


def _pool_pitch(width, bytes_per_texel):
    return (width * bytes_per_texel + 255) & ~255  # executor.hip PlanPool: rows padded to 256 bytes, per plane


def _pool_planes(width):
    """(pitch, bytes per texel) of the planes a PostBlur tap of REBLUR_DIFFUSE_SPECULAR reads: the (normal, viewZ) guide, two RGBA16F signals, the pass's R32F viewZ"""
    return [(_pool_pitch(width, 16), 16), (_pool_pitch(width, 8), 8), (_pool_pitch(width, 8), 8), (_pool_pitch(width, 4), 4)]


# (label, w, h, [(pitch, bytes per texel), ...], expected)
CASES = [
    ("1440p, pool pitches", 2560, 1440, _pool_planes(2560), True),
    ("4K, pool pitches", 3840, 2160, _pool_planes(3840), True),
    ("8K: more than 2^24 texels", 7680, 4320, _pool_planes(7680), False),
    ("1440p, one signal with a padded pitch", 2560, 1440, [(2560 * 16, 16), (2560 * 8 + 256, 8), (2560 * 8, 8), (2560 * 4, 4)], False),
    ("1440p, every plane padded by the same number of texels", 2560, 1440, [(2592 * 16, 16), (2592 * 8, 8), (2592 * 8, 8), (2592 * 4, 4)], True),
    ("200 wide: the 256-byte row padding differs per texel size", 200, 104, _pool_planes(200), False),
    ("96 wide, PostBlur: the R32F plane has another pitch in texels", 96, 72, _pool_planes(96), False),
    ("96 wide, Blur: guide and signals agree", 96, 72, _pool_planes(96)[:3], True),
    ("128 wide", 128, 72, _pool_planes(128), True),
    ("exactly 2^24 texels", 4096, 4096, _pool_planes(4096), True),
    ("one row more than 2^24 texels", 4096, 4097, _pool_planes(4096), False),
    ("a pitch that is no whole number of texels", 64, 64, [(64 * 16 + 8, 16), (64 * 8 + 4, 8)], False),
    ("a pitch below the width", 64, 64, [(32 * 16, 16), (32 * 8, 8)], False),
    ("R16_UNORM signals (occlusion family)", 2560, 1440, [(2560 * 16, 16), (2560 * 2, 2), (2560 * 2, 2)], True),
    ("the guide plane alone", 2560, 1440, [(2560 * 16, 16)], True),
    ("no plane", 64, 64, [], False),
]


def test_tap_index_predicate_and_the_offsets_it_promises(tmp_path):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not (os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(SRC), os.path.getmtime(HEADER))):
        r = subprocess.run([CLANG] + FLAGS + [SRC, "-o", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    cases = tmp_path / "cases.txt"
    cases.write_text("".join("%d %d %d %s\n" % (w, h, len(planes), " ".join("%d %d" % p for p in planes)) for _, w, h, planes, _ in CASES))
    r = subprocess.run([EXE, str(cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert not [line for line in r.stderr.splitlines() if "Sanitizer" in line or "runtime error" in line], r.stderr[-3000:]
    got = json.loads(r.stdout)
    assert len(got["tap_index"]) == len(CASES)
    for verdict, (label, _, _, _, expected) in zip(got["tap_index"], CASES):
        assert bool(verdict) == expected, label
    assert got["offsets_checked"] > 0 and got["bad_offsets"] == 0, got
