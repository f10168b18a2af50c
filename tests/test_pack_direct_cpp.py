"""Combined direct and indirect lighting from C++: tests/cpp/pack_direct_integration.cpp calls IntegrationHip::PackInputsDirect (include/NRDIntegrationHip.hpp over
nrdHipPackInputsDirect) and evaluates NRD_HIP_MixDiffuseHitDist of include/NRD.hip.h on the host. Built against the installed headers the way tests/test_pack_lobes_cpp.py
builds its program. CPU: the struct sizes (static_assert), the refusals, which touch no device, and the mixing function over the table of edge cases of tests/direct_model.py,
bit for bit; GPU: IntegrationHip::PackInputsDirect returns what the C-ABI returns, and both the values worked out by hand."""
import os
import subprocess

import numpy as np
import pytest

import direct_model as DM
from raytracingdenoiser_amd import build as native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pack_direct_integration.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "pack_direct_integration")
HEADERS = [os.path.join(ROOT, "include", h) for h in ("NRDHip.h", "NRDIntegrationHip.hpp", "NRD.hip.h")]


def _build():
    lib = native_build.build_product()
    os.makedirs(OUT_DIR, exist_ok=True)
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(p) for p in [SRC, lib] + HEADERS):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-attributes", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", SRC, "-o", EXE,
           "-L" + os.path.dirname(lib), "-lNRD_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../../../raytracingdenoiser_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cpp_direct_program_compiles_links_and_is_refused_by_name():
    _build()
    r = subprocess.run([EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only OK" in r.stdout


def test_mixing_function_on_the_host_agrees_with_the_model_bit_for_bit(tmp_path):
    """NRD_HIP_MixDiffuseHitDist over the edge cases -- every branch for maxContribution 0, 0.5, 0.65 and 1, NaN / inf / 0 / negative hit distances and weights -- and over
    random rows: the header's function in C++ (unfused, -ffp-contract=off) == tests/direct_model.py in float32 numpy"""
    _build()
    rng = np.random.RandomState(11)
    random_rows = np.stack([rng.uniform(0, 30, 4096), rng.uniform(0, 30, 4096), rng.uniform(0, 5, 4096), rng.uniform(0, 5, 4096), rng.choice([0.0, 0.5, 0.65, 1.0], 4096)], -1).astype(np.float32)
    table = np.concatenate([DM.edge_table(), random_rows])
    src, dst = str(tmp_path / "rows.bin"), str(tmp_path / "mixed.bin")
    table.tofile(src)
    r = subprocess.run([EXE, "--mix", src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mixed %d rows" % len(table) in r.stdout, r.stdout + r.stderr
    got = np.fromfile(dst, np.float32)
    want = np.concatenate([DM.mix_diffuse_hit_dist(row[0:1], row[1:2], row[2:3], row[3:4], row[4]) for row in table])
    assert got.shape == want.shape
    same = got.view(np.uint32) == want.view(np.uint32)
    both_nan = np.isnan(got) & np.isnan(want)  # (a NaN h_i is returned as it is: any NaN payload)
    assert (same | both_nan).all(), table[~(same | both_nan)][:5]
    mixed = got != table[:, 0]
    assert mixed[len(DM.edge_table()):].mean() > 0.5 and (~mixed[: len(DM.edge_table())]).sum() > 40  # both sides of the branch are in the table


@pytest.mark.gpu
def test_cpp_direct_program_packs_what_the_c_abi_packs():
    if os.environ.get("NRD_PARITY_BACKEND") == "emu":
        pytest.skip("the program links the real HIP runtime and allocates device memory: no emulated twin")
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed texels: 0 mismatching values, 0 differing from the C-ABI call's" in r.stdout and "pack direct integration OK" in r.stdout
