"""The probabilistic split from C++: tests/cpp/pack_lobes_integration.cpp calls IntegrationHip::PackInputsLobes / CheckHitDistCoverage (include/NRDIntegrationHip.hpp over
nrdHipPackInputsLobes / nrdHipCheckHitDistCoverage) for one 67 x 21 frame: one pack, then the audit of the packed planes for both areas. Built and run the way
tests/test_sigma_layers_cpp.py does its program. CPU: compiles, links and runs the host-only part (the refusals, which touch no device); GPU: the whole program."""
import os
import subprocess

import pytest

from raytracingdenoiser_amd import build as native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pack_lobes_integration.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "pack_lobes_integration")
HEADERS = [os.path.join(ROOT, "include", h) for h in ("NRDHip.h", "NRDIntegrationHip.hpp")]


def _build():
    lib = native_build.build_product()
    os.makedirs(OUT_DIR, exist_ok=True)
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(p) for p in [SRC, lib] + HEADERS):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-attributes", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", SRC, "-o", EXE,
           "-L" + os.path.dirname(lib), "-lNRD_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../../../raytracingdenoiser_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cpp_lobes_program_compiles_links_and_is_refused_by_name():
    _build()
    r = subprocess.run([EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only OK" in r.stdout


@pytest.mark.gpu
def test_cpp_lobes_program_packs_and_audits_one_frame():
    if os.environ.get("NRD_PARITY_BACKEND") == "emu":
        pytest.skip("the program links the real HIP runtime and allocates device memory: no emulated twin")
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed texels: 0 mismatching values" in r.stdout and "3x3: 1 diffuse hole(s), the first at (10, 12); 5x5: 0" in r.stdout and "pack lobes integration OK" in r.stdout
