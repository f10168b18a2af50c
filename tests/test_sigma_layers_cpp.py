"""SIGMA for many lights from C++: tests/cpp/sigma_layers_integration.cpp drives nrd::IntegrationHip with layersNum = 2 (include/NRDIntegrationHip.hpp) for one
64 x 32 frame and holds layer 1 against an unlayered IntegrationHip run on layer 1's planes, byte for byte. Built and run the way tests/test_integration_cpp.py does its
program. CPU: compiles, links and runs the host-only part (the user pool with its layer strides); GPU: the whole program."""
import os
import subprocess

import pytest

from raytracingdenoiser_amd import build as native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sigma_layers_integration.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "sigma_layers_integration")
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


def test_cpp_layered_integration_compiles_links_and_keeps_the_pool_strides():
    _build()
    r = subprocess.run([EXE, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only OK" in r.stdout


@pytest.mark.gpu
def test_cpp_layered_integration_layer_equals_unlayered_run():
    if os.environ.get("NRD_PARITY_BACKEND") == "emu":
        pytest.skip("the program links the real HIP runtime and allocates device memory: no emulated twin")
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "layer 1 has 0 mismatching bytes" in r.stdout and "sigma layers integration OK" in r.stdout
