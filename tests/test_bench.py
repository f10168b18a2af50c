"""bench.py: a plain run measures the headline value only; --full adds the replays, the roofline and the CPU baseline with its parity check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures: each takes work of its own outside the timed region
FULL_ONLY = ("tile_fallback", "roofline", "whole_chain", "passes", "frame_ms", "cpu_baseline", "parity")


def test_full_is_off_by_default(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--warmup", "2"])
    assert not bench.parse_args().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--warmup", "2", "--full"])
    assert bench.parse_args().full


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--width", "192", "--height", "128"] + list(args),
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_computes_what_a_full_run_computes(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("bench.py needs the HIP runtime (the emulated parity backend cannot run it)")
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--cpu-frames", "2", "--dump-outputs", str(tmp_path / "full"))
    assert not [k for k in FULL_ONLY if k in plain], sorted(plain)
    assert all(k in full for k in FULL_ONLY), sorted(full)
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert full["parity"]["max_rel_err"] == 0.0 and full["roofline"]["kernel"].startswith("REBLUR_")
    # the extra measurements of --full come before or after the timed steps and change none of their inputs: the last timed frame's outputs are the same bits
    assert plain["dump_outputs"]["shapes"] == full["dump_outputs"]["shapes"] and plain["dump_outputs"]["shapes"]
    for key in plain["dump_outputs"]["shapes"]:
        a, b = np.load(tmp_path / "plain" / (key + ".npy")), np.load(tmp_path / "full" / (key + ".npy"))
        assert a.tobytes() == b.tobytes(), key
