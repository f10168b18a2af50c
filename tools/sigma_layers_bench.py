"""SIGMA for many lights: times the layered executor (include/NRDHip.h nrdHipCreateExecutorLayered: N shadow layers in one pass chain, the layer in grid.z) against the loop
over the lights it replaces. SIGMA_SHADOW at 1920 x 1080, N in {1, 4, 8, 16, 32} lights, every variant eager and in graph mode, all in one process:
  (a) loop                  the loop of INTEGRATION.md 3a on ONE unlayered executor, temporal stabilisation off (maxStabilizedFrameNum = 0) -- the baseline: only what
                            existed before the layered executor
  (b) layered               the layered executor, stabilisation off: the same bytes as (a) (checked at full size before anything is timed)
  (c) layered_stabilized    the layered executor with the default stabilisation: per-light history in one instance ...
  (c0) separate_stabilized  ... against what that took before: N unlayered executors over N instances
Protocol: 10 warm-up frames per variant, then HIP events around a window of at least 0.5 s of back-to-back frames; the variants alternate and the whole round is repeated
5 times. Reported per variant: the median, min and max over the repetitions of ms per frame (a frame = all N lights), ms per light, and the ratio (a) / (b). The times are
those of a Python host driving the C-ABI: launch overhead of the host is part of them, as it is of any frame.
usage: python tools/sigma_layers_bench.py [--lights 1 4 8 16 32] [--width 1920 --height 1080] [--reps 5] [--window 0.5] [--out profiles/sigma_layers_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from raytracingdenoiser_amd import api, frontend, scene  # noqa: E402
from raytracingdenoiser_amd.executor import HipExecutor  # noqa: E402

RT, F = api.ResourceType, api.Format
NAME = "SIGMA_SHADOW"
OFF = dict(maxStabilizedFrameNum=0)


class Variant:
    """one way to denoise the N layers of a frame; frame(f) enqueues frame f"""

    def __init__(self, kind, n, frame, penumbra, graph):
        self.kind, self.n, self.src, self.penumbra = kind, n, frame, penumbra
        w, h = penumbra.shape[2], penumbra.shape[1]
        self.w, self.h = w, h
        self.overrides = OFF if kind in ("loop", "layered") else None
        self.out = frontend.shadow_stack(penumbra, n, h, w)
        self.out.zero_()
        self.guides = [(rt, t.contiguous(), fmt) for rt, t, fmt in scene.user_planes(NAME, frame) if rt != RT.IN_PENUMBRA]
        layered = kind.startswith("layered") and n > 1
        count = n if kind == "separate_stabilized" else 1
        self.instances = [api.Instance([(0, scene.DENOISERS[NAME][0])]) for _ in range(count)]
        self.executors = [HipExecutor(inst, w, h, layers=n if layered else 1) for inst in self.instances]
        for i, ex in enumerate(self.executors):
            ex.set_graph_mode(graph)
            for rt, t, fmt in self.guides:
                ex.bind(rt, t, fmt)
            if layered:
                ex.bind_layers(RT.IN_PENUMBRA, penumbra, F.R16_SFLOAT)
                ex.bind_layers(RT.OUT_SHADOW_TRANSLUCENCY, self.out, F.R8_UNORM)
            elif kind != "loop" or n == 1:
                ex.bind(RT.IN_PENUMBRA, penumbra[i], F.R16_SFLOAT)
                ex.bind(RT.OUT_SHADOW_TRANSLUCENCY, self.out[i], F.R8_UNORM)

    def _settings(self, inst, f):
        cam = self.src["camera"]
        assert inst.set_denoiser_settings(0, scene.denoiser_settings(NAME, self.src, self.overrides)) == api.Result.SUCCESS
        assert inst.set_common_settings(scene.common_settings(cam, cam, self.w, self.h, f)) == api.Result.SUCCESS

    def frame(self, f):
        if self.kind == "loop":  # rebind two slots, set the settings, denoise -- per light
            ex, inst = self.executors[0], self.instances[0]
            for i in range(self.n):
                if self.n > 1:
                    ex.bind(RT.IN_PENUMBRA, self.penumbra[i], F.R16_SFLOAT)
                    ex.bind(RT.OUT_SHADOW_TRANSLUCENCY, self.out[i], F.R8_UNORM)
                self._settings(inst, f)
                ex.denoise()
        else:
            for ex, inst in zip(self.executors, self.instances):
                self._settings(inst, f)
                ex.denoise()

    def destroy(self):
        for ex in self.executors:
            ex.destroy()
        for inst in self.instances:
            inst.destroy()


def timed_window(variant, first_frame, frames):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for k in range(frames):
        variant.frame(first_frame + k)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lights", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back frames per timed window, at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_layers_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    w, h = args.width, args.height
    frame = scene.generate_sequence(NAME, w, h, 1, device="cuda")[0]
    result = {"denoiser": NAME, "width": w, "height": h, "device": torch.cuda.get_device_name(0), "warmup_frames": args.warmup, "window_seconds_min": args.window,
              "repetitions": args.reps, "host": "python (ctypes over the C-ABI)", "lights": {}}
    kinds = ("loop", "layered", "layered_stabilized", "separate_stabilized")
    for n in args.lights:
        # the lights: the scene's penumbra, moved sideways by a different amount per light (different tile maps, the same amount of work)
        penumbra = frontend.light_stack(frame["penumbra"], n, (h, w), "float16")
        for i in range(n):
            penumbra[i].copy_(torch.roll(frame["penumbra"].view(h, w), shifts=37 * i, dims=1))
        entry = {}
        for graph in (False, True):
            variants = {kind: Variant(kind, n, frame, penumbra, graph) for kind in kinds}
            # (a) and (b) must agree byte for byte at this size before anything is timed
            variants["loop"].frame(0)
            variants["layered"].frame(0)
            torch.cuda.synchronize()
            equal = bool(torch.equal(variants["loop"].out, variants["layered"].out))
            assert equal, "N = %d: the layered executor and the loop disagree at %d x %d" % (n, w, h)
            assert int(variants["layered"].out.unique().numel()) > 2
            frames, f0 = {}, {}
            for kind, v in variants.items():
                for f in range(1, 1 + args.warmup):
                    v.frame(f)
                per_frame = timed_window(v, 1 + args.warmup, 10) / 10.0  # calibration: how many frames fill the window
                frames[kind] = max(10, int(math.ceil(args.window * 1000.0 / max(per_frame, 1e-3))))
                f0[kind] = 11 + args.warmup
            samples = {kind: [] for kind in kinds}
            for _ in range(args.reps):
                for kind, v in variants.items():  # alternating
                    ms = timed_window(v, f0[kind], frames[kind])
                    f0[kind] += frames[kind]
                    while ms < args.window * 1000.0:  # the calibration was too short (it ran cold): a longer window, timed again
                        frames[kind] = int(math.ceil(frames[kind] * args.window * 1000.0 / max(ms, 1e-3) * 1.1))
                        ms = timed_window(v, f0[kind], frames[kind])
                        f0[kind] += frames[kind]
                    samples[kind].append(ms / frames[kind])
            mode = {"equal_bytes_loop_vs_layered": equal}
            for kind in kinds:
                med = statistics.median(samples[kind])
                mode[kind] = {"ms_per_frame_median": med, "ms_per_frame_min": min(samples[kind]), "ms_per_frame_max": max(samples[kind]), "ms_per_light_median": med / n,
                              "frames_per_window": frames[kind], "ms_per_frame_samples": samples[kind]}
            mode["ratio_loop_over_layered"] = mode["loop"]["ms_per_frame_median"] / mode["layered"]["ms_per_frame_median"]
            mode["ratio_separate_over_layered_stabilized"] = mode["separate_stabilized"]["ms_per_frame_median"] / mode["layered_stabilized"]["ms_per_frame_median"]
            # "not slower beyond the spread": the layered median against the slowest repetition of the baseline
            mode["layered_not_slower_than_loop"] = mode["layered"]["ms_per_frame_median"] <= mode["loop"]["ms_per_frame_max"]
            entry["graph" if graph else "eager"] = mode
            print("N = %2d %-5s  loop %.4f  layered %.4f  (x%.2f)   separate+TS %.4f  layered+TS %.4f  (x%.2f)  ms per frame" % (
                n, "graph" if graph else "eager", mode["loop"]["ms_per_frame_median"], mode["layered"]["ms_per_frame_median"], mode["ratio_loop_over_layered"],
                mode["separate_stabilized"]["ms_per_frame_median"], mode["layered_stabilized"]["ms_per_frame_median"], mode["ratio_separate_over_layered_stabilized"]), flush=True)
            for v in variants.values():
                v.destroy()
        result["lights"][str(n)] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
