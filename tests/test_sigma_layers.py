"""The layered executor (include/NRDHip.h nrdHipCreateExecutorLayered): N SIGMA shadow layers -- one per light -- denoised by ONE pass chain, the layer in the third
grid dimension. The contract held here: after any sequence of frames, layer l of OUT_SHADOW_TRANSLUCENCY and of every pool plane holds byte for byte what a separate
unlayered executor over its own instance holds that ran the same frames on layer l's planes; nothing is written between the layers of a user stack.

Frame 83 x 45 (partial in the 16x16 tiles, the 32x8 workgroups and the 16x16 smooth-tile groups; pool pitches are padded), N = 3 (the stride is multiplied, not only added):
layer 0 = the scene's penumbra, layer 1 = every pixel lit (all tiles leave early), layer 2 = the scene's penumbra flipped left-right -- three different tile maps.

The planes are raw byte buffers bound through the C-ABI, so that the same tests run on the GPU and, with NRD_PARITY_BACKEND=emu on a machine without one, on the CPU
emulation of the device sources (tests/emu); only the test of the public Python path needs torch.cuda tensors."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import parity
from raytracingdenoiser_amd import api

RT, F, R = api.ResourceType, api.Format, api.Result
EMU = os.environ.get("NRD_PARITY_BACKEND") == "emu"
W, H, N = 83, 45, 3
STAMP = 0xA7  # every byte of a user buffer that is no texel: row padding, the bytes between two layers, a guard row behind the last layer
LIT = 65504.0


def _lib():
    if EMU:
        from emu import emu_run

        return emu_run.load()
    return api.load_library()


def _sync():
    if not EMU:
        import torch

        torch.cuda.synchronize()


class Buf:
    """bytes the kernels can address: a CUDA tensor, or host memory under the emulation"""

    def __init__(self, host):
        if EMU:
            self.mem = np.array(host, dtype=np.uint8, copy=True)
            self.ptr = self.mem.ctypes.data
        else:
            import torch

            self.mem = torch.from_numpy(np.ascontiguousarray(host)).cuda()
            self.ptr = self.mem.data_ptr()

    def upload(self, host):
        if EMU:
            self.mem[...] = host
        else:
            import torch

            self.mem.copy_(torch.from_numpy(np.ascontiguousarray(host)))

    def read(self):
        _sync()
        return self.mem.copy() if EMU else self.mem.cpu().numpy()


def _read_device(ptr, nbytes):
    _sync()
    if EMU:
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8).copy()
    from raytracingdenoiser_amd.executor import _hip_runtime

    host = np.empty(nbytes, dtype=np.uint8)
    assert _hip_runtime().hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nbytes, 2) == 0
    return host


class Stack:
    """n planes of h x w texels of bpt bytes in one buffer: rows padded by 3 texels, the layers 24 bytes (rounded up to 4) further apart than a plane, a guard row behind the
    last layer. Everything that is no texel holds STAMP; the texels start as `fill`."""

    def __init__(self, n, h, w, bpt, fill=0):
        self.n, self.h, self.w, self.bpt = n, h, w, bpt
        self.pitch = (w + 3) * bpt
        self.layer_bytes = (self.pitch * h + 24 + 3) & ~3
        self.host = np.full(n * self.layer_bytes + self.pitch, STAMP, dtype=np.uint8)
        self.texels = np.zeros(self.host.size, dtype=bool)
        for l in range(n):
            self._rows(self.texels, l)[...] = True
            self._rows(self.host, l)[...] = fill
        self.buf = Buf(self.host)

    def _rows(self, flat, l):
        return flat[l * self.layer_bytes: l * self.layer_bytes + self.pitch * self.h].reshape(self.h, self.pitch)[:, : self.w * self.bpt]

    def upload(self, planes):
        for l, p in enumerate(planes):
            self._rows(self.host, l)[...] = np.ascontiguousarray(p).view(np.uint8).reshape(self.h, self.w * self.bpt)
        self.buf.upload(self.host)

    def layers(self):
        got = self.buf.read()
        return [self._rows(got, l).copy() for l in range(self.n)], bool(np.all(got[~self.texels] == STAMP))

    def stamp_outside(self, rect_w, rect_h, value):
        """overwrites the texels outside the top-left rect of every layer, on the device"""
        self.host = self.buf.read()
        for l in range(self.n):
            rows = self._rows(self.host, l)
            rows[rect_h:] = value
            rows[:, rect_w * self.bpt:] = value
        self.buf.upload(self.host)

    def desc(self, fmt, layer=0):
        return api.HipPlaneDesc(self.buf.ptr + layer * self.layer_bytes, self.pitch, int(fmt), self.w, self.h)


class Run:
    """an instance and its executor over the C-ABI: layers=None -> nrdHipCreateExecutor, otherwise nrdHipCreateExecutorLayered"""

    def __init__(self, name, w, h, layers=None):
        self.lib = _lib()
        self.inst = api.Instance([(0, parity.DENOISERS[name][0])], lib=self.lib)
        self.handle = C.c_void_p()
        if layers is None:
            self.created = R(self.lib.nrdHipCreateExecutor(self.inst.handle, w, h, None, C.byref(self.handle)))
        else:
            self.created = R(self.lib.nrdHipCreateExecutorLayered(self.inst.handle, w, h, layers, None, C.byref(self.handle)))
        self.keep = {}

    def error(self):
        return self.lib.nrdHipGetLastError(self.handle).decode()

    def bind(self, rt, stack, fmt, layer=0):
        self.keep[int(rt)] = stack
        return R(self.lib.nrdHipBindResource(self.handle, int(rt), C.byref(stack.desc(fmt, layer))))

    def bind_layers(self, rt, stack, fmt, layer_bytes=None):
        self.keep[int(rt)] = stack
        return R(self.lib.nrdHipBindResourceLayers(self.handle, int(rt), C.byref(stack.desc(fmt)), stack.layer_bytes if layer_bytes is None else layer_bytes))

    def settings(self, cs, st):
        assert self.inst.set_denoiser_settings(0, st) == R.SUCCESS and self.inst.set_common_settings(cs) == R.SUCCESS

    def denoise(self):
        ids = (C.c_uint32 * 1)(0)
        return R(self.lib.nrdHipDenoise(self.handle, ids, 1))

    def layers_num(self):
        n = C.c_uint32(77)
        assert R(self.lib.nrdHipGetLayersNum(self.handle, C.byref(n))) == R.SUCCESS
        return n.value

    def pool_memory(self):
        p, t = C.c_uint64(), C.c_uint64()
        assert R(self.lib.nrdHipGetPoolMemoryUsage(self.handle, C.byref(p), C.byref(t))) == R.SUCCESS
        return p.value, t.value

    def pool_planes(self, layer=None):
        """the bytes [h, pitch] of every pool plane (of one layer; None: through nrdHipGetPoolPlane)"""
        out = []
        for pool, descs in ((RT.PERMANENT_POOL, self.inst.permanent_pool), (RT.TRANSIENT_POOL, self.inst.transient_pool)):
            for i in range(len(descs)):
                d = api.HipPlaneDesc()
                if layer is None:
                    assert R(self.lib.nrdHipGetPoolPlane(self.handle, int(pool), i, C.byref(d))) == R.SUCCESS
                else:
                    assert R(self.lib.nrdHipGetPoolPlaneLayer(self.handle, int(pool), i, layer, C.byref(d))) == R.SUCCESS, self.error()
                out.append(_read_device(d.data, d.height * d.rowPitchBytes).reshape(d.height, d.rowPitchBytes))
        return out

    def destroy(self):
        if self.handle:
            self.lib.nrdHipDestroyExecutor(self.handle)
            self.handle = None
        self.inst.destroy()


def _texel_bytes(fmt):
    return api.FORMAT_BYTES[F(fmt)]


def _np(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def layer_planes(rt, plane):
    """the N layers of a per-layer input: the scene's, every pixel lit (IN_PENUMBRA; the scene's IN_TRANSLUCENCY), the scene's flipped left-right"""
    plane = _np(plane)
    middle = np.full_like(plane, LIT) if rt == RT.IN_PENUMBRA else plane
    return [plane, middle, np.ascontiguousarray(plane[:, ::-1])]


@functools.lru_cache(maxsize=None)
def _sequence(name, frames):
    return parity.generate_sequence(name, W, H, frames)


def _embed(plane, resource, origin, sentinel):
    """the rect-sized plane at `origin` of a resource-sized one"""
    plane = _np(plane)
    big = np.full((resource[1], resource[0]) + plane.shape[2:], sentinel, dtype=plane.dtype)
    big[origin[1]: origin[1] + plane.shape[0], origin[0]: origin[0] + plane.shape[1]] = plane
    return big


OUTSIDE = 0x3C  # dynamic resolution: what the output texels outside the rect hold before the first frame


def run_case(name, frames, overrides=None, resource=None, origin=(0, 0), graph=False, separate=True):
    """Runs `frames` frames through one layered executor (N layers) and, with separate=True, through N unlayered executors with their own instances; after EVERY frame the
    outputs and every pool plane of every layer must be byte-equal and the stamps intact. Returns, per frame, (the N output planes, the pool planes per layer, graph stats)."""
    seq = _sequence(name, frames)
    rw, rh = resource or (W, H)
    (out_rt, _, out_ch, out_fmt), = parity.output_planes(name, W, H)
    cs_kw = dict(resourceSize=(rw, rh), resourceSizePrev=(rw, rh), rectOrigin=origin) if resource else {}
    layered = Run(name, rw, rh, layers=N)
    assert layered.created == R.SUCCESS and layered.layers_num() == N
    singles = [Run(name, rw, rh) for _ in range(N if separate else 0)]
    if graph:
        assert R(layered.lib.nrdHipSetGraphMode(layered.handle, 1)) == R.SUCCESS

    def out_stack(n):
        s = Stack(n, rh, rw, out_ch, fill=OUTSIDE if resource else 0)
        if resource:
            s.upload([_embed(np.zeros((H, W, out_ch), np.uint8), resource, (0, 0), OUTSIDE)] * n)
        return s

    out_layered, out_single = out_stack(N), [out_stack(1) for _ in singles]
    assert layered.bind_layers(out_rt, out_layered, out_fmt) == R.SUCCESS, layered.error()
    for run, s in zip(singles, out_single):
        assert run.bind(out_rt, s, out_fmt) == R.SUCCESS, run.error()
    stacks, results = {}, []
    for f, frame in enumerate(seq):
        for rt, t, fmt in parity.user_planes(name, frame):
            per_layer = rt in (RT.IN_PENUMBRA, RT.IN_TRANSLUCENCY)
            planes = layer_planes(rt, t) if per_layer else [_np(t)]
            if resource:  # the guides live at rectOrigin inside their planes, the noisy inputs at (0, 0)
                planes = [_embed(p, resource, (0, 0) if per_layer else origin, 33) for p in planes]
            if rt not in stacks:
                stacks[rt] = Stack(len(planes), rh, rw, _texel_bytes(fmt))
            stacks[rt].upload(planes)
            if per_layer:
                assert layered.bind_layers(rt, stacks[rt], fmt) == R.SUCCESS, layered.error()
            else:
                assert layered.bind(rt, stacks[rt], fmt) == R.SUCCESS, layered.error()
            for l, run in enumerate(singles):
                assert run.bind(rt, stacks[rt], fmt, layer=l if per_layer else 0) == R.SUCCESS, run.error()
        cam, cam_prev = frame["camera"], seq[max(f - 1, 0)]["camera"]
        for run in [layered] + singles:
            run.settings(parity.common_settings(cam, cam_prev, W, H, f, **cs_kw), parity.denoiser_settings(name, frame, overrides))
            assert run.denoise() == R.SUCCESS, run.error()
        got, intact = out_layered.layers()
        assert intact, "frame %d: a byte between / behind the layers of OUT_SHADOW_TRANSLUCENCY was written" % f
        pools = [layered.pool_planes(layer=l) for l in range(N)]
        for l, (run, s) in enumerate(zip(singles, out_single)):
            (want,), single_intact = s.layers()
            assert single_intact
            assert np.array_equal(got[l], want), "frame %d layer %d: OUT_SHADOW_TRANSLUCENCY differs from the separate run in %d bytes" % (f, l, int(np.sum(got[l] != want)))
            for i, (a, b) in enumerate(zip(pools[l], run.pool_planes())):
                assert np.array_equal(a, b), "frame %d layer %d: pool plane %d differs from the separate run in %d bytes" % (f, l, i, int(np.sum(a != b)))
        for rt, s in stacks.items():  # the inputs: untouched, stamps and texels
            assert np.array_equal(s.buf.read(), s.host), "frame %d: input %s was written" % (f, rt.name)
        if resource and f == 0:
            # frame 0 holds the Clear_* dispatches of a history reset, which cover whole planes on any executor: what the passes proper leave alone shows from here on
            for s in [out_layered] + out_single:
                s.stamp_outside(W, H, OUTSIDE)
        stats = None
        if graph:
            a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
            assert R(layered.lib.nrdHipGetGraphStats(layered.handle, C.byref(a), C.byref(b), C.byref(c))) == R.SUCCESS
            stats = (a.value, b.value, c.value)
        results.append((got, pools, stats))
    assert np.array_equal(pools[0][0], layered.pool_planes()[0])  # nrdHipGetPoolPlane keeps describing layer 0
    for run in [layered] + singles:
        run.destroy()
    assert len(np.unique(results[-1][0][0])) > 2 and not np.array_equal(results[-1][0][0], results[-1][0][2])  # denoised shadows, and different ones per layer
    return results


@functools.lru_cache(maxsize=None)
def case_default():
    """case 1, shared: SIGMA_SHADOW, default stabilisation, 4 frames"""
    return run_case("SIGMA_SHADOW", 4)


# ------------------------------------------------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.gpu
def test_layered_equals_separate_default_stabilisation():
    """1. 4 frames of SIGMA_SHADOW with the default temporal stabilisation -- per-light history in one instance: every frame, every layer, every pool plane (asserted inside)"""
    results = case_default()
    assert len(results) == 4
    lit = results[-1][0][1]
    assert set(np.unique(lit)) <= {0, 255}, "the all-lit layer holds lit pixels and untouched sky only: it shares nothing with its neighbours"


@pytest.mark.gpu
def test_layered_equals_separate_without_stabilisation():
    """2. the same with maxStabilizedFrameNum = 0 (no TemporalStabilization pass in the list), 2 frames"""
    run_case("SIGMA_SHADOW", 2, overrides=dict(maxStabilizedFrameNum=0))


@pytest.mark.gpu
def test_layered_equals_separate_translucency():
    """3. SIGMA_SHADOW_TRANSLUCENCY (RGBA8 output, IN_TRANSLUCENCY per layer, flipped with its penumbra), 3 frames"""
    run_case("SIGMA_SHADOW_TRANSLUCENCY", 3)


@pytest.mark.gpu
def test_one_layer_against_the_cpu_oracle():
    """4. layer 2 of case 1 against the CPU oracle run on that layer's inputs, within parity.REL_TOL: independent of the unlayered GPU path"""
    results = case_default()
    seq = _sequence("SIGMA_SHADOW", 4)
    import torch

    ora = parity.OracleRun("SIGMA_SHADOW", W, H)
    for f, frame in enumerate(seq):
        flipped = dict(frame)
        flipped["penumbra"] = torch.from_numpy(layer_planes(RT.IN_PENUMBRA, frame["penumbra"])[2])
        ora.step(flipped, parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], W, H, f), parity.denoiser_settings("SIGMA_SHADOW", frame))
        want = ora.output(RT.OUT_SHADOW_TRANSLUCENCY).reshape(H, W)
        e = parity.rel_error(results[f][0][2].astype(np.float32).reshape(H, W), want)
        print("frame %d: layer 2 vs the oracle, max relative error %g" % (f, e))
        assert e <= parity.REL_TOL, "frame %d: layer 2 vs the oracle: %g" % (f, e)


@pytest.mark.gpu
def test_one_layer_is_the_plain_executor():
    """5. nrdHipCreateExecutorLayered with layersNum = 1 is nrdHipCreateExecutor: same bytes over 3 frames (plain binds), nrdHipGetLayersNum 1, the same pool memory; 3 layers: 3x"""
    name = "SIGMA_SHADOW"
    seq = _sequence(name, 4)[:3]
    runs = [Run(name, W, H, layers=1), Run(name, W, H), Run(name, W, H, layers=N)]
    assert all(r.created == R.SUCCESS for r in runs)
    assert [r.layers_num() for r in runs] == [1, 1, N]
    assert runs[0].pool_memory() == runs[1].pool_memory() and runs[1].pool_memory()[0] > 0
    assert runs[2].pool_memory() == tuple(N * v for v in runs[1].pool_memory())
    outs = [Stack(1, H, W, 1) for _ in range(2)]
    stacks = {}
    for f, frame in enumerate(seq):
        for rt, t, fmt in parity.user_planes(name, frame):
            stacks.setdefault(rt, Stack(1, H, W, _texel_bytes(fmt))).upload([_np(t)])
        for run, out in zip(runs[:2], outs):
            for rt, _, fmt in parity.user_planes(name, frame):
                assert run.bind(rt, stacks[rt], fmt) == R.SUCCESS, run.error()
            assert run.bind(RT.OUT_SHADOW_TRANSLUCENCY, out, F.R8_UNORM) == R.SUCCESS, run.error()
            run.settings(parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], W, H, f), parity.denoiser_settings(name, frame))
            assert run.denoise() == R.SUCCESS, run.error()
        (a,), ia = outs[0].layers()
        (b,), ib = outs[1].layers()
        assert ia and ib and np.array_equal(a, b), "frame %d" % f
        assert all(np.array_equal(p, q) for p, q in zip(runs[0].pool_planes(), runs[1].pool_planes())), "frame %d: pool planes" % f
        assert all(np.array_equal(p, q) for p, q in zip(runs[0].pool_planes(layer=0), runs[1].pool_planes())), "frame %d: nrdHipGetPoolPlaneLayer( 0 )" % f
    assert len(np.unique(a)) > 2
    for r in runs:
        r.destroy()


@pytest.mark.gpu
def test_dynamic_resolution_shifted_rect():
    """6. resource 96 x 64, rect 83 x 45 at origin (5, 7), 3 layers, 2 frames: only the shared guides get rect-at-origin twins; equal to the separate runs (whole planes: inside
    the rect and outside), and the output texels outside the rect keep what they held. The Clear_* dispatches of frame 0 (history reset) cover the whole output plane
    on every executor, so the texels outside the rect are stamped again behind frame 0 and must survive the frame after it."""
    results = run_case("SIGMA_SHADOW", 2, resource=(96, 64), origin=(5, 7))
    for layer in results[1][0]:
        assert np.all(layer[H:] == OUTSIDE) and np.all(layer[:, W:] == OUTSIDE), "an output texel outside the rect was written"
    assert len(np.unique(results[-1][0][0][:H, :W])) > 2


@pytest.mark.gpu
def test_graph_mode_layered():
    """7. graph mode (launch records carry the grid, z extent included) over 3 frames: the bytes of the eager run, one graph built per topology"""
    eager = case_default()
    graph = run_case("SIGMA_SHADOW", 4, graph=True, separate=False)
    for f in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(graph[f][0], eager[f][0])), "frame %d: outputs" % f
        for l in range(N):
            assert all(np.array_equal(a, b) for a, b in zip(graph[f][1][l], eager[f][1][l])), "frame %d layer %d: pool planes" % (f, l)
    launches, builds, _ = graph[-1][2]
    assert launches == 4, graph[-1][2]
    # one graph per topology = per distinct sequence of kernels: the lists of the four frames, fetched from a host-only instance fed the same settings (the first frame's
    # list holds Clear_* dispatches -- both of which launch the one clear kernel --, the ping-pong phases behind it differ in planes only)
    seq, name = _sequence("SIGMA_SHADOW", 4), "SIGMA_SHADOW"
    inst = api.Instance([(0, parity.DENOISERS[name][0])], lib=_lib())
    topologies = set()
    for f, frame in enumerate(seq):
        assert inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame)) == R.SUCCESS
        assert inst.set_common_settings(parity.common_settings(frame["camera"], seq[max(f - 1, 0)]["camera"], W, H, f)) == R.SUCCESS
        r, dispatches = inst.get_compute_dispatches()
        assert r == R.SUCCESS
        topologies.add(tuple("Clear" if d.shader.startswith("Clear_") else d.shader for d in dispatches))
    inst.destroy()
    assert builds == len(topologies), (graph[-1][2], topologies)


# ------------------------------------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals_touch_nothing():
    """8. every refusal returns its documented code, leaves a message where an executor exists, and enqueues nothing: the output stack keeps its stamps AND its texels"""
    name = "SIGMA_SHADOW"
    lib = _lib()
    frame = _sequence(name, 4)[0]
    for bad in (0, 33):
        run = Run(name, W, H, layers=bad)
        assert run.created == R.INVALID_ARGUMENT and not run.handle, bad
        run.inst.destroy()
    reblur = Run("REBLUR_DIFFUSE", W, H, layers=2)
    assert reblur.created == R.UNSUPPORTED and not reblur.handle
    reblur.inst.destroy()

    run, plain = Run(name, W, H, layers=N), Run(name, W, H)
    assert run.created == R.SUCCESS and plain.created == R.SUCCESS
    out = Stack(N, H, W, 1, fill=0x11)
    pen = Stack(N, H, W, 2)
    pen.upload(layer_planes(RT.IN_PENUMBRA, frame["penumbra"]))
    guides = {}
    for rt, t, fmt in parity.user_planes(name, frame):
        if rt != RT.IN_PENUMBRA:
            guides[rt] = (Stack(1, H, W, _texel_bytes(fmt)), fmt)
            guides[rt][0].upload([_np(t)])

    def refused(code, want, who=run):
        assert code == want, (code, want, who.error())
        assert who.error(), "no message"

    refused(run.bind(RT.IN_PENUMBRA, pen, F.R16_SFLOAT), R.INVALID_ARGUMENT)
    assert "IN_PENUMBRA" in run.error()
    refused(run.bind_layers(RT.IN_VIEWZ, guides[RT.IN_VIEWZ][0], F.R32_SFLOAT), R.INVALID_ARGUMENT)
    refused(plain.bind_layers(RT.IN_PENUMBRA, pen, F.R16_SFLOAT), R.INVALID_ARGUMENT, plain)
    refused(run.bind_layers(RT.IN_PENUMBRA, pen, F.R16_SFLOAT, layer_bytes=pen.pitch * H - 4), R.INVALID_ARGUMENT)
    refused(run.bind_layers(RT.IN_PENUMBRA, pen, F.R16_SFLOAT, layer_bytes=pen.pitch * H + 2), R.INVALID_ARGUMENT)
    # nothing was bound by the refused calls: the frame cannot run, and says which slot is missing
    for rt, (s, fmt) in guides.items():
        assert run.bind(rt, s, fmt) == R.SUCCESS, run.error()
    assert run.bind_layers(RT.OUT_SHADOW_TRANSLUCENCY, out, F.R8_UNORM) == R.SUCCESS, run.error()
    run.settings(parity.common_settings(frame["camera"], frame["camera"], W, H, 0), parity.denoiser_settings(name, frame))
    refused(run.denoise(), R.INVALID_ARGUMENT)
    assert "IN_PENUMBRA" in run.error()
    assert run.bind_layers(RT.IN_PENUMBRA, pen, F.R16_SFLOAT) == R.SUCCESS, run.error()

    d = api.HipPlaneDesc()
    refused(R(lib.nrdHipGetPoolPlaneLayer(run.handle, int(RT.PERMANENT_POOL), 0, N, C.byref(d))), R.INVALID_ARGUMENT)
    refused(R(lib.nrdHipSetOwnedRows(run.handle, 0, H - 1)), R.UNSUPPORTED)
    refused(R(lib.nrdHipSetOwnedRows(run.handle, 8, H)), R.UNSUPPORTED)
    assert R(lib.nrdHipSetOwnedRows(run.handle, 0, H)) == R.SUCCESS  # the whole frame is no restriction
    r, ptr, num = run.inst.get_compute_dispatches_raw([0])
    assert r == R.SUCCESS and num > 0
    rows0, rows1 = (C.c_int32 * num)(*[0] * num), (C.c_int32 * num)(*[H] * num)
    refused(R(lib.nrdHipExecuteDispatchRange(run.handle, C.cast(ptr, C.c_void_p), num, 0, num, rows0, rows1)), R.UNSUPPORTED)
    report, mask = api.HipInputReport(), C.c_uint32()
    refused(R(lib.nrdHipCheckInputs(run.handle, C.cast(ptr, C.c_void_p), num, C.byref(report), C.byref(mask))), R.UNSUPPORTED)
    scratch = Buf(np.zeros(C.sizeof(api.HipInputReport), np.uint8))
    refused(R(lib.nrdHipCheckInputsAsync(run.handle, C.cast(ptr, C.c_void_p), num, C.c_void_p(scratch.ptr), C.byref(mask))), R.UNSUPPORTED)
    assert not scratch.read().any(), "the refused audit cleared its report: something was enqueued"

    got, intact = out.layers()
    assert intact and all(np.all(layer == 0x11) for layer in got), "a refused call ran something"
    # ... and the executor still works: the list fetched above runs as a whole
    assert R(lib.nrdHipExecuteDispatchRange(run.handle, C.cast(ptr, C.c_void_p), num, 0, num, None, None)) == R.SUCCESS, run.error()
    got, intact = out.layers()
    assert intact and not all(np.all(layer == 0x11) for layer in got)
    run.destroy()
    plain.destroy()


# ------------------------------------------------------------------------------------------------------------------------------------------------ the public Python path
@pytest.mark.gpu
def test_front_to_back_through_the_python_path():
    """9. frontend.pack_shadow_lights (3 lights) -> HipExecutor(layers=3).bind_packed + frontend.shadow_stack -> denoise() -> frontend.resolve_shadow_lights equals the documented
    loop over the lights (one unlayered executor, stabilisation off) byte for byte"""
    if EMU:
        pytest.skip("HipExecutor binds torch.cuda tensors: the public Python path needs a GPU (the C-ABI under it is emulated by the other tests)")
    import torch

    from raytracingdenoiser_amd import frontend
    from raytracingdenoiser_amd.executor import HipExecutor

    name, n = "SIGMA_SHADOW", 3
    frame = _sequence(name, 4)[0]
    rng = np.random.RandomState(7)
    z = np.abs(_np(frame["viewz"])).reshape(H, W)
    d = (rng.uniform(0.05, 4.0, (n, H, W)) * (1.0 + 0.05 * z)).astype(np.float32)
    d[rng.uniform(size=(n, H, W)) < 0.4] = LIT
    d[0, :, : W // 3], d[2, :, 2 * W // 3:] = LIT, 0.0
    lights = [(api.LightType.LOCAL, 0.5), (api.LightType.DIRECTIONAL, 0.02), (api.LightType.LOCAL, 2.0)]
    lighting = torch.from_numpy(rng.uniform(0.0, 3.0, (n, H, W, 4)).astype(np.float32)).cuda()
    packed = frontend.pack_shadow_lights(lights, torch.from_numpy(d).cuda(), distance_to_light=torch.from_numpy(d + 5.0).cuda())
    guides = [(rt, t.cuda().contiguous(), fmt) for rt, t, fmt in parity.user_planes(name, frame) if rt != RT.IN_PENUMBRA]
    off = dict(maxStabilizedFrameNum=0)

    def prepare(ex, inst):
        for rt, t, fmt in guides:
            ex.bind(rt, t, fmt)
        assert inst.set_denoiser_settings(0, parity.denoiser_settings(name, frame, off)) == R.SUCCESS
        assert inst.set_common_settings(parity.common_settings(frame["camera"], frame["camera"], W, H, 0)) == R.SUCCESS

    # layered
    inst = api.Instance([(0, parity.DENOISERS[name][0])])
    ex = HipExecutor(inst, W, H, layers=n)
    assert ex.layers_num() == n
    shadows = frontend.shadow_stack(lighting, n, H, W)
    shadows.zero_()
    ex.bind_packed({RT.IN_PENUMBRA: packed[RT.IN_PENUMBRA], RT.OUT_SHADOW_TRANSLUCENCY: (shadows, F.R8_UNORM)})
    prepare(ex, inst)
    ex.denoise()
    lit = frontend.resolve_shadow_lights(shadows, lighting)
    torch.cuda.synchronize()
    host, _, _ = ex.read_pool_plane(RT.PERMANENT_POOL, 0, layer=2)
    assert np.array_equal(ex.pool_plane_tensor(RT.PERMANENT_POOL, 0, layer=2).cpu().numpy(), host)
    ex.destroy()
    # the documented loop
    inst = api.Instance([(0, parity.DENOISERS[name][0])])
    ex = HipExecutor(inst, W, H)
    loop = frontend.shadow_stack(lighting, n, H, W)
    loop.zero_()
    for i in range(n):
        ex.bind(RT.IN_PENUMBRA, packed[RT.IN_PENUMBRA][0][i], F.R16_SFLOAT)
        ex.bind(RT.OUT_SHADOW_TRANSLUCENCY, loop[i], F.R8_UNORM)
        prepare(ex, inst)
        ex.denoise()
    want = frontend.resolve_shadow_lights(loop, lighting)
    torch.cuda.synchronize()
    ex.destroy()
    assert np.array_equal(shadows.cpu().numpy(), loop.cpu().numpy()), "the shadow layers"
    assert np.array_equal(lit.cpu().numpy(), want.cpu().numpy()), "the resolved radiance"
    assert len(np.unique(shadows.cpu().numpy())) > 2


# ------------------------------------------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_are_exported_and_declared():
    lib = api.load_library()
    for symbol in ("nrdHipCreateExecutorLayered", "nrdHipBindResourceLayers", "nrdHipGetPoolPlaneLayer", "nrdHipGetLayersNum"):
        assert symbol in api.NRD_HIP_SYMBOLS
        assert getattr(lib, symbol)
    # argument checks that need no device
    assert R(lib.nrdHipGetLayersNum(None, C.byref(C.c_uint32()))) == R.INVALID_ARGUMENT
    d = api.HipPlaneDesc()
    assert R(lib.nrdHipBindResourceLayers(None, int(RT.IN_PENUMBRA), C.byref(d), 4)) == R.INVALID_ARGUMENT
    assert R(lib.nrdHipGetPoolPlaneLayer(None, int(RT.PERMANENT_POOL), 0, 0, C.byref(d))) == R.INVALID_ARGUMENT
    inst = api.Instance([(0, api.Denoiser.SIGMA_SHADOW)])
    handle = C.c_void_p()
    for bad in (0, 33):
        assert R(lib.nrdHipCreateExecutorLayered(inst.handle, W, H, bad, None, C.byref(handle))) == R.INVALID_ARGUMENT and not handle
    inst.destroy()
