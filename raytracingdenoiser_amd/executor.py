"""Plumbing over include/NRDHip.h: device memory comes from torch (ROCm), everything else is the C-ABI.

There is no CPU path here: creating an executor without a visible GPU raises.
"""
import ctypes as C

import numpy as np

from . import api

_hip = None


def _hip_runtime():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    return _hip


def texel_bytes(fmt):
    return api.FORMAT_BYTES[api.Format(fmt)]


class _DeviceBytes:
    """device memory the library owns, as torch.as_tensor takes it (the CUDA array interface): the pool arena of a layered executor"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


PER_LAYER_SLOTS = (api.ResourceType.IN_PENUMBRA, api.ResourceType.IN_TRANSLUCENCY, api.ResourceType.OUT_SHADOW_TRANSLUCENCY)


class HipExecutor:
    """One nrd::Instance bound to pool planes in HBM; launches the pass chain on `stream` (a torch.cuda.Stream or None).
    layers > 1 (an instance of SIGMA denoisers only): `layers` shadow layers, one per light, denoised by one pass chain -- include/NRDHip.h nrdHipCreateExecutorLayered.
    The per-layer slots (PER_LAYER_SLOTS) are then bound as [N, H, W(, C)] stacks with bind_layers, the guides with bind as ever; the pool belongs to the library."""

    def __init__(self, instance, width, height, stream=None, layers=1):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("NRD HIP executor needs a GPU (no CPU fallback exists)")
        self.instance = instance
        self.lib = instance.lib
        self.width, self.height = width, height
        self.stream = stream
        self.layers = layers
        handle = C.c_void_p()
        stream_ptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._bound = {}  # keeps tensors alive
        self._checked_list = None  # (identifiers, pointer, count, instance.list_generation): the list check_inputs fetched for the denoise() that follows
        if layers != 1:  # (a caller-provided arena stays unlayered: the library allocates the layered pool)
            self.arena = None
            r = api.Result(self.lib.nrdHipCreateExecutorLayered(instance.handle, width, height, layers, stream_ptr, C.byref(handle)))
            if r != api.Result.SUCCESS:
                raise RuntimeError("nrdHipCreateExecutorLayered(%d layers) failed: %s" % (layers, r.name))
            self.handle = handle
            return
        # the pool arena is a torch allocation, so pool planes can be aliased as tensors (needed for the RCCL all-gather)
        size = self.lib.nrdHipGetArenaSize(instance.handle, width, height)
        self.arena = torch.zeros(max(size, 256), dtype=torch.uint8, device="cuda")
        assert self.arena.data_ptr() % 256 == 0
        r = api.Result(self.lib.nrdHipCreateExecutorWithArena(instance.handle, width, height, stream_ptr, self.arena.data_ptr(), size, C.byref(handle)))
        if r != api.Result.SUCCESS:
            raise RuntimeError("nrdHipCreateExecutorWithArena failed: %s" % r.name)
        self.handle = handle

    def _check(self, code, what):
        r = api.Result(code)
        if r != api.Result.SUCCESS:
            raise RuntimeError("%s failed: %s (%s)" % (what, r.name, self.lib.nrdHipGetLastError(self.handle).decode()))

    def bind(self, resource_type, tensor, fmt):
        """tensor: CUDA tensor whose rows are the plane rows (any dtype; [H, W, C] or [H, W]); rows must be dense, the row pitch may exceed
        the row size (e.g. a [:, :W] view of a wider allocation)."""
        assert tensor.is_cuda and tensor[0].is_contiguous()
        pitch = tensor.stride(0) * tensor.element_size()
        desc = api.HipPlaneDesc(tensor.data_ptr(), pitch, int(fmt), self.width, self.height)
        self._check(self.lib.nrdHipBindResource(self.handle, int(resource_type), C.byref(desc)), "nrdHipBindResource(%s)" % api.ResourceType(resource_type).name)
        self._bound[int(resource_type)] = tensor

    def bind_layers(self, resource_type, tensor, fmt):
        """a per-layer slot of a layered executor: tensor [N, H, W(, C)] with N == layers, layer l = tensor[l]; the layers may lie further apart than their size (stride(0)
        is the layerBytes of nrdHipBindResourceLayers), e.g. frontend.shadow_stack or a [:, :H] view of a taller stack"""
        assert tensor.is_cuda and tensor.shape[0] == self.layers and tensor[0][0].is_contiguous()
        pitch = tensor.stride(1) * tensor.element_size()
        desc = api.HipPlaneDesc(tensor.data_ptr(), pitch, int(fmt), self.width, self.height)
        self._check(self.lib.nrdHipBindResourceLayers(self.handle, int(resource_type), C.byref(desc), tensor.stride(0) * tensor.element_size()),
                    "nrdHipBindResourceLayers(%s)" % api.ResourceType(resource_type).name)
        self._bound[int(resource_type)] = tensor

    def bind_packed(self, packed):
        """binds what frontend.pack_inputs returned: {ResourceType: (tensor, Format)}; on a layered executor the per-layer slots are taken as stacks (bind_layers)"""
        for resource_type, (tensor, fmt) in packed.items():
            if self.layers > 1 and int(resource_type) in [int(t) for t in PER_LAYER_SLOTS]:
                self.bind_layers(resource_type, tensor, fmt)
            else:
                self.bind(resource_type, tensor, fmt)

    def resolve(self, diffuse_mode=None, specular_mode=None, resolve=0, shadow=False, **kw):
        """frontend.resolve_outputs on the planes bound to this executor: the OUT_* planes of the given signal modes (frontend.SignalMode; `resolve` = frontend.ResolveMode for the
        SH modes), OUT_SHADOW_TRANSLUCENCY with shadow=True, IN_NORMAL_ROUGHNESS / IN_VIEWZ where bound, the camera of the last SetCommonSettings, on the executor's stream.
        Further keywords (albedo, rf0, remodulate, denormalize_hit_dist, want, out, channels=3 for [H, W, 3] colour outputs, ...) are passed on. Returns fp32 tensors by name."""
        from . import frontend

        args = dict(normal_roughness=self._bound.get(int(api.ResourceType.IN_NORMAL_ROUGHNESS)), viewz=self._bound.get(int(api.ResourceType.IN_VIEWZ)),
                    common_settings=getattr(self.instance, "last_common_settings", None), stream=self.stream, lib=self.lib)
        for which, mode in (("diffuse", diffuse_mode), ("specular", specular_mode)):
            if mode:
                slot0, slot1 = frontend.signal_slots(which, mode, "OUT")
                args[which] = dict(mode=mode, resolve=resolve, in0=self._bound[int(slot0)], in1=self._bound[int(slot1)] if slot1 is not None else None)
        if shadow:
            args["shadow"] = self._bound[int(api.ResourceType.OUT_SHADOW_TRANSLUCENCY)]
        args.update(kw)
        return frontend.resolve_outputs(**args)

    def denoise(self, identifiers=None):
        ids = identifiers if identifiers is not None else self.instance.identifiers
        checked, self._checked_list = self._checked_list, None
        if checked is not None and checked[0] == list(ids) and checked[3] == self.instance.list_generation:
            # check_inputs fetched this frame's list already (nrd::GetComputeDispatches advances the instance's ping-pong state: once per frame): execute that very list.
            # Only while nothing happened to the instance since -- new settings or another fetch make the list stale (a dropped frame, settings changed after the check),
            # and this frame's is fetched below as if there had been no check.
            self.execute_raw(checked[1], checked[2])
            return
        arr = (C.c_uint32 * len(ids))(*ids)
        self._check(self.lib.nrdHipDenoise(self.handle, arr, len(ids)), "nrdHipDenoise")

    def check_inputs(self, identifiers=None, raise_on_violation=False, dispatches=None):
        """Audits the bound inputs against NRD's input rules before the frame is denoised -- include/NRDHip.h nrdHipCheckInputs: one launch, a stream synchronisation and a
        72-byte read-back. Call it after set_common_settings / set_denoiser_settings of the frame. Returns an api.InputCheck: truthy when clean, `rules` = {name: (count,
        first (x, y) or None)} per checked rule; raise_on_violation=True raises ValueError naming rule, count and first pixel instead.
        The frame's dispatch list is fetched here, and the denoise() that follows with the same identifiers executes that list instead of fetching it again -- unless
        settings were set or a list was fetched on the instance in between: then the held list is stale, it is dropped and denoise() fetches its own. A fetched list
        is meant to be executed: a frame that is checked and then dropped has still advanced the instance's ping-pong planes, as any unexecuted GetComputeDispatches
        does, so restart the accumulation (AccumulationMode.RESTART) on the next frame. dispatches = (pointer, count) checks a list the caller fetched (and executes) itself."""
        if not hasattr(self.instance, "last_common_settings"):
            raise RuntimeError("check_inputs: call instance.set_common_settings(cs) for this frame first (the rect of the report comes from it)")
        ptr, n = self._frame_list(identifiers, dispatches)
        return api.check_inputs(self.lib, self.handle, ptr, n, int(self.instance.last_common_settings.rectSize[0]), raise_on_violation)

    def _frame_list(self, identifiers, dispatches):
        if dispatches is not None:
            return dispatches
        ids = list(identifiers if identifiers is not None else self.instance.identifiers)
        r, ptr, n = self.instance.get_compute_dispatches_raw(ids)
        if r != api.Result.SUCCESS:
            raise RuntimeError("nrd::GetComputeDispatches failed: %s" % r.name)
        self._checked_list = (ids, ptr, n, self.instance.list_generation)
        return ptr, n

    def check_inputs_async(self, device_report, identifiers=None, dispatches=None):
        """the same audit enqueued on the executor's stream: device_report (18 x int32 / uint32 or 72 x uint8 on the device) receives the NrdHipInputReport in stream order, with
        no allocation and no synchronisation (capturable into a graph) -- include/NRDHip.h nrdHipCheckInputsAsync. The list: as for check_inputs.
        Returns the mask of the rules checked (bit r = api.INPUT_RULES[r])."""
        assert device_report.is_cuda and device_report.is_contiguous() and device_report.numel() * device_report.element_size() >= C.sizeof(api.HipInputReport)
        ptr, n = self._frame_list(identifiers, dispatches)
        mask = C.c_uint32()
        self._check(self.lib.nrdHipCheckInputsAsync(self.handle, C.cast(ptr, C.c_void_p), n, C.c_void_p(device_report.data_ptr()), C.byref(mask)), "nrdHipCheckInputsAsync")
        return mask.value

    def execute_raw(self, dispatch_ptr, num):
        self._check(self.lib.nrdHipExecuteDispatches(self.handle, C.cast(dispatch_ptr, C.c_void_p), num), "nrdHipExecuteDispatches")

    def pool_plane_desc(self, pool, index, layer=0):
        desc = api.HipPlaneDesc()
        if layer == 0:
            self._check(self.lib.nrdHipGetPoolPlane(self.handle, int(pool), index, C.byref(desc)), "nrdHipGetPoolPlane")
        else:
            self._check(self.lib.nrdHipGetPoolPlaneLayer(self.handle, int(pool), index, layer, C.byref(desc)), "nrdHipGetPoolPlaneLayer")
        return desc

    def layers_num(self):
        n = C.c_uint32()
        self._check(self.lib.nrdHipGetLayersNum(self.handle, C.byref(n)), "nrdHipGetLayersNum")
        return n.value

    def read_pool_plane(self, pool, index, layer=0):
        """Synchronous device->host copy of a pool plane (of one layer): returns (uint8 ndarray [h, pitch], Format, width)."""
        import torch

        torch.cuda.synchronize()
        d = self.pool_plane_desc(pool, index, layer)
        host = np.empty((d.height, d.rowPitchBytes), dtype=np.uint8)
        err = _hip_runtime().hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(d.data), host.nbytes, 2)
        if err != 0:
            raise RuntimeError("hipMemcpy D2H failed: %d" % err)
        return host, api.Format(d.format), d.width

    def pool_plane_tensor(self, pool, index, layer=0):
        """uint8 tensor view [h, pitch] aliasing a pool plane (of one layer) inside the arena (no copy)."""
        d = self.pool_plane_desc(pool, index, layer)
        if self.arena is None:  # a layered executor: the arena belongs to the library (valid until destroy())
            import torch

            return torch.as_tensor(_DeviceBytes(d.data, d.height * d.rowPitchBytes), device="cuda").view(d.height, d.rowPitchBytes)
        off = d.data - self.arena.data_ptr()
        return self.arena[off : off + d.height * d.rowPitchBytes].view(d.height, d.rowPitchBytes)

    def execute_range(self, dispatch_ptr, num, first, count, row_begin=None, row_end=None):
        """dispatches [first, first + count) of the list; row_begin / row_end: per-dispatch rows to produce (lists of length num) or None"""
        # lists are converted per call; a caller on a hot path passes ready-made ctypes arrays (sharding.HaloPlan.c_rows)
        rb = row_begin if row_begin is None or isinstance(row_begin, C.Array) else (C.c_int32 * num)(*row_begin)
        re = row_end if row_end is None or isinstance(row_end, C.Array) else (C.c_int32 * num)(*row_end)
        self._check(self.lib.nrdHipExecuteDispatchRange(self.handle, C.cast(dispatch_ptr, C.c_void_p), num, first, count, rb, re), "nrdHipExecuteDispatchRange")

    def set_owned_rows(self, row_begin, row_end):
        self._check(self.lib.nrdHipSetOwnedRows(self.handle, row_begin, row_end), "nrdHipSetOwnedRows")

    def set_graph_mode(self, enable):
        """one hipGraph launch per dispatch range instead of one launch per pass (include/NRDHip.h nrdHipSetGraphMode)"""
        self._check(self.lib.nrdHipSetGraphMode(self.handle, 1 if enable else 0), "nrdHipSetGraphMode")

    def graph_stats(self):
        """(graph launches, graphs built, node-parameter updates)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.nrdHipGetGraphStats(self.handle, C.byref(a), C.byref(b), C.byref(c)), "nrdHipGetGraphStats")
        return a.value, b.value, c.value

    def tile_fallback_stats(self):
        """(tiles of the last frame left to a fallback kernel, tiles in total) -- include/NRDHip.h nrdHipGetTileFallbackStats"""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self.lib.nrdHipGetTileFallbackStats(self.handle, C.byref(a), C.byref(b)), "nrdHipGetTileFallbackStats")
        return a.value, b.value

    def measure_motion_rows(self, ptr, n, row_begin=0, row_end=0xFFFFFFFF):
        """largest vertical surface-motion reprojection distance (rows) over rows [row_begin, row_end) of this frame's rect -- include/NRDHip.h nrdHipMeasureMotionRows"""
        out = C.c_float()
        self._check(self.lib.nrdHipMeasureMotionRows(self.handle, C.cast(ptr, C.c_void_p), n, row_begin, min(row_end, 0xFFFFFFFF), C.byref(out)), "nrdHipMeasureMotionRows")
        return out.value

    def measure_motion_rows_async(self, ptr, n, row_begin, row_end, device_word):
        """the same measurement enqueued on the executor's stream: the result lands in device_word (a 1-element float32 CUDA tensor) in stream order, no host synchronisation
        -- include/NRDHip.h nrdHipMeasureMotionRowsAsync. The caller all-reduces the tensor and reads it once."""
        assert device_word.is_cuda and device_word.numel() == 1 and device_word.element_size() == 4
        self._check(self.lib.nrdHipMeasureMotionRowsAsync(self.handle, C.cast(ptr, C.c_void_p), n, row_begin, min(row_end, 0xFFFFFFFF), C.c_void_p(device_word.data_ptr())),
                    "nrdHipMeasureMotionRowsAsync")

    def set_history_reach_word(self, device_word):
        """device_word: a 1-element float32 CUDA tensor (kept alive by the caller) the temporal passes report their history reach into (rows; atomicMax) -- or None to switch the
        tracking off. include/NRDHip.h nrdHipSetHistoryReachWord."""
        assert device_word is None or (device_word.numel() == 1 and device_word.element_size() == 4)
        self._check(self.lib.nrdHipSetHistoryReachWord(self.handle, C.c_void_p(device_word.data_ptr() if device_word is not None else 0)), "nrdHipSetHistoryReachWord")

    def set_profiling(self, enable):
        self._check(self.lib.nrdHipSetProfiling(self.handle, 1 if enable else 0), "nrdHipSetProfiling")

    def collect_pass_timings(self):
        """{shaderFileName: (total_ms, launches)} for all dispatches since the last collect (synchronises the stream)."""
        n = len(self.instance.pipelines) + 1  # + the per-frame guide preparation (decode / shift kernels in front of the first pass), reported under GUIDE_PREPARATION
        idx, ms, cnt, written = (C.c_uint32 * n)(), (C.c_double * n)(), (C.c_uint32 * n)(), C.c_uint32()
        self._check(self.lib.nrdHipCollectPassTimings(self.handle, idx, ms, cnt, n, C.byref(written)), "nrdHipCollectPassTimings")
        names = list(self.instance.pipelines) + [self.GUIDE_PREPARATION]
        return {names[idx[i]]: (ms[i], cnt[i]) for i in range(written.value)}

    # absent (0 launches) when the tile-classification kernel of the list writes the guide planes itself: single-GPU REBLUR / RELAX lists (include/NRDHip.h)
    GUIDE_PREPARATION = "(guide planes: DecodeGuidesKernel)"

    def pool_memory(self):
        p, t = C.c_uint64(), C.c_uint64()
        self._check(self.lib.nrdHipGetPoolMemoryUsage(self.handle, C.byref(p), C.byref(t)), "nrdHipGetPoolMemoryUsage")
        return p.value, t.value

    def destroy(self):
        if self.handle:
            self.lib.nrdHipDestroyExecutor(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
