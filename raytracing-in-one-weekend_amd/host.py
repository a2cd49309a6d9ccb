"""Host-side mirror of the reference's job structs for this path, above the C ABI.

The reference's host is C# (Unity); no C# toolchain exists in this image, so the mirror is Python (ctypes) and keeps
the reference's names and argument meaning so that tests read like the reference's call site
(Assets/Scripts/Unity/Raytracer.cs:674-738):

    job = SampleBatchJob(context, Size=..., View=..., Seed=..., SampleCountRange=..., TraceDepth=..., ...)
    job.InputColor = ...; job.OutputColor = ...
    job.Schedule().Complete()

`Context` owns the device state (scene, staging); `DeviceBuffer` mirrors CudaBuffer
(Assets/ThirdParty/nVidia OptiX Denoiser/OptixApi.cs:226-251).
"""
import ctypes as C

import numpy as np

from . import abi
from .lib import check, load


class DeviceBuffer:
    """Device allocation with Allocate / Copy / EnsureCapacity semantics of CudaBuffer (OptixApi.cs:226-251)."""

    def __init__(self, context, nbytes=0):
        self.context = context
        self.handle = C.c_void_p(0)
        self.nbytes = 0
        if nbytes:
            self.ensure_capacity(nbytes)

    def ensure_capacity(self, nbytes):
        if nbytes <= self.nbytes and self.handle:
            return
        self.free()
        h = C.c_void_p()
        check(load().rtowDeviceAlloc(self.context.handle, nbytes, C.byref(h)), "rtowDeviceAlloc")
        self.handle, self.nbytes = h, nbytes

    def upload(self, array):
        a = np.ascontiguousarray(array)
        self.ensure_capacity(a.nbytes)
        check(load().rtowDeviceCopy(self.context.handle, a.ctypes.data, self.handle, a.nbytes, abi.MEMCPY_HOST_TO_DEVICE), "rtowDeviceCopy")
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        check(load().rtowDeviceCopy(self.context.handle, self.handle, out.ctypes.data, out.nbytes, abi.MEMCPY_DEVICE_TO_HOST), "rtowDeviceCopy")
        return out

    def zero(self):
        check(load().rtowDeviceMemset(self.context.handle, self.handle, 0, self.nbytes), "rtowDeviceMemset")
        return self

    def free(self):
        if self.handle:
            load().rtowDeviceFree(self.context.handle, self.handle)
        self.handle, self.nbytes = C.c_void_p(0), 0

    @property
    def ptr(self):
        return self.handle.value


def _ray_array(rays):
    """`rays` as the ray queries take them - an array of abi.RAY_DTYPE, or (n, 8) float32: origin, time, direction, pad - contiguous, and how many: (array, count)"""
    a = np.ascontiguousarray(rays)
    if a.dtype != np.dtype(abi.RAY_DTYPE):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 8)
    return a, int(a.shape[0])


class Context:
    """RtowContext: one per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device_ordinal=0, log=None, log_level=0, flags=0, lds_scene_budget=0, scheduler_tune=None, hit_list_capacity=0, slice_block_threads=0):
        """flags: abi.CONTEXT_* (RtowContextFlags); lds_scene_budget / scheduler_tune: the development knobs of RtowContextOptions;
        hit_list_capacity: most surfaces one ray may meet where the whole hit list is kept (0 = 1024)."""
        self._cb = abi.LogCallback(log) if log else abi.LogCallback()
        opts = abi.ContextOptions(device_ordinal, self._cb, None, log_level, flags, lds_scene_budget)
        if scheduler_tune is not None:
            if len(scheduler_tune) != 9:
                raise ValueError("scheduler_tune takes 8 stage thresholds + the box-walk slice")
            for i, v in enumerate(scheduler_tune):
                opts.schedulerTune[i] = int(v)
        opts.hitListCapacity = int(hit_list_capacity)
        opts.sliceBlockThreads = int(slice_block_threads)      # reserved: 0 (or 1024); the 512- / 256-lane workgroups of round 3 were removed
        self.handle = C.c_void_p()
        check(load().rtowCreateContext(C.byref(opts), C.byref(self.handle)), "rtowCreateContext")
        self._scene_keepalive = None
        self._registered = []

    def register_host_buffers(self, *arrays):
        """Pin the host's long-lived accumulation pools (UNITY/Raytracer.cs:279-288) so that rtowSampleBatch runs without staging copies
        on the output side; the arrays must stay alive until unregister_host_buffers() / close()."""
        for a in arrays:
            check(load().rtowRegisterHostBuffer(self.handle, a.ctypes.data, a.nbytes), "rtowRegisterHostBuffer")
            self._registered.append(a)

    def unregister_host_buffers(self):
        for a in self._registered:
            load().rtowUnregisterHostBuffer(self.handle, a.ctypes.data)
        self._registered = []

    def batch_status(self):
        """Status of the batches enqueued since the last report (waits for the most recent one, wherever it was enqueued)."""
        check(load().rtowGetBatchStatus(self.handle), "rtowGetBatchStatus")

    # ---- multi-GPU: one process per GPU, rows gathered over RCCL behind the C ABI ----
    @staticmethod
    def comm_set_library_path(path):
        """rtowCommSetLibraryPath: which RCCL build rtowComm* loads (None = the default search); before the first rtowComm* call of the process."""
        check(load().rtowCommSetLibraryPath(path.encode() if path else None), "rtowCommSetLibraryPath")

    @staticmethod
    def comm_unique_id():
        cid = abi.CommId()
        check(load().rtowCommGetUniqueId(C.byref(cid)), "rtowCommGetUniqueId")
        return C.string_at(C.addressof(cid), 128)       # all 128 bytes (a c_char array's .value would stop at the first NUL)

    def comm_init(self, id_bytes, rank, world):
        cid = abi.CommId()
        C.memmove(C.addressof(cid), id_bytes, 128)
        check(load().rtowCommInit(self.handle, C.byref(cid), rank, world), "rtowCommInit")

    def comm_destroy(self):
        check(load().rtowCommDestroy(self.handle), "rtowCommDestroy")

    def gather_rows(self, width, height, divider, mine, frame, what=abi.GATHER_COLOR, root=0, stream=None):
        """mine / frame: abi.AccumBuffers of device pointers (frame may be None on non-root ranks)."""
        check(load().rtowGatherRowsDevice(self.handle, width, height, divider, C.byref(mine), C.byref(frame) if frame is not None else None, what, root, stream),
              "rtowGatherRowsDevice")

    @staticmethod
    def hybrid_plan(world, rank, tiles, samples_per_batch, step):
        """rtowHybridPlan: this rank's slice fields, sample share and Seed in a tiles x batches partition (G = T x B)."""
        plan = abi.HybridPlan()
        check(load().rtowHybridPlan(world, rank, tiles, samples_per_batch, step, C.byref(plan)), "rtowHybridPlan")
        return plan

    def exchange_accum(self, width, height, tiles, partial, accum, what=abi.GATHER_ALL, stream=None):
        """rtowExchangeAccumDevice: partial sums of this rank's tile -> folded into `accum` on the rank that owns each row (row % G)."""
        check(load().rtowExchangeAccumDevice(self.handle, width, height, tiles, C.byref(partial), C.byref(accum), what, stream), "rtowExchangeAccumDevice")

    def close(self):
        if self.handle:
            load().rtowDestroyContext(self.handle)   # drops the registrations (hipHostUnregister) while the arrays are still alive ...
            self._registered = []                    # ... and only then may they go
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, scene_desc):
        """World rebuild hand-off (the tail of Raytracer.RebuildWorld, UNITY/Raytracer.cs:1167-1183)."""
        check(load().rtowUploadScene(self.handle, C.byref(scene_desc)), "rtowUploadScene")

    def upload_sky_cubemap(self, cubemap_desc):
        """`new Cubemap(skyCubemap)` (RT/Texture.cs:150-169): the six faces travel once; None drops the cubemap."""
        check(load().rtowUploadSkyCubemap(self.handle, C.byref(cubemap_desc) if cubemap_desc is not None else None), "rtowUploadSkyCubemap")

    def upload_blue_noise(self, desc):
        """BlueNoiseData's textures (UNITY/BlueNoiseData.cs): half4 texels, `textureCount` square textures; None drops the set."""
        check(load().rtowUploadBlueNoise(self.handle, C.byref(desc) if desc is not None else None), "rtowUploadBlueNoise")

    def upload_stb_noise(self, desc):
        """SpatioTemporalBlueNoiseData's five texture sets (UNITY/SpatioTemporalBlueNoiseData.cs); None drops them."""
        check(load().rtowUploadStbNoise(self.handle, C.byref(desc) if desc is not None else None), "rtowUploadStbNoise")

    def scene_info(self):
        info = abi.SceneInfo()
        check(load().rtowGetSceneInfo(self.handle, C.byref(info)), "rtowGetSceneInfo")
        return info

    def camera_ray_list_stats(self):
        """rtowGetCameraRayListStats as a dict: entries[k] = owned pixels whose camera-ray list names k nodes, no_list, owned, pruned, valid."""
        st = abi.CameraRayListStats()
        check(load().rtowGetCameraRayListStats(self.handle, C.byref(st)), "rtowGetCameraRayListStats")
        return {"entries": [int(x) for x in st.pixelsWithEntries], "no_list": int(st.pixelsWithoutList), "owned": int(st.ownedPixels),
                "pruned": bool(st.pruned), "valid": bool(st.valid)}

    def hit_world(self, origin, direction, time=0.0):
        """Raytracer.HitWorld (UNITY/Raytracer.cs:1353; the auto-focus probe of ScheduleSample, :608-609) through rtowProbeNearestHit:
        (hit, distance, entity index) - `if hit: focusDistance = distance`."""
        d, e = C.c_float(), C.c_int32()
        o3, d3 = abi.Float3(*[float(x) for x in origin]), abi.Float3(*[float(x) for x in direction])
        check(load().rtowProbeNearestHit(self.handle, C.byref(o3), C.byref(d3), float(time), C.byref(d), C.byref(e)), "rtowProbeNearestHit")
        return e.value >= 0, d.value, e.value

    def _trace(self, count, launch, want, want_rays=False):
        """The buffers of one query: allocate those named in `want`, run `launch(hits, rays_ptr)`, wait, download."""
        kinds = {"distance": (np.float32, (count,)), "entityIndex": (np.int32, (count,)), "normal": (np.float32, (count, 3))}
        bufs = {k: DeviceBuffer(self, max(1, count) * 4 * (3 if k == "normal" else 1)) for k in kinds if k in want}
        rays = DeviceBuffer(self, max(1, count) * C.sizeof(abi.Ray)) if want_rays else None
        try:
            hits = abi.HitBuffers(*[bufs[k].handle.value if k in bufs else None for k in ("distance", "entityIndex", "normal")])
            launch(hits, rays.handle if rays else None)
            self.synchronize()
            out = {k: bufs[k].download(*kinds[k]) for k in bufs}
            if rays:
                out["rays"] = rays.download(np.dtype(abi.RAY_DTYPE), (count,))
            return out
        finally:
            for b in list(bufs.values()) + ([rays] if rays else []):
                b.free()

    def trace_rays(self, rays, want=("distance", "entityIndex", "normal"), stream=None):
        """rtowTraceRaysDevice on host data: `rays` is an array of abi.RAY_DTYPE (or (n, 8) float32: origin, time, direction, pad).
        Returns {"distance": (n,) float32, "entityIndex": (n,) int32, "normal": (n, 3) float32} for the names in `want`."""
        a, count = _ray_array(rays)
        dev = DeviceBuffer(self, max(1, count) * C.sizeof(abi.Ray))
        try:
            if count:
                dev.upload(a)
            return self._trace(count, lambda hits, _: check(load().rtowTraceRaysDevice(self.handle, count, dev.handle, C.byref(hits), stream), "rtowTraceRaysDevice"), want)
        finally:
            dev.free()

    def trace_view(self, view, width, height, time=0.0, want_rays=False, want=("distance", "entityIndex", "normal"), stream=None):
        """rtowTraceViewDevice: the first hit of every pixel centre's camera ray (pixel = row * width + col, row 0 at the bottom).
        Returns the arrays of trace_rays, plus "rays" (abi.RAY_DTYPE) with want_rays."""
        p = abi.TraceViewParams(int(width), int(height), view, float(time), 0)
        return self._trace(int(width) * int(height),
                           lambda hits, rays: check(load().rtowTraceViewDevice(self.handle, C.byref(p), C.byref(hits), rays, stream), "rtowTraceViewDevice"), want, want_rays)

    def hit_world_interval(self, origin, direction, time, tmin, tmax):
        """rtowProbeNearestHitInterval: the nearest Entity.Hit(r, tmin, tmax) of one ray, walked on the host: (hit, distance, entity index); `hit` is the ray's
        occlusion bit.  An interval that does not satisfy 0 <= tmin <= tmax is a miss."""
        d, e = C.c_float(), C.c_int32()
        o3, d3 = abi.Float3(*[float(x) for x in origin]), abi.Float3(*[float(x) for x in direction])
        check(load().rtowProbeNearestHitInterval(self.handle, C.byref(o3), C.byref(d3), float(time), float(tmin), float(tmax), C.byref(d), C.byref(e)),
              "rtowProbeNearestHitInterval")
        return e.value >= 0, d.value, e.value

    def _upload_rays_intervals(self, rays, intervals):
        """Device copies of `rays` (as for trace_rays) and of `intervals` (abi.RAY_INTERVAL_DTYPE or (n, 2) float32; None: no buffer): (count, rays, intervals or None)"""
        a, count = _ray_array(rays)
        iv = None
        if intervals is not None:
            iv = np.ascontiguousarray(intervals)
            if iv.dtype != np.dtype(abi.RAY_INTERVAL_DTYPE):
                iv = np.ascontiguousarray(iv, dtype=np.float32).reshape(-1, 2)
            if int(iv.shape[0]) != count:
                raise ValueError("intervals must hold one (tMin, tMax) pair per ray")
        dev = DeviceBuffer(self, max(1, count) * C.sizeof(abi.Ray))
        dev_iv = DeviceBuffer(self, max(1, count) * C.sizeof(abi.RayInterval)) if iv is not None else None
        if count:
            dev.upload(a)
            if dev_iv:
                dev_iv.upload(iv)
        return count, dev, dev_iv

    def trace_rays_interval(self, rays, intervals=None, want=("distance", "entityIndex", "normal"), stream=None):
        """rtowTraceRaysIntervalDevice on host data: the nearest Entity.Hit(r, tMin, tMax) per ray.  `rays` as for trace_rays; `intervals` an array of
        abi.RAY_INTERVAL_DTYPE (or (n, 2) float32), None = (0, +inf) for every ray (then trace_rays' result).  Returns the arrays of trace_rays."""
        count, dev, dev_iv = self._upload_rays_intervals(rays, intervals)
        try:
            return self._trace(count, lambda hits, _: check(load().rtowTraceRaysIntervalDevice(self.handle, count, dev.handle, dev_iv.handle if dev_iv else None, C.byref(hits),
                                                                                                stream), "rtowTraceRaysIntervalDevice"), want)
        finally:
            for b in (dev, dev_iv):
                if b:
                    b.free()

    def trace_occlusion(self, rays, intervals=None, stream=None):
        """rtowTraceOcclusionDevice on host data: (n,) uint8, 1 where any entity has Entity.Hit(r, tMin, tMax).  Arguments as for trace_rays_interval."""
        count, dev, dev_iv = self._upload_rays_intervals(rays, intervals)
        out = DeviceBuffer(self, max(1, count))
        try:
            check(load().rtowTraceOcclusionDevice(self.handle, count, dev.handle, dev_iv.handle if dev_iv else None, out.handle, stream), "rtowTraceOcclusionDevice")
            self.synchronize()
            return out.download(np.uint8, (count,))
        finally:
            for b in (dev, dev_iv, out):
                if b:
                    b.free()

    def shade_hits(self, rays, entity_index, environment=None, outputs=tuple(abi.SURFACE_OUTPUTS)):
        """rtowShadeHitsDevice on host data: `rays` as for trace_rays, `entity_index` the (n,) int32 "entityIndex" a trace call returned for them; `environment` an
        abi.Environment (None: RTOW_SKY_NONE, a miss's albedo is black).  Returns {"albedo": (n, 3) float32, "emission": (n, 3), "texCoord": (n, 2),
        "metallicGlossiness": (n, 2), "materialIndex": (n,) int32, "materialInfo": (n,) uint32} for the names in `outputs`.  Runs on the context's own stream and waits for it
        (ShadeHitsJob is the form for device buffers on a caller's stream)."""
        a, count = _ray_array(rays)
        ent = np.ascontiguousarray(entity_index, dtype=np.int32).reshape(-1)
        if ent.shape[0] != count:
            raise ValueError("entity_index must hold one int32 per ray")
        unknown = [k for k in outputs if k not in abi.SURFACE_OUTPUTS]
        if unknown:
            raise ValueError("unknown surface outputs: %s" % unknown)
        p = abi.ShadeHitsParams(environment if environment is not None else abi.Environment(abi.SKY_NONE), 0, 0)
        dev_rays = DeviceBuffer(self, max(1, count) * C.sizeof(abi.Ray))
        dev_ent = DeviceBuffer(self, max(1, count) * 4)
        bufs = {k: DeviceBuffer(self, max(1, count) * 4 * abi.SURFACE_OUTPUTS[k][1]) for k in abi.SURFACE_OUTPUTS if k in outputs}
        try:
            if count:
                dev_rays.upload(a)
                dev_ent.upload(ent)
            surface = abi.SurfaceBuffers(*[bufs[k].handle.value if k in bufs else None for k in abi.SURFACE_OUTPUTS])
            check(load().rtowShadeHitsDevice(self.handle, C.byref(p), count, dev_rays.handle, dev_ent.handle, C.byref(surface), None), "rtowShadeHitsDevice")
            self.synchronize()
            out = {}
            for k, b in bufs.items():
                dtype, width = abi.SURFACE_OUTPUTS[k]
                out[k] = b.download(np.dtype(dtype), (count, width) if width > 1 else (count,))
            return out
        finally:
            for b in list(bufs.values()) + [dev_rays, dev_ent]:
                b.free()

    def _trace_guide(self, count, launch, want):
        """The buffers of one guide query: allocate those named in `want` (abi.GUIDE_OUTPUTS), run `launch(out)`, wait, download."""
        unknown = [k for k in want if k not in abi.GUIDE_OUTPUTS]
        if unknown:
            raise ValueError("unknown guide outputs: %s" % unknown)
        shape = {k: (np.dtype(d), (count, w) if w > 1 else (count,)) for k, (d, w) in abi.GUIDE_OUTPUTS.items()}
        bufs = {k: DeviceBuffer(self, max(1, count) * shape[k][0].itemsize * abi.GUIDE_OUTPUTS[k][1]) for k in abi.GUIDE_OUTPUTS if k in want}
        try:
            launch(abi.guide_buffers({k: b.handle.value for k, b in bufs.items()}))
            self.synchronize()
            return {k: b.download(*shape[k]) for k, b in bufs.items()}
        finally:
            for b in bufs.values():
                b.free()

    def trace_guide_rays(self, rays, max_bounces=abi.GUIDE_DEFAULT_MAX_BOUNCES, want=tuple(abi.GUIDE_OUTPUTS), stream=None):
        """rtowTraceGuideRaysDevice on host data: every ray followed through mirrors and glass to the first surface that is not perfectly specular (or the sky, or
        `max_bounces` surfaces).  `rays` as for trace_rays.  Returns, for the names in `want`, trace_rays' arrays for the LAST segment plus "rays" (that segment's rays,
        abi.RAY_DTYPE: with "entityIndex" the input of shade_hits), "throughput" (n, 3), "pathDistance" (n,), "bounces" (n,) int32 and "end" (n,) uint8 (abi.GUIDE_END_*)."""
        a, count = _ray_array(rays)
        p = abi.GuideParams(int(max_bounces), 0, 0)
        dev = DeviceBuffer(self, max(1, count) * C.sizeof(abi.Ray))
        try:
            if count:
                dev.upload(a)
            return self._trace_guide(count, lambda out: check(load().rtowTraceGuideRaysDevice(self.handle, C.byref(p), count, dev.handle, C.byref(out), stream),
                                                              "rtowTraceGuideRaysDevice"), want)
        finally:
            dev.free()

    def trace_guide_view(self, view, width, height, max_bounces=abi.GUIDE_DEFAULT_MAX_BOUNCES, time=0.0, want=tuple(abi.GUIDE_OUTPUTS), stream=None):
        """rtowTraceGuideViewDevice: trace_guide_rays on trace_view's rays (pixel = row * width + col, row 0 at the bottom)."""
        p = abi.GuideParams(int(max_bounces), 0, 0)
        v = abi.TraceViewParams(int(width), int(height), view, float(time), 0)
        return self._trace_guide(int(width) * int(height),
                                 lambda out: check(load().rtowTraceGuideViewDevice(self.handle, C.byref(p), C.byref(v), C.byref(out), stream), "rtowTraceGuideViewDevice"), want)

    def record_paths(self, params, pixels_or_list, in_color=None, in_scw=None, select=abi.PATH_SELECT_INDEX, sample_index=0, want_segments=True, stream=None):
        """rtowRecordPathsDevice: one sample of every listed pixel, replayed as rtowSampleBatchDevice(params, ...) runs it there, with its segments.
        pixels_or_list: frame pixel indices (row * W + col), or (pixel_list, capacity) with a DeviceBuffer / device address of 4 + capacity uint32 words.
        in_color (W*H, 4) / in_scw (W*H,): the accumulators the batch reads - float32 arrays or DeviceBuffers; None: zeros.
        select: abi.PATH_SELECT_INDEX (sample `sample_index`) or abi.PATH_SELECT_BRIGHTEST.
        Returns (summaries, segments): numpy arrays of abi.PATH_SUMMARY_DTYPE, shape (n,), and of abi.PATH_SEGMENT_DTYPE, shape (n, traceDepth) - None without
        want_segments - for the n = min(words[0], capacity) entries of the list."""
        n_pixels = int(params.size.x) * int(params.size.y)
        depth = int(params.traceDepth)
        own = []
        try:
            if isinstance(pixels_or_list, tuple):
                words, capacity = pixels_or_list
                words = words.ptr if isinstance(words, DeviceBuffer) else words
                capacity = int(capacity)
                head = np.empty(1, np.uint32)
                check(load().rtowDeviceCopy(self.handle, words, head.ctypes.data, 4, abi.MEMCPY_DEVICE_TO_HOST), "rtowDeviceCopy")
                count = min(int(head[0]), capacity)
            else:
                pixels = np.ascontiguousarray(pixels_or_list, dtype=np.uint32).reshape(-1)
                count = capacity = int(pixels.size)
                own.append(DeviceBuffer(self, abi.pixel_list_bytes(capacity)).upload(np.concatenate([np.array([count, 0, 0, 0], np.uint32), pixels])))
                words = own[-1].ptr

            def device(a, width):
                if isinstance(a, DeviceBuffer):
                    return a.ptr
                own.append(DeviceBuffer(self, n_pixels * width * 4))
                if a is None:
                    own[-1].zero()
                else:
                    own[-1].upload(np.ascontiguousarray(a, dtype=np.float32).reshape(n_pixels, width))
                return own[-1].ptr

            color, scw = device(in_color, 4), device(in_scw, 1)
            s_type, g_type = np.dtype(abi.PATH_SUMMARY_DTYPE), np.dtype(abi.PATH_SEGMENT_DTYPE)
            summaries = DeviceBuffer(self, max(1, capacity) * s_type.itemsize).zero()
            own.append(summaries)
            segments = None
            if want_segments:
                segments = DeviceBuffer(self, max(1, capacity * depth) * g_type.itemsize).zero()
                own.append(segments)
            p = abi.RecordPathsParams(int(select), int(sample_index), 0, 0)
            lst = abi.PixelList(words, capacity)
            check(load().rtowRecordPathsDevice(self.handle, C.byref(params), C.byref(p), C.byref(lst), color, scw, summaries.handle,
                                               segments.handle if segments else None, stream), "rtowRecordPathsDevice")
            self.synchronize()
            out_s = summaries.download(s_type, (capacity,))[:count] if capacity else np.zeros(0, s_type)
            out_g = None
            if want_segments:
                out_g = segments.download(g_type, (capacity, depth))[:count] if capacity else np.zeros((0, depth), g_type)
            return out_s, out_g
        finally:
            for b in own:
                b.free()

    def synchronize(self):
        check(load().rtowSynchronize(self.handle), "rtowSynchronize")

    def last_sample_kernel_ms(self):
        ms = C.c_float()
        check(load().rtowGetLastSampleKernelMs(self.handle, C.byref(ms)), "rtowGetLastSampleKernelMs")
        return ms.value


def _buffers(color, normal, albedo, scw):
    return abi.AccumBuffers(color, normal, albedo, scw)


class JobHandle:
    def __init__(self, result):
        self.result = result

    def Complete(self):
        return self.result


class SampleBatchJob:
    """Mirror of `struct SampleBatchJob : IJobParallelFor` (JOBS/SampleBatchJob.cs:17-51): same field names.

    Input*/Output* are numpy float32 arrays (host form -> rtowSampleBatch) or DeviceBuffer objects
    (device-resident form -> rtowSampleBatchDevice).  OutputDiagnostics likewise.  CancellationToken is a
    ctypes c_uint8 (NativeReference<bool>) or None.
    """

    def __init__(self, context, params=None, **fields):
        self.context = context
        self.params = params if params is not None else abi.SampleParams()
        self.CancellationToken = None
        self.InputColor = self.InputNormal = self.InputAlbedo = self.InputSampleCountWeight = None
        self.OutputColor = self.OutputNormal = self.OutputAlbedo = self.OutputSampleCountWeight = None
        self.OutputDiagnostics = None
        for k, v in fields.items():
            setattr(self, k, v)

    # reference field names -> RtowSampleParams
    Size = property(lambda s: (s.params.size.x, s.params.size.y), lambda s, v: setattr(s.params, "size", abi.Float2(float(v[0]), float(v[1]))))
    SliceOffset = property(lambda s: s.params.sliceOffset, lambda s, v: setattr(s.params, "sliceOffset", int(v)))
    SliceDivider = property(lambda s: s.params.sliceDivider, lambda s, v: setattr(s.params, "sliceDivider", int(v)))
    Seed = property(lambda s: s.params.seed, lambda s, v: setattr(s.params, "seed", int(v)))
    View = property(lambda s: s.params.view, lambda s, v: setattr(s.params, "view", v))
    Environment = property(lambda s: s.params.environment, lambda s, v: setattr(s.params, "environment", v))
    TraceDepth = property(lambda s: s.params.traceDepth, lambda s, v: setattr(s.params, "traceDepth", int(v)))
    SubPixelJitter = property(lambda s: bool(s.params.subPixelJitter), lambda s, v: setattr(s.params, "subPixelJitter", int(bool(v))))
    NoiseColor = property(lambda s: s.params.noiseColor, lambda s, v: setattr(s.params, "noiseColor", int(v)))

    @property
    def SampleCountRange(self):
        return (self.params.sampleCountRange[0], self.params.sampleCountRange[1])

    @SampleCountRange.setter
    def SampleCountRange(self, v):
        self.params.sampleCountRange[0], self.params.sampleCountRange[1] = int(v[0]), int(v[1])

    @property
    def SampleCountWeightExtrema(self):
        return (self.params.sampleCountWeightExtrema.x, self.params.sampleCountWeightExtrema.y)

    @SampleCountWeightExtrema.setter
    def SampleCountWeightExtrema(self, v):
        self.params.sampleCountWeightExtrema = abi.Float2(float(v[0]), float(v[1]))

    def Schedule(self, arrayLength=None, innerloopBatchCount=1, dependsOn=None, stream=None):
        """`sampleBatchJob.Schedule(totalBufferSize, 1, dep)` (UNITY/Raytracer.cs:730).  Runs synchronously for host
        buffers (like IJob.Execute on a worker thread); enqueues on `stream` for device buffers."""
        lib = load()
        n = int(self.params.size.x) * int(self.params.size.y)
        if arrayLength is not None and arrayLength != n:
            raise ValueError("arrayLength must equal Size.x * Size.y")
        cancel = C.addressof(self.CancellationToken) if self.CancellationToken is not None else None
        ins = (self.InputColor, self.InputNormal, self.InputAlbedo, self.InputSampleCountWeight)
        outs = (self.OutputColor, self.OutputNormal, self.OutputAlbedo, self.OutputSampleCountWeight)
        if all(isinstance(b, DeviceBuffer) for b in ins + outs):
            bi = _buffers(*[b.ptr for b in ins])
            bo = _buffers(*[b.ptr for b in outs])
            diag = self.OutputDiagnostics.ptr if self.OutputDiagnostics is not None else None
            rc = lib.rtowSampleBatchDevice(self.context.handle, C.byref(self.params), C.byref(bi), C.byref(bo), diag, stream, cancel)
        else:
            for a, width in zip(ins + outs, (4, 3, 3, 1) * 2):
                if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.size == n * width):
                    raise ValueError("host buffers must be C-contiguous float32 arrays of W*H elements")
            bi = _buffers(*[a.ctypes.data for a in ins])
            bo = _buffers(*[a.ctypes.data for a in outs])
            diag = self.OutputDiagnostics.ctypes.data if self.OutputDiagnostics is not None else None
            rc = lib.rtowSampleBatch(self.context.handle, C.byref(self.params), C.byref(bi), C.byref(bo), diag, cancel)
        return JobHandle(rc)


def sample_batch_chain_device(context, params_list, ins, outs, diags=None, stream=None, cancel=None):
    """rtowSampleBatchChainDevice: `len(params_list)` successive batches of one frame enqueued together (the reference keeps two in flight,
    UNITY/Raytracer.cs:586-593); batch 0 reads `ins`, every later batch reads what its predecessor wrote to `outs`.
    ins / outs: four DeviceBuffers each; diags: one DeviceBuffer (or None) per batch."""
    count = len(params_list)
    arr = (abi.SampleParams * count)(*params_list)
    bi = _buffers(*[b.ptr for b in ins])
    bo = _buffers(*[b.ptr for b in outs])
    dptr = None
    if diags is not None:
        dptr = (C.c_void_p * count)(*[d.ptr if d is not None else None for d in diags])
    return load().rtowSampleBatchChainDevice(context.handle, count, arr, C.byref(bi), C.byref(bo), dptr, stream, cancel)


def sample_pixels_device(context, params_list, pixel_list, capacity, ins, outs, diags=None, stream=None, cancel=None):
    """rtowSamplePixelsDevice: the chain above for the pixels of a device list only (pixel_list: a DeviceBuffer or device address of 4 + capacity uint32 words,
    as build_pixel_list leaves it or as the host filled it); no other element of `outs` or `diags` is written.  params_list: 1 .. 16 batches, slice 0 / 1."""
    count = len(params_list)
    arr = (abi.SampleParams * count)(*params_list)
    bi = _buffers(*[b.ptr for b in ins])
    bo = _buffers(*[b.ptr for b in outs])
    dptr = None
    if diags is not None:
        dptr = (C.c_void_p * count)(*[d.ptr if d is not None else None for d in diags])
    words = pixel_list.ptr if isinstance(pixel_list, DeviceBuffer) else pixel_list
    lst = abi.PixelList(words, int(capacity))
    return load().rtowSamplePixelsDevice(context.handle, count, arr, C.byref(lst), C.byref(bi), C.byref(bo), dptr, stream, cancel)


def sample_batch_chain_adaptive_device(context, params_list, ins, outs, extrema_out, lag=2, extrema_in=None, diags=None, stream=None, cancel=None):
    """rtowSampleBatchChainAdaptiveDevice: the chain above, batch k >= lag deciding its sample counts from the SampleCountWeightExtrema the device reduced
    after batch k - lag (extrema_out: a DeviceBuffer of len(params_list) float2, or a device address); batches k < lag from extrema_in (a DeviceBuffer or device
    address of `lag` float2) or, if None, from their own params.  Continue a schedule with extrema_in = previous extrema_out address + 8 * (previous count - lag)."""
    count = len(params_list)
    arr = (abi.SampleParams * count)(*params_list)
    bi = _buffers(*[b.ptr for b in ins])
    bo = _buffers(*[b.ptr for b in outs])
    dptr = None
    if diags is not None:
        dptr = (C.c_void_p * count)(*[d.ptr if d is not None else None for d in diags])
    addr = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
    feed = abi.AdaptiveFeed(addr(extrema_in), addr(extrema_out), int(lag), 0)
    return load().rtowSampleBatchChainAdaptiveDevice(context.handle, count, arr, C.byref(bi), C.byref(bo), dptr, C.byref(feed), stream, cancel)


def sample_batch_group_device(context, params_list, ins, outs_list, diags=None, stream=None, cancel=None):
    """rtowSampleBatchGroupDevice: `len(params_list)` INDEPENDENT batches of one frame in one launch; every batch reads `ins` (four DeviceBuffers) and stores
    to its own four DeviceBuffers outs_list[k]; diags: one DeviceBuffer (or None) per batch."""
    count = len(params_list)
    arr = (abi.SampleParams * count)(*params_list)
    bi = _buffers(*[b.ptr for b in ins])
    bo = (abi.AccumBuffers * count)(*[_buffers(*[b.ptr for b in o]) for o in outs_list])
    dptr = None
    if diags is not None:
        dptr = (C.c_void_p * count)(*[d.ptr if d is not None else None for d in diags])
    return load().rtowSampleBatchGroupDevice(context.handle, count, arr, C.byref(bi), bo, dptr, stream, cancel)


def sample_batch_chain_host(context, params_list, inputs=None, want_diag=True):
    """rtowSampleBatchChain: `len(params_list)` successive batches on HOST buffers in one blocking call; returns the final accumulators like
    sample_batch_host, with out["diag"] = one record array per batch."""
    count = len(params_list)
    w, h = int(params_list[0].size.x), int(params_list[0].size.y)
    n = w * h
    if inputs is None:
        inputs = {"color": np.zeros((n, 4), np.float32), "normal": np.zeros((n, 3), np.float32),
                  "albedo": np.zeros((n, 3), np.float32), "scw": np.zeros(n, np.float32)}
    ins = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in inputs.items()}
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in ins.items()}
    diags = [np.zeros((n, params_list[0].diagnosticsStride // 4), np.float32) for _ in range(count)] if want_diag else None
    arr = (abi.SampleParams * count)(*params_list)
    bi = _buffers(*[ins[k].ctypes.data for k in ("color", "normal", "albedo", "scw")])
    bo = _buffers(*[out[k].ctypes.data for k in ("color", "normal", "albedo", "scw")])
    dptr = (C.c_void_p * count)(*[d.ctypes.data for d in diags]) if want_diag else None
    check(load().rtowSampleBatchChain(context.handle, count, arr, C.byref(bi), C.byref(bo), dptr, None), "rtowSampleBatchChain")
    out["diag"] = diags
    return out


def sample_batch_host(context, params, inputs=None, want_diag=True):
    """Convenience used by tests/bench: run one batch with host buffers; returns dict like the oracle binding."""
    w, h = int(params.size.x), int(params.size.y)
    n = w * h
    if inputs is None:
        inputs = {"color": np.zeros((n, 4), np.float32), "normal": np.zeros((n, 3), np.float32),
                  "albedo": np.zeros((n, 3), np.float32), "scw": np.zeros(n, np.float32)}
    ins = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in inputs.items()}
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in ins.items()}
    diag = np.zeros((n, params.diagnosticsStride // 4), np.float32) if want_diag else None
    job = SampleBatchJob(context, params)
    job.InputColor, job.InputNormal, job.InputAlbedo, job.InputSampleCountWeight = ins["color"], ins["normal"], ins["albedo"], ins["scw"]
    job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = out["color"], out["normal"], out["albedo"], out["scw"]
    job.OutputDiagnostics = diag
    rc = job.Schedule(n, 1).Complete()
    check(rc, "rtowSampleBatch")
    out["diag"] = diag
    return out


class CombineJob:
    """Mirror of `struct CombineJob` (JOBS/CombineJob.cs:10-27); device buffers."""

    def __init__(self, context, Size, DebugMode=False, LdrAlbedo=False):
        self.context, self.Size, self.DebugMode, self.LdrAlbedo = context, Size, DebugMode, LdrAlbedo
        self.InputColor = self.InputNormal = self.InputAlbedo = None
        self.OutputColor = self.OutputNormal = self.OutputAlbedo = None

    def Schedule(self, stream=None):
        p = abi.CombineParams(int(self.Size[0]), int(self.Size[1]), int(self.DebugMode), int(self.LdrAlbedo))
        rc = load().rtowCombineDevice(self.context.handle, C.byref(p), self.InputColor.ptr, self.InputNormal.ptr, self.InputAlbedo.ptr,
                                      self.OutputColor.ptr, self.OutputNormal.ptr, self.OutputAlbedo.ptr, stream)
        return JobHandle(rc)


class FinalizeTexturesJob:
    """Mirror of `struct FinalizeTexturesJob` (JOBS/FinalizeTexturesJob.cs:11-21); device buffers."""

    def __init__(self, context, pixel_count):
        self.context, self.pixel_count = context, pixel_count
        self.InputColor = self.InputNormal = self.InputAlbedo = None
        self.OutputColor = self.OutputNormal = self.OutputAlbedo = None

    def Schedule(self, stream=None):
        rc = load().rtowFinalizeDevice(self.context.handle, self.pixel_count, self.InputColor.ptr, self.InputNormal.ptr, self.InputAlbedo.ptr,
                                       self.OutputColor.ptr, self.OutputNormal.ptr, self.OutputAlbedo.ptr, stream)
        return JobHandle(rc)


def _device_ptr(buf):
    """a DeviceBuffer, or a raw device address (int) such as a view into one"""
    return buf.ptr if isinstance(buf, DeviceBuffer) else buf


class DenoiseJob:
    """The reference's denoise step (OpenImageDenoiseJob / OptixDenoiseJob, JOBS/DenoiseJobs.cs:10-119) as rtowDenoiseDevice: the edge-avoiding
    a-trous filter of include/rtow.h on combine's float3 colour, normal and albedo.  Device buffers (or raw device addresses); `Scratch` holds
    abi.denoise_scratch_bytes(Width, Height) bytes and may stay None with Iterations == 1."""

    def __init__(self, context, Width, Height, Iterations=abi.DENOISE_DEFAULT_ITERATIONS, NormalSharpness=abi.DENOISE_DEFAULT_NORMAL_SHARPNESS,
                 ColorSigma=abi.DENOISE_DEFAULT_COLOR_SIGMA, AlbedoSigma=abi.DENOISE_DEFAULT_ALBEDO_SIGMA, Flags=abi.DENOISE_DEFAULT_FLAGS, Reserved=0):
        self.context, self.Width, self.Height = context, Width, Height
        self.Iterations, self.NormalSharpness, self.ColorSigma, self.AlbedoSigma, self.Flags, self.Reserved = \
            Iterations, NormalSharpness, ColorSigma, AlbedoSigma, Flags, Reserved
        self.InputColor = self.InputNormal = self.InputAlbedo = self.OutputColor = self.Scratch = None

    def params(self):
        return abi.DenoiseParams(int(self.Width), int(self.Height), int(self.Iterations), int(self.NormalSharpness), float(self.ColorSigma),
                                 float(self.AlbedoSigma), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        rc = load().rtowDenoiseDevice(self.context.handle, C.byref(p), _device_ptr(self.InputColor), _device_ptr(self.InputNormal),
                                      _device_ptr(self.InputAlbedo), _device_ptr(self.Scratch), _device_ptr(self.OutputColor), stream)
        return JobHandle(rc)


class MomentsJob:
    """rtowAccumulateMomentsDevice: per-pixel luminance moments (s1, s2, n) over the colour buffers of independent batches of one frame - the `outs[k]` colours of
    sample_batch_group_device, before they are folded.  Colors: 1 .. 16 device buffers (or raw device addresses) of float4 per pixel; InputMoments: the moments so
    far (None = zeros; may be OutputMoments itself); OutputMoments: abi.moments_bytes(PixelCount) bytes."""

    def __init__(self, context, PixelCount):
        self.context, self.PixelCount = context, PixelCount
        self.Colors = []
        self.InputMoments = self.OutputMoments = None

    def Schedule(self, stream=None):
        count = len(self.Colors)
        colors = (C.c_void_p * max(count, 1))(*[_device_ptr(c) for c in self.Colors])
        rc = load().rtowAccumulateMomentsDevice(self.context.handle, int(self.PixelCount), count, colors, _device_ptr(self.InputMoments),
                                                _device_ptr(self.OutputMoments), stream)
        return JobHandle(rc)


class DenoiseVarianceJob(DenoiseJob):
    """rtowDenoiseVarianceDevice: DenoiseJob's filter with the colour term scaled by the local variance that MomentsJob's moments give (include/rtow.h).  `Moments`:
    float3 per pixel; `Scratch`: abi.denoise_variance_scratch_bytes(Width, Height) bytes, never None; `OutputVariance` (optional): float per pixel, the filtered
    variance of the last level, abi.DENOISE_VARIANCE_UNKNOWN where a pixel has no estimate."""

    def __init__(self, context, Width, Height, Iterations=abi.DENOISE_VARIANCE_DEFAULT_ITERATIONS, NormalSharpness=abi.DENOISE_VARIANCE_DEFAULT_NORMAL_SHARPNESS,
                 ColorSigma=abi.DENOISE_VARIANCE_DEFAULT_COLOR_SIGMA, AlbedoSigma=abi.DENOISE_VARIANCE_DEFAULT_ALBEDO_SIGMA, Flags=abi.DENOISE_VARIANCE_DEFAULT_FLAGS,
                 Reserved=0):
        super().__init__(context, Width, Height, Iterations, NormalSharpness, ColorSigma, AlbedoSigma, Flags, Reserved)
        self.Moments = self.OutputVariance = None

    def Schedule(self, stream=None):
        p = self.params()
        rc = load().rtowDenoiseVarianceDevice(self.context.handle, C.byref(p), _device_ptr(self.InputColor), _device_ptr(self.InputNormal),
                                              _device_ptr(self.InputAlbedo), _device_ptr(self.Moments), _device_ptr(self.Scratch),
                                              _device_ptr(self.OutputColor), _device_ptr(self.OutputVariance), stream)
        return JobHandle(rc)


class ReprojectJob:
    """rtowReprojectAccumDevice: what replaces the ZeroMemory of ScheduleSample(firstBatch) (UNITY/Raytracer.cs:616-626) after a camera move over a static
    world - the previous view's accumulators gathered to the new view's pixels.  Device buffers (or raw device addresses): Rays / HitDistance / HitEntityIndex
    are rtowTraceViewDevice's outputs for the NEW view, PreviousHitDistance / PreviousHitEntityIndex those kept from PreviousView; the four Previous* are the
    accumulators rendered at PreviousView, the four Output* receive the carried sums; OutputSource (optional) the previous pixel each pixel carries, -1 = none."""

    def __init__(self, context, Width, Height, PreviousView, DepthTolerance=abi.REPROJECT_DEFAULT_DEPTH_TOLERANCE, MaxHistory=abi.REPROJECT_DEFAULT_MAX_HISTORY,
                 Flags=abi.REPROJECT_DEFAULT_FLAGS, Reserved=0):
        self.context, self.Width, self.Height, self.PreviousView = context, Width, Height, PreviousView
        self.DepthTolerance, self.MaxHistory, self.Flags, self.Reserved = DepthTolerance, MaxHistory, Flags, Reserved
        self.Rays = self.HitDistance = self.HitEntityIndex = self.PreviousHitDistance = self.PreviousHitEntityIndex = None
        self.PreviousColor = self.PreviousNormal = self.PreviousAlbedo = self.PreviousSampleCountWeight = None
        self.OutputColor = self.OutputNormal = self.OutputAlbedo = self.OutputSampleCountWeight = self.OutputSource = None

    def params(self):
        return abi.ReprojectParams(int(self.Width), int(self.Height), self.PreviousView, float(self.DepthTolerance), int(self.MaxHistory), int(self.Flags),
                                   int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        hits = abi.HitBuffers(_device_ptr(self.HitDistance), _device_ptr(self.HitEntityIndex), None)
        prev_hits = abi.HitBuffers(_device_ptr(self.PreviousHitDistance), _device_ptr(self.PreviousHitEntityIndex), None)
        prev = _buffers(*[_device_ptr(b) for b in (self.PreviousColor, self.PreviousNormal, self.PreviousAlbedo, self.PreviousSampleCountWeight)])
        out = _buffers(*[_device_ptr(b) for b in (self.OutputColor, self.OutputNormal, self.OutputAlbedo, self.OutputSampleCountWeight)])
        rc = load().rtowReprojectAccumDevice(self.context.handle, C.byref(p), _device_ptr(self.Rays), C.byref(hits), C.byref(prev_hits), C.byref(prev), C.byref(out),
                                             _device_ptr(self.OutputSource), stream)
        return JobHandle(rc)


class ReprojectBilinearJob(ReprojectJob):
    """rtowReprojectAccumBilinearDevice: ReprojectJob through the four previous pixels around the reprojected point, each validated on its own and the bilinear
    weights renormalised over the valid ones (SVGF's reprojection).  The fields are ReprojectJob's; with PreviousMoments and OutputMoments (both or neither,
    abi.moments_bytes(Width * Height) bytes each) the luminance moments travel in the same pass through the same taps, capped at MaxBatches, and no
    ReprojectMomentsJob is needed.  OutputSource (optional) receives the previous pixel of the heaviest valid tap, -1 = none."""

    def __init__(self, context, Width, Height, PreviousView, DepthTolerance=abi.REPROJECT_DEFAULT_DEPTH_TOLERANCE, MaxHistory=abi.REPROJECT_DEFAULT_MAX_HISTORY,
                 Flags=abi.REPROJECT_DEFAULT_FLAGS, Reserved=0, MaxBatches=abi.REPROJECT_MOMENTS_DEFAULT_MAX_BATCHES):
        super().__init__(context, Width, Height, PreviousView, DepthTolerance, MaxHistory, Flags, Reserved)
        self.MaxBatches = MaxBatches
        self.PreviousMoments = self.OutputMoments = None

    def Schedule(self, stream=None):
        p = self.params()
        hits = abi.HitBuffers(_device_ptr(self.HitDistance), _device_ptr(self.HitEntityIndex), None)
        prev_hits = abi.HitBuffers(_device_ptr(self.PreviousHitDistance), _device_ptr(self.PreviousHitEntityIndex), None)
        prev = _buffers(*[_device_ptr(b) for b in (self.PreviousColor, self.PreviousNormal, self.PreviousAlbedo, self.PreviousSampleCountWeight)])
        out = _buffers(*[_device_ptr(b) for b in (self.OutputColor, self.OutputNormal, self.OutputAlbedo, self.OutputSampleCountWeight)])
        rc = load().rtowReprojectAccumBilinearDevice(self.context.handle, C.byref(p), _device_ptr(self.Rays), C.byref(hits), C.byref(prev_hits), C.byref(prev),
                                                     C.byref(out), _device_ptr(self.PreviousMoments), int(self.MaxBatches), _device_ptr(self.OutputMoments),
                                                     _device_ptr(self.OutputSource), stream)
        return JobHandle(rc)


class ReprojectMomentsJob:
    """rtowReprojectMomentsDevice: the previous view's luminance moments (MomentsJob's) gathered to the new view's pixels through ReprojectJob's OutputSource, so that the
    variance estimate survives a camera move as the accumulators do.  Device buffers (or raw device addresses): Source int32 per pixel, PreviousMoments and
    OutputMoments abi.moments_bytes(PixelCount) bytes each (a gather: not in place).  MaxBatches caps the history a pixel carries; the mean s1 / n stays."""

    def __init__(self, context, PixelCount, MaxBatches=abi.REPROJECT_MOMENTS_DEFAULT_MAX_BATCHES):
        self.context, self.PixelCount, self.MaxBatches = context, PixelCount, MaxBatches
        self.Source = self.PreviousMoments = self.OutputMoments = None

    def Schedule(self, stream=None):
        rc = load().rtowReprojectMomentsDevice(self.context.handle, int(self.PixelCount), _device_ptr(self.Source), _device_ptr(self.PreviousMoments),
                                               int(self.MaxBatches), _device_ptr(self.OutputMoments), stream)
        return JobHandle(rc)


class EstimateMomentsJob:
    """rtowEstimateMomentsDevice: moments for the pixels whose history is shorter than MinBatches batches - reprojection holes, or with InputMoments None every pixel of
    a frame rendered as one batch or as a chain - estimated from the 7 x 7 neighbourhood of the accumulated Color (float4, .w = samples), weighted by the first-hit
    guides HitDistance / HitEntityIndex / HitNormal of rtowTraceViewDevice for this view.  InputMoments: None = zeros, or OutputMoments itself (in place);
    OutputMoments: abi.moments_bytes(Width * Height) bytes, what DenoiseVarianceJob takes as Moments; OutputFilled (optional): one byte per pixel, 1 where estimated."""

    def __init__(self, context, Width, Height, MinBatches=abi.ESTIMATE_MOMENTS_DEFAULT_MIN_BATCHES, MinTaps=abi.ESTIMATE_MOMENTS_DEFAULT_MIN_TAPS,
                 NormalSharpness=abi.ESTIMATE_MOMENTS_DEFAULT_NORMAL_SHARPNESS, DepthTolerance=abi.ESTIMATE_MOMENTS_DEFAULT_DEPTH_TOLERANCE,
                 Flags=abi.ESTIMATE_MOMENTS_DEFAULT_FLAGS, Reserved=0):
        self.context, self.Width, self.Height = context, Width, Height
        self.MinBatches, self.MinTaps, self.NormalSharpness, self.DepthTolerance, self.Flags, self.Reserved = MinBatches, MinTaps, NormalSharpness, DepthTolerance, Flags, Reserved
        self.Color = self.HitDistance = self.HitEntityIndex = self.HitNormal = None
        self.InputMoments = self.OutputMoments = self.OutputFilled = None

    def params(self):
        return abi.EstimateMomentsParams(int(self.Width), int(self.Height), int(self.MinBatches), int(self.MinTaps), int(self.NormalSharpness),
                                         float(self.DepthTolerance), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        hits = abi.HitBuffers(_device_ptr(self.HitDistance), _device_ptr(self.HitEntityIndex), _device_ptr(self.HitNormal))
        rc = load().rtowEstimateMomentsDevice(self.context.handle, C.byref(p), _device_ptr(self.Color), C.byref(hits), _device_ptr(self.InputMoments),
                                              _device_ptr(self.OutputMoments), _device_ptr(self.OutputFilled), stream)
        return JobHandle(rc)


class NoiseMaskJob:
    """rtowNoiseMaskDevice: from the luminance moments (MomentsJob's, carried by ReprojectMomentsJob, filled by EstimateMomentsJob) to the byte mask PixelListJob takes as
    Mask - 1 where the filtered squared error of the pixel's mean (relative to mean^2 + LuminanceFloor^2 unless abi.NOISE_MASK_ABSOLUTE) is at or above ErrorThreshold,
    or within Dilate pixels of such a pixel.  MaxQualifying > 0 raises the threshold to the histogram bin edge that keeps the qualifying pixels within that budget.
    Device buffers (or raw device addresses): Moments abi.moments_bytes(Width * Height) bytes, OutputMask one byte per pixel, OutputError (optional) one float per
    pixel (abi.NOISE_MASK_UNKNOWN where there is no estimate), OutputStats (optional) one abi.NoiseStats in DEVICE memory, Scratch abi.noise_mask_scratch_bytes()."""

    def __init__(self, context, Width, Height, ErrorThreshold=abi.NOISE_MASK_DEFAULT_ERROR_THRESHOLD, LuminanceFloor=abi.NOISE_MASK_DEFAULT_LUMINANCE_FLOOR,
                 Dilate=abi.NOISE_MASK_DEFAULT_DILATE, MaxQualifying=None, Flags=abi.NOISE_MASK_DEFAULT_FLAGS, Reserved=0):
        self.context, self.Width, self.Height = context, Width, Height
        if MaxQualifying is None:
            MaxQualifying = int(Width) * int(Height) // abi.NOISE_MASK_DEFAULT_BUDGET_DIVISOR
        self.ErrorThreshold, self.LuminanceFloor, self.Dilate, self.MaxQualifying, self.Flags, self.Reserved = \
            ErrorThreshold, LuminanceFloor, Dilate, MaxQualifying, Flags, Reserved
        self.Moments = self.OutputMask = self.OutputError = self.OutputStats = self.Scratch = None

    def params(self):
        return abi.NoiseMaskParams(int(self.Width), int(self.Height), float(self.ErrorThreshold), float(self.LuminanceFloor), int(self.Dilate),
                                   int(self.MaxQualifying), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        rc = load().rtowNoiseMaskDevice(self.context.handle, C.byref(p), _device_ptr(self.Moments), _device_ptr(self.OutputMask), _device_ptr(self.OutputError),
                                        _device_ptr(self.OutputStats), _device_ptr(self.Scratch), stream)
        return JobHandle(rc)


class RectifyHistoryJob:
    """rtowRectifyHistoryDevice: carried history (ReprojectJob's four outputs, ReprojectMomentsJob's moments) that the first batches of the new view refute is scaled
    down or dropped - a pixel whose carried mean luminance lies outside SigmaScale standard deviations plus RelativeTolerance means of the Fresh samples in its
    (2 Radius + 1)^2 guide-weighted neighbourhood.  Device buffers (or raw device addresses): the four History* accumulators; Fresh the float4 colour sums of the new
    view's batches rendered from zero; HitDistance / HitEntityIndex / HitNormal of rtowTraceViewDevice for the new view; InputMoments / OutputMoments both or neither;
    each Output* may be its input (in place).  OutputKeep (optional): one float per pixel, the factor applied; OutputStats (optional): one abi.RectifyStats in DEVICE
    memory.  Runs before MomentsJob and rtowAddAccumDevice fold the fresh batches in."""

    def __init__(self, context, Width, Height, Radius=abi.RECTIFY_DEFAULT_RADIUS, MinTaps=abi.RECTIFY_DEFAULT_MIN_TAPS,
                 NormalSharpness=abi.RECTIFY_DEFAULT_NORMAL_SHARPNESS, DepthTolerance=abi.RECTIFY_DEFAULT_DEPTH_TOLERANCE, SigmaScale=abi.RECTIFY_DEFAULT_SIGMA_SCALE,
                 RelativeTolerance=abi.RECTIFY_DEFAULT_RELATIVE_TOLERANCE, Flags=abi.RECTIFY_DEFAULT_FLAGS, Reserved=0):
        self.context, self.Width, self.Height = context, Width, Height
        self.Radius, self.MinTaps, self.NormalSharpness, self.DepthTolerance = Radius, MinTaps, NormalSharpness, DepthTolerance
        self.SigmaScale, self.RelativeTolerance, self.Flags, self.Reserved = SigmaScale, RelativeTolerance, Flags, Reserved
        self.HistoryColor = self.HistoryNormal = self.HistoryAlbedo = self.HistorySampleCountWeight = None
        self.Fresh = self.HitDistance = self.HitEntityIndex = self.HitNormal = self.InputMoments = None
        self.OutputColor = self.OutputNormal = self.OutputAlbedo = self.OutputSampleCountWeight = None
        self.OutputMoments = self.OutputKeep = self.OutputStats = None

    def params(self):
        return abi.RectifyParams(int(self.Width), int(self.Height), int(self.Radius), int(self.MinTaps), int(self.NormalSharpness), float(self.DepthTolerance),
                                 float(self.SigmaScale), float(self.RelativeTolerance), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        hits = abi.HitBuffers(_device_ptr(self.HitDistance), _device_ptr(self.HitEntityIndex), _device_ptr(self.HitNormal))
        history = _buffers(*[_device_ptr(b) for b in (self.HistoryColor, self.HistoryNormal, self.HistoryAlbedo, self.HistorySampleCountWeight)])
        out = _buffers(*[_device_ptr(b) for b in (self.OutputColor, self.OutputNormal, self.OutputAlbedo, self.OutputSampleCountWeight)])
        rc = load().rtowRectifyHistoryDevice(self.context.handle, C.byref(p), C.byref(history), _device_ptr(self.Fresh), C.byref(hits), _device_ptr(self.InputMoments),
                                             C.byref(out), _device_ptr(self.OutputMoments), _device_ptr(self.OutputKeep), _device_ptr(self.OutputStats), stream)
        return JobHandle(rc)


class ExposureJob:
    """rtowMeterExposureDevice: the exposure a frame asks for, measured on the device - a 256-bin histogram of log-luminance over InputColor (the float3 colour finalize
    would take), the mean of the bins between the LowPermille and HighPermille ranks of the metered pixels mapped to 2^Compensation, limited to MinStops .. MaxStops and
    approached by Rate per call.  Device buffers (or raw device addresses): InputColor; Scratch of abi.exposure_scratch_bytes() bytes; State, one abi.ExposureState in
    DEVICE memory that lives across frames (zero-filled = no history) and is what ToneMapJob reads - the host never has to."""

    def __init__(self, context, Width, Height, LowPermille=abi.EXPOSURE_DEFAULT_LOW_PERMILLE, HighPermille=abi.EXPOSURE_DEFAULT_HIGH_PERMILLE,
                 Compensation=abi.EXPOSURE_DEFAULT_COMPENSATION, MinStops=abi.EXPOSURE_DEFAULT_MIN_STOPS, MaxStops=abi.EXPOSURE_DEFAULT_MAX_STOPS,
                 Rate=abi.EXPOSURE_DEFAULT_RATE, Flags=0, Reserved=0):
        self.context, self.Width, self.Height = context, Width, Height
        self.LowPermille, self.HighPermille, self.Compensation, self.MinStops, self.MaxStops = LowPermille, HighPermille, Compensation, MinStops, MaxStops
        self.Rate, self.Flags, self.Reserved = Rate, Flags, Reserved
        self.InputColor = self.Scratch = self.State = None

    def params(self):
        return abi.ExposureParams(int(self.Width), int(self.Height), int(self.LowPermille), int(self.HighPermille), float(self.Compensation), float(self.MinStops),
                                  float(self.MaxStops), float(self.Rate), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        rc = load().rtowMeterExposureDevice(self.context.handle, C.byref(p), _device_ptr(self.InputColor), _device_ptr(self.Scratch), _device_ptr(self.State), stream)
        return JobHandle(rc)


class ToneMapJob:
    """rtowFinalizeToneMappedDevice: FinalizeTexturesJob with an exposure and a tone curve (abi.TONE_CLAMP / TONE_ACES_FITTED / TONE_ACES_FILM) in front of the colour's
    byte conversion - the line the reference left commented out (JOBS/FinalizeTexturesJob.cs:28).  Device buffers (or raw device addresses).  State (optional): the
    abi.ExposureState ExposureJob keeps in device memory, whose exposure multiplies Exposure when the kernel runs; InputNormal / OutputNormal and InputAlbedo /
    OutputAlbedo may each stay None as a pair.  TONE_CLAMP with Exposure 1 and no State gives FinalizeTexturesJob's bytes."""

    def __init__(self, context, PixelCount, Curve=abi.TONE_DEFAULT_CURVE, Exposure=abi.TONE_DEFAULT_EXPOSURE, Flags=0):
        self.context, self.PixelCount, self.Curve, self.Exposure, self.Flags = context, PixelCount, Curve, Exposure, Flags
        self.State = self.InputColor = self.InputNormal = self.InputAlbedo = None
        self.OutputColor = self.OutputNormal = self.OutputAlbedo = None

    def params(self):
        return abi.ToneMapParams(int(self.PixelCount), int(self.Curve), float(self.Exposure), int(self.Flags), (C.c_int32 * 2)(0, 0))

    def Schedule(self, stream=None):
        p = self.params()
        rc = load().rtowFinalizeToneMappedDevice(self.context.handle, C.byref(p), _device_ptr(self.State), _device_ptr(self.InputColor), _device_ptr(self.InputNormal),
                                                 _device_ptr(self.InputAlbedo), _device_ptr(self.OutputColor), _device_ptr(self.OutputNormal),
                                                 _device_ptr(self.OutputAlbedo), stream)
        return JobHandle(rc)


class BloomJob:
    """rtowBloomDevice: HDR bloom on the float3 colour between the upsample and the meter - a bright pass at Threshold (in exposed units, faded in over Knee), a
    pyramid of Levels mips whose first downsample is luminance weighted with abi.BLOOM_KARIS_AVERAGE (fireflies), the pyramid summed upwards with Scatter, and
    Intensity times the sum added to the frame.  Device buffers (or raw device addresses): InputColor; Scratch of abi.bloom_scratch_bytes(Width, Height) bytes;
    OutputColor, which may be InputColor itself; State (optional), the abi.ExposureState ExposureJob keeps in device memory - bloom runs in front of the meter, so it
    sees the previous frame's exposure."""

    def __init__(self, context, Width, Height, Levels=abi.BLOOM_DEFAULT_LEVELS, Threshold=abi.BLOOM_DEFAULT_THRESHOLD, Knee=abi.BLOOM_DEFAULT_KNEE,
                 Scatter=abi.BLOOM_DEFAULT_SCATTER, Intensity=abi.BLOOM_DEFAULT_INTENSITY, Exposure=abi.BLOOM_DEFAULT_EXPOSURE, Flags=abi.BLOOM_DEFAULT_FLAGS, Reserved=0):
        self.context, self.Width, self.Height, self.Levels = context, Width, Height, Levels
        self.Threshold, self.Knee, self.Scatter, self.Intensity, self.Exposure, self.Flags, self.Reserved = Threshold, Knee, Scatter, Intensity, Exposure, Flags, Reserved
        self.State = self.InputColor = self.Scratch = self.OutputColor = None

    def params(self):
        return abi.BloomParams(int(self.Width), int(self.Height), int(self.Levels), float(self.Threshold), float(self.Knee), float(self.Scatter), float(self.Intensity),
                               float(self.Exposure), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        rc = load().rtowBloomDevice(self.context.handle, C.byref(p), _device_ptr(self.State), _device_ptr(self.InputColor), _device_ptr(self.Scratch),
                                    _device_ptr(self.OutputColor), stream)
        return JobHandle(rc)


class PixelListJob:
    """rtowBuildPixelListDevice: the pixels of a Width x Height frame that lie in the rectangle [X0, X1) x [Y0, Y1) and in the row slice, whose Mask byte (optional) is
    not 0 and whose accumulated sample count Color[4 p + 3] (optional) is not >= MinSampleCount, as a device list in 8 x 8 tile order for rtowSamplePixelsDevice.
    Device buffers (or raw device addresses): List holds abi.pixel_list_bytes(Capacity) bytes, Scratch abi.pixel_list_scratch_bytes(Width, Height).  The rectangle
    defaults to the frame, the slice to every row."""

    def __init__(self, context, Width, Height, Capacity, X0=0, Y0=0, X1=None, Y1=None, SliceOffset=0, SliceDivider=1, MinSampleCount=0.0, Flags=0, Reserved=0):
        self.context, self.Width, self.Height, self.Capacity = context, Width, Height, Capacity
        self.X0, self.Y0, self.X1, self.Y1 = X0, Y0, Width if X1 is None else X1, Height if Y1 is None else Y1
        self.SliceOffset, self.SliceDivider, self.MinSampleCount, self.Flags, self.Reserved = SliceOffset, SliceDivider, MinSampleCount, Flags, Reserved
        self.Color = self.Mask = self.Scratch = self.List = None

    def params(self):
        return abi.PixelListParams(int(self.Width), int(self.Height), int(self.X0), int(self.Y0), int(self.X1), int(self.Y1), int(self.SliceOffset),
                                   int(self.SliceDivider), float(self.MinSampleCount), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        lst = abi.PixelList(_device_ptr(self.List), int(self.Capacity))
        rc = load().rtowBuildPixelListDevice(self.context.handle, C.byref(p), _device_ptr(self.Color), _device_ptr(self.Mask), _device_ptr(self.Scratch), C.byref(lst), stream)
        return JobHandle(rc)


def build_pixel_list(context, width, height, capacity, color=None, mask=None, min_sample_count=0.0, rect=None, slice_offset=0, slice_divider=1, stream=None):
    """One PixelListJob with buffers of its own: returns (list DeviceBuffer of 4 + capacity uint32 words, the scratch DeviceBuffer - keep it alive until the stream has
    run the call).  rect: (x0, y0, x1, y1), default the frame; color / mask: DeviceBuffers or device addresses, or None."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, width, height)
    job = PixelListJob(context, width, height, capacity, x0, y0, x1, y1, slice_offset, slice_divider, min_sample_count)
    job.Color, job.Mask = color, mask
    job.List = DeviceBuffer(context, abi.pixel_list_bytes(capacity))
    job.Scratch = DeviceBuffer(context, max(4, abi.pixel_list_scratch_bytes(width, height)))
    check(job.Schedule(stream).Complete(), "rtowBuildPixelListDevice")
    return job.List, job.Scratch


def refine_noisy_pixels(context, width, height, params_list, moments, accum, capacity=None, **mask_settings):
    """One round of variance-driven adaptive sampling on the context's own stream, over the existing calls: NoiseMaskJob on `moments` -> build_pixel_list(mask=...) ->
    per batch of params_list: sample_pixels_device from zeroed accumulators, rtowAccumulateMomentsDevice into `moments` in place (a pixel that is not listed has
    color.w == 0 and is skipped by the moments rule), rtowAddAccumDevice onto `accum`.  moments: DeviceBuffer of abi.moments_bytes(width * height); accum: the frame's
    four accumulator DeviceBuffers (color, normal, albedo, sampleCountWeight); params_list: one abi.SampleParams per batch - equal sample counts, as the moments expect,
    and seeds the frame has not used; capacity: of the pixel list (default: every pixel); mask_settings: NoiseMaskJob's keyword arguments.
    Returns (abi.NoiseStats as the device left it, listed: words[0] of the list - above `capacity` the list overflowed and its first `capacity` pixels were sampled)."""
    n = int(width) * int(height)
    capacity = n if capacity is None else int(capacity)
    lib = load()
    job = NoiseMaskJob(context, width, height, **mask_settings)
    own = [DeviceBuffer(context, n), DeviceBuffer(context, C.sizeof(abi.NoiseStats)), DeviceBuffer(context, abi.noise_mask_scratch_bytes())]
    own += [DeviceBuffer(context, n * k * 4) for k in (4, 3, 3, 1)]
    try:
        job.Moments, job.OutputMask, job.OutputStats, job.Scratch = moments, own[0], own[1], own[2]
        check(job.Schedule().Complete(), "rtowNoiseMaskDevice")
        plist, scratch = build_pixel_list(context, width, height, capacity, mask=own[0])
        own += [plist, scratch]
        part = own[3:7]
        dst, src = _buffers(*[_device_ptr(b) for b in accum]), _buffers(*[b.ptr for b in part])
        colors = (C.c_void_p * 1)(part[0].ptr)
        for p in params_list:
            for b in part:
                b.zero()
            check(sample_pixels_device(context, [p], plist, capacity, part, part), "rtowSamplePixelsDevice")
            check(lib.rtowAccumulateMomentsDevice(context.handle, n, 1, colors, _device_ptr(moments), _device_ptr(moments), None), "rtowAccumulateMomentsDevice")
            check(lib.rtowAddAccumDevice(context.handle, n, C.byref(dst), C.byref(src), None), "rtowAddAccumDevice")
        context.synchronize()
        stats = abi.NoiseStats.from_buffer_copy(own[1].download(np.uint8, (C.sizeof(abi.NoiseStats),)).tobytes())
        listed = int(plist.download(np.uint32, (4,))[0])
        return stats, listed
    finally:
        for b in own:
            b.free()


class UpsampleJob:
    """rtowUpsampleDevice: a frame rendered at SrcWidth x SrcHeight (the host's bufferSize under resolutionScaling, UNITY/Raytracer.cs:478-480) brought to the displayed
    DstWidth x DstHeight before FinalizeTexturesJob - what replaces the Point / Bilinear raster blit of the scaled texture (:1123).  Device buffers (or raw device
    addresses): SrcColor is combine's or the denoiser's float3 colour; Src* / Dst* HitDistance, HitEntityIndex, HitNormal are rtowTraceViewDevice's outputs at the two
    sizes with the batch's view (GUIDED mode), SrcAlbedo / DstAlbedo rtowShadeHitsDevice's at the two sizes (RTOW_UPSAMPLE_DEMODULATE_ALBEDO); OutputColor receives
    float3 per dst pixel, OutputStage (optional) one byte per dst pixel: the stage that answered."""

    def __init__(self, context, SrcWidth, SrcHeight, DstWidth, DstHeight, Mode=abi.UPSAMPLE_DEFAULT_MODE, NormalSharpness=abi.UPSAMPLE_DEFAULT_NORMAL_SHARPNESS,
                 DepthTolerance=abi.UPSAMPLE_DEFAULT_DEPTH_TOLERANCE, Flags=abi.UPSAMPLE_DEFAULT_FLAGS, Reserved=0):
        self.context, self.SrcWidth, self.SrcHeight, self.DstWidth, self.DstHeight = context, SrcWidth, SrcHeight, DstWidth, DstHeight
        self.Mode, self.NormalSharpness, self.DepthTolerance, self.Flags, self.Reserved = Mode, NormalSharpness, DepthTolerance, Flags, Reserved
        self.SrcColor = self.SrcHitDistance = self.SrcHitEntityIndex = self.SrcHitNormal = self.SrcAlbedo = None
        self.DstHitDistance = self.DstHitEntityIndex = self.DstHitNormal = self.DstAlbedo = None
        self.OutputColor = self.OutputStage = None

    def params(self):
        return abi.UpsampleParams(int(self.SrcWidth), int(self.SrcHeight), int(self.DstWidth), int(self.DstHeight), int(self.Mode), int(self.NormalSharpness),
                                  float(self.DepthTolerance), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        src_hits = abi.HitBuffers(_device_ptr(self.SrcHitDistance), _device_ptr(self.SrcHitEntityIndex), _device_ptr(self.SrcHitNormal))
        dst_hits = abi.HitBuffers(_device_ptr(self.DstHitDistance), _device_ptr(self.DstHitEntityIndex), _device_ptr(self.DstHitNormal))
        rc = load().rtowUpsampleDevice(self.context.handle, C.byref(p), _device_ptr(self.SrcColor), C.byref(src_hits), _device_ptr(self.SrcAlbedo), C.byref(dst_hits),
                                       _device_ptr(self.DstAlbedo), _device_ptr(self.OutputColor), _device_ptr(self.OutputStage), stream)
        return JobHandle(rc)


class ShadeHitsJob:
    """rtowShadeHitsDevice on device buffers (or raw device addresses): Rays / EntityIndex are a trace call's rays and hit entity indices, `Count` elements; the six
    outputs (Albedo, Emission, TexCoord, MetallicGlossiness, MaterialIndex, MaterialInfo) may each stay None (not written), not all.  Environment: the sky a miss takes
    its albedo from (abi.Environment; None = RTOW_SKY_NONE)."""

    def __init__(self, context, Count, Environment=None, Flags=0, Reserved=0):
        self.context, self.Count, self.Environment, self.Flags, self.Reserved = context, Count, Environment, Flags, Reserved
        self.Rays = self.EntityIndex = None
        self.Albedo = self.Emission = self.TexCoord = self.MetallicGlossiness = self.MaterialIndex = self.MaterialInfo = None

    def params(self):
        return abi.ShadeHitsParams(self.Environment if self.Environment is not None else abi.Environment(abi.SKY_NONE), int(self.Flags), int(self.Reserved))

    def Schedule(self, stream=None):
        p = self.params()
        ptr = lambda b: _device_ptr(b) if b is not None else None
        surface = abi.SurfaceBuffers(*[ptr(b) for b in (self.Albedo, self.Emission, self.TexCoord, self.MetallicGlossiness, self.MaterialIndex, self.MaterialInfo)])
        rc = load().rtowShadeHitsDevice(self.context.handle, C.byref(p), int(self.Count), ptr(self.Rays), ptr(self.EntityIndex), C.byref(surface), stream)
        return JobHandle(rc)


class ReduceMetricsJob:
    """Mirror of `struct ReduceMetricsJob` (JOBS/ReduceMetricsJob.cs:10-20); device buffers in, scalars out."""

    def __init__(self, context, pixel_count, diagnostics_stride=4):
        self.context, self.pixel_count, self.stride = context, pixel_count, diagnostics_stride
        self.Diagnostics = self.AccumulatedColor = self.AccumulatedSampleCountWeight = None
        self.metrics = abi.Metrics()

    def Schedule(self, stream=None):
        rc = load().rtowReduceMetricsDevice(self.context.handle, self.pixel_count, self.Diagnostics.ptr, self.stride, self.AccumulatedColor.ptr,
                                            self.AccumulatedSampleCountWeight.ptr, stream, C.byref(self.metrics))
        return JobHandle(rc)

    TotalRayCount = property(lambda s: s.metrics.totalRayCount)
    TotalSamples = property(lambda s: s.metrics.totalSamples)
    SampleCountWeightExtrema = property(lambda s: (s.metrics.sampleCountWeightExtrema.x, s.metrics.sampleCountWeightExtrema.y))
    SampleCountExtrema = property(lambda s: (s.metrics.sampleCountExtrema[0], s.metrics.sampleCountExtrema[1]))
