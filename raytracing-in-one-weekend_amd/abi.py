"""ctypes mirror of include/rtow.h (the C ABI of librtow_hip.so).

Field order and types must match the header exactly; tests/test_abi.py checks sizeof() of every
struct against the values the C compiler reports (rtowGetStructSizes is not needed: the oracle
library is compiled from the same header and exposes the sizes it saw).
"""
import ctypes as C

RTOW_API_VERSION = 12

# RtowResult
RTOW_SUCCESS = 0
RTOW_ERROR_INVALID_VALUE = 1
RTOW_ERROR_MEMORY_ALLOCATION = 2
RTOW_ERROR_NO_DEVICE = 3
RTOW_ERROR_NO_SCENE = 4
RTOW_ERROR_UNSUPPORTED = 5
RTOW_ERROR_LAUNCH_FAILURE = 6
RTOW_ERROR_CANCELLED = 7
RTOW_ERROR_CAPACITY = 8
RTOW_ERROR_INTERNAL = 99

# RtowEntityType (RT/Entity.cs:13-20)
ENTITY_NONE, ENTITY_SPHERE, ENTITY_RECT, ENTITY_BOX, ENTITY_TRIANGLE = range(5)
# RtowMaterialType (RT/Material.cs:9-14)
MATERIAL_STANDARD, MATERIAL_DIELECTRIC, MATERIAL_PROBABILISTIC_VOLUME = range(3)
# RtowTextureType (RT/Texture.cs:13-21)
TEXTURE_NONE, TEXTURE_CONSTANT, TEXTURE_CHECKER_PATTERN, TEXTURE_PERLIN_NOISE, TEXTURE_IMAGE, TEXTURE_CONSTANT_SCALAR = range(6)
# RtowSkyType (RT/Environment.cs:5-10)
SKY_NONE, SKY_GRADIENT, SKY_CUBEMAP = range(3)
# RtowNoiseColor (RT/RandomSource.cs:8-13)
NOISE_WHITE, NOISE_BLUE, NOISE_SPATIOTEMPORAL_BLUE = range(3)
# RtowMemcpyKind
MEMCPY_HOST_TO_HOST, MEMCPY_HOST_TO_DEVICE, MEMCPY_DEVICE_TO_HOST, MEMCPY_DEVICE_TO_DEVICE = range(4)


class Float2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class Float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(float(x), float(y), float(z))

    def tuple(self):
        return (self.x, self.y, self.z)


class Float4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Texture(C.Structure):
    _fields_ = [("type", C.c_int32), ("mainColor", Float3), ("parameter", C.c_float),
                ("scalarValueChannel", C.c_int32), ("imageIndex", C.c_int32)]


class Image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pixelStride", C.c_int32), ("pixels", C.c_void_p)]


class Material(C.Structure):
    _fields_ = [("type", C.c_int32), ("albedo", Texture), ("glossiness", Texture), ("emission", Texture),
                ("metallic", Texture), ("parameter", C.c_float)]


class Entity(C.Structure):
    _fields_ = [("type", C.c_int32), ("moving", C.c_int32), ("rotation", Float4), ("position", Float3),
                ("destinationOffset", Float3), ("timeRange", Float2), ("materialIndex", C.c_int32),
                ("size", Float3), ("contentIndex", C.c_int32)]


class Triangle(C.Structure):
    """RT/EntityTypes/Triangle.cs:8-12 byte for byte (96 bytes): Data {v2-v0, v1-v0, v0}, Normals, TextureCoordinates."""
    _fields_ = [("data", Float3 * 3), ("normals", Float3 * 3), ("textureCoordinates", Float2 * 3)]


class SceneDesc(C.Structure):
    _fields_ = [("entities", C.POINTER(Entity)), ("entityCount", C.c_int32),
                ("materials", C.POINTER(Material)), ("materialCount", C.c_int32),
                ("maxBvhDepth", C.c_int32), ("triangles", C.POINTER(Triangle)), ("triangleCount", C.c_int32),
                ("images", C.POINTER(Image)), ("imageCount", C.c_int32)]


class SceneInfo(C.Structure):
    _fields_ = [("entityCount", C.c_int32), ("materialCount", C.c_int32), ("bvhNodeCount", C.c_int32),
                ("bvhDepth", C.c_int32), ("ldsBytesScene", C.c_int32), ("sceneInLds", C.c_int32),
                ("sceneBytesDevice", C.c_uint64), ("hitSpillBytes", C.c_uint64), ("hitListCapacity", C.c_int32), ("wideCodes", C.c_int32),
                ("thresholdSet", C.c_int32), ("schedulerTune", C.c_int32 * 9)]


class View(C.Structure):
    _fields_ = [("origin", Float3), ("lowerLeftCorner", Float3), ("horizontal", Float3), ("vertical", Float3),
                ("forward", Float3), ("up", Float3), ("right", Float3), ("lensRadius", C.c_float)]


CUBEMAP_UNSIGNED_BYTE, CUBEMAP_SIGNED_HALF = 0, 1
RNG_REFERENCE, RNG_PER_SAMPLE, RNG_PER_SAMPLE_XOROSHIRO = 0, 1, 2


class CubemapDesc(C.Structure):
    _fields_ = [("faceWidth", C.c_int32), ("faceHeight", C.c_int32), ("channelType", C.c_int32), ("pixelStride", C.c_int32),
                ("faces", C.c_void_p)]


class BlueNoiseDesc(C.Structure):
    _fields_ = [("rowStride", C.c_uint32), ("textureCount", C.c_uint32), ("texels", C.c_void_p)]


class StbNoiseDesc(C.Structure):
    _fields_ = [("rowStride", C.c_uint32), ("textureCount", C.c_uint32), ("scalar", C.c_void_p), ("vector2", C.c_void_p),
                ("cosineUnitVector3", C.c_void_p), ("unitVector2", C.c_void_p), ("unitVector3", C.c_void_p)]


class Environment(C.Structure):
    _fields_ = [("skyType", C.c_int32), ("skyBottomColor", Float3), ("skyTopColor", Float3)]


class SampleParams(C.Structure):
    _fields_ = [("size", Float2), ("sliceOffset", C.c_int32), ("sliceDivider", C.c_int32), ("seed", C.c_uint32),
                ("view", View), ("environment", Environment), ("sampleCountRange", C.c_uint32 * 2),
                ("traceDepth", C.c_int32), ("subPixelJitter", C.c_int32), ("noiseColor", C.c_int32),
                ("sampleCountWeightExtrema", Float2), ("diagnosticsStride", C.c_int32), ("noiseTextureIndex", C.c_int32),
                ("rngPolicy", C.c_int32)]


class AccumBuffers(C.Structure):
    _fields_ = [("color", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p),
                ("sampleCountWeight", C.c_void_p)]


class AdaptiveFeed(C.Structure):
    _fields_ = [("extremaIn", C.c_void_p), ("extremaOut", C.c_void_p), ("lag", C.c_int32), ("reserved", C.c_int32)]


LogCallback = C.CFUNCTYPE(None, C.c_int32, C.c_char_p, C.c_char_p, C.c_void_p)


# RtowContextFlags
CONTEXT_EXACT_TIES_ALWAYS, CONTEXT_EXACT_TIES_NEVER, CONTEXT_REFERENCE_DIAGNOSTICS, CONTEXT_NO_CAMERA_RAY_LISTS, CONTEXT_NO_CHUNK_ORDER, CONTEXT_FORCE_WIDE_CODES, CONTEXT_NO_THRESHOLD_TUNING, CONTEXT_NO_CHAIN_FUSION = 1, 2, 4, 8, 16, 32, 64, 128
CONTEXT_NODE_IMAGE_64 = 256   # development: 64-byte tree nodes in LDS where the sphere kernels would walk the 80-byte image
CONTEXT_UNPRUNED_CAMERA_RAY_LISTS = 512   # development: camera-ray lists keep every node whose leaf boxes the pixel's beam meets
# RtowGatherMask
GATHER_COLOR, GATHER_NORMAL, GATHER_ALBEDO, GATHER_SAMPLE_COUNT_WEIGHT, GATHER_ALL, GATHER_NO_BATCH_WAIT, GATHER_LOOPBACK = 1, 2, 4, 8, 15, 16, 32


class ContextOptions(C.Structure):
    _fields_ = [("deviceOrdinal", C.c_int32), ("logCallback", LogCallback), ("logCallbackData", C.c_void_p),
                ("logCallbackLevel", C.c_int32), ("flags", C.c_uint32), ("ldsSceneBudgetBytes", C.c_int32), ("schedulerTune", C.c_int32 * 9),
                ("hitListCapacity", C.c_int32), ("sliceBlockThreads", C.c_int32)]


class CommId(C.Structure):
    _fields_ = [("bytes", C.c_char * 128)]


class HybridPlan(C.Structure):
    _fields_ = [("tileCount", C.c_int32), ("groupCount", C.c_int32), ("tile", C.c_int32), ("group", C.c_int32),
                ("sliceOffset", C.c_int32), ("sliceDivider", C.c_int32), ("samples", C.c_uint32), ("seed", C.c_uint32)]


class Metrics(C.Structure):
    _fields_ = [("totalRayCount", C.c_int32), ("totalSamples", C.c_int32), ("sampleCountWeightExtrema", Float2),
                ("sampleCountExtrema", C.c_int32 * 2), ("totalRayCount64", C.c_int64), ("totalSamples64", C.c_int64)]


class CombineParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("debugMode", C.c_int32), ("ldrAlbedo", C.c_int32)]


# RtowDenoiseFlags
RTOW_DENOISE_DEMODULATE_ALBEDO = 1
# recommended settings of rtowDenoiseDevice (include/rtow.h; the sigmas are tuned on tests/test_gpu_denoise.py's quality test)
DENOISE_DEFAULT_ITERATIONS = 5
DENOISE_DEFAULT_NORMAL_SHARPNESS = 4
DENOISE_DEFAULT_COLOR_SIGMA = 0.5
DENOISE_DEFAULT_ALBEDO_SIGMA = 0.5
DENOISE_DEFAULT_FLAGS = RTOW_DENOISE_DEMODULATE_ALBEDO


class DenoiseParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("normalSharpness", C.c_int32),
                ("colorSigma", C.c_float), ("albedoSigma", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


class Ray(C.Structure):
    """RtowRay (32 bytes): Ray.Origin, Ray.Time, Ray.Direction (not normalised by the library), pad."""
    _fields_ = [("origin", Float3), ("time", C.c_float), ("direction", Float3), ("pad", C.c_float)]


# numpy view of an RtowRay array: rays["origin"], rays["time"], rays["direction"]
RAY_DTYPE = [("origin", "<f4", (3,)), ("time", "<f4"), ("direction", "<f4", (3,)), ("pad", "<f4")]


class RayInterval(C.Structure):
    """RtowRayInterval (8 bytes): tMin, tMax in parameter units of the ray's direction as stored."""
    _fields_ = [("tMin", C.c_float), ("tMax", C.c_float)]


# numpy view of an RtowRayInterval array
RAY_INTERVAL_DTYPE = [("tMin", "<f4"), ("tMax", "<f4")]


class HitBuffers(C.Structure):
    """RtowHitBuffers: device pointers, any may be NULL (not written), not all three."""
    _fields_ = [("distance", C.c_void_p), ("entityIndex", C.c_void_p), ("normal", C.c_void_p)]


class TraceViewParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("view", View), ("time", C.c_float), ("reserved", C.c_int32)]


# RtowReprojectFlags
RTOW_REPROJECT_MATCH_ENTITY = 1
# recommended settings of rtowReprojectAccumDevice (include/rtow.h)
REPROJECT_DEFAULT_DEPTH_TOLERANCE = 0.01
REPROJECT_DEFAULT_MAX_HISTORY = 64
REPROJECT_DEFAULT_FLAGS = RTOW_REPROJECT_MATCH_ENTITY


class ReprojectParams(C.Structure):
    """RtowReprojectParams (112 bytes): previousView is the view the carried accumulators and previousHits were made with."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("previousView", View), ("depthTolerance", C.c_float), ("maxHistory", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


# RtowUpsampleMode
RTOW_UPSAMPLE_POINT, RTOW_UPSAMPLE_BILINEAR, RTOW_UPSAMPLE_GUIDED = 0, 1, 2
# RtowUpsampleFlags
RTOW_UPSAMPLE_MATCH_ENTITY = 1
RTOW_UPSAMPLE_DEMODULATE_ALBEDO = 2
# recommended settings of rtowUpsampleDevice (include/rtow.h; sharpness and tolerance are the best point of profiles/upsample_timing.py's grid on
# tests/test_gpu_upsample.py's quality test, profiles/r09_upsample.json)
UPSAMPLE_DEFAULT_MODE = RTOW_UPSAMPLE_GUIDED
UPSAMPLE_DEFAULT_NORMAL_SHARPNESS = 0
UPSAMPLE_DEFAULT_DEPTH_TOLERANCE = 0.2
UPSAMPLE_DEFAULT_FLAGS = RTOW_UPSAMPLE_MATCH_ENTITY | RTOW_UPSAMPLE_DEMODULATE_ALBEDO
UPSAMPLE_MAX_SIZE = 16384


class UpsampleParams(C.Structure):
    """RtowUpsampleParams (36 bytes): src = the rendered size, dst = the displayed size."""
    _fields_ = [("srcWidth", C.c_int32), ("srcHeight", C.c_int32), ("dstWidth", C.c_int32), ("dstHeight", C.c_int32), ("mode", C.c_int32),
                ("normalSharpness", C.c_int32), ("depthTolerance", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


# rtowBuildPixelListDevice / rtowSamplePixelsDevice (include/rtow.h): a pixel list is 4 + capacity uint32 words of device memory
PIXEL_LIST_HEADER_WORDS = 4
PIXEL_LIST_MAX_PIXELS = 1 << 27          # RTOW_PIXEL_LIST_MAX_PIXELS: the largest W * H a list may name pixels of
SAMPLE_PIXELS_MAX_BATCHES = 16           # batches one rtowSamplePixelsDevice call may chain


class PixelList(C.Structure):
    """RtowPixelList (16 bytes): words[0] = how many pixels qualified (may exceed capacity), words[1..3] = 0, words[4 + i] = row * W + col."""
    _fields_ = [("words", C.c_void_p), ("capacity", C.c_uint32)]


class PixelListParams(C.Structure):
    """RtowPixelListParams (44 bytes): the frame, the rectangle [x0, x1) x [y0, y1), the row slice, and the sample count below which a pixel qualifies."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("sliceOffset", C.c_int32), ("sliceDivider", C.c_int32), ("minSampleCount", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


def pixel_list_bytes(capacity):
    """RTOW_PIXEL_LIST_BYTES(capacity)"""
    return (PIXEL_LIST_HEADER_WORDS + int(capacity)) * 4


def pixel_list_scratch_bytes(width, height):
    """RTOW_PIXEL_LIST_SCRATCH_BYTES(w, h): one word per 8 x 8 tile of the frame"""
    return ((int(width) + 7) // 8) * ((int(height) + 7) // 8) * 4


# rtowRecordPathsDevice (include/rtow.h): one sample of every listed pixel, segment by segment
PATH_SELECT_INDEX, PATH_SELECT_BRIGHTEST = 0, 1                                                      # RtowPathSelect
PATH_SKY, PATH_LAMBERT, PATH_METAL, PATH_GLOSSY, PATH_REFRACT, PATH_REFLECT = 0, 1, 2, 3, 4, 5      # RtowPathEvent
PATH_EVENTS = (PATH_SKY, PATH_LAMBERT, PATH_METAL, PATH_GLOSSY, PATH_REFRACT, PATH_REFLECT)
# RtowPathSegment.info
PATH_INFO_MATERIAL_MASK = 0xFFFF          # 0xFFFF: the sky segment
PATH_INFO_EVENT_SHIFT, PATH_INFO_EVENT_MASK = 16, 7
PATH_INFO_PERFECT_SPECULAR = 1 << 19
# RtowPathSummary.flags
PATH_FLAG_SUCCEEDED, PATH_FLAG_NO_SUCH_SAMPLE, PATH_FLAG_NOT_A_PIXEL = 1, 2, 4
PATH_SKY_REACH = 99999.0                  # a sky segment's `to` is direction * this (JOBS/SampleBatchJob.cs:346)


class PathSegment(C.Structure):
    """RtowPathSegment (96 bytes): depth d of the recorded sample."""
    _fields_ = [("origin", Float3), ("distance", C.c_float), ("direction", Float3), ("entityIndex", C.c_int32), ("to", Float3), ("info", C.c_uint32),
                ("normal", Float3), ("randomEvents", C.c_float), ("attenuation", Float3), ("pad0", C.c_float), ("emission", Float3), ("pad1", C.c_float)]


# (the C member `from` is a Python keyword: the mirrors call it "origin", the numpy types keep the C name)
PATH_SEGMENT_DTYPE = [("from", "<f4", (3,)), ("distance", "<f4"), ("direction", "<f4", (3,)), ("entityIndex", "<i4"), ("to", "<f4", (3,)), ("info", "<u4"),
                      ("normal", "<f4", (3,)), ("randomEvents", "<f4"), ("attenuation", "<f4", (3,)), ("pad0", "<f4"), ("emission", "<f4", (3,)), ("pad1", "<f4")]


class PathSummary(C.Structure):
    """RtowPathSummary (68 bytes): the recorded sample of one list entry."""
    _fields_ = [("pixel", C.c_int32), ("sampleIndex", C.c_int32), ("sampleCount", C.c_int32), ("segmentCount", C.c_int32), ("flags", C.c_uint32),
                ("time", C.c_float), ("luminance", C.c_float), ("randomEvents", C.c_float), ("color", Float3), ("normal", Float3), ("albedo", Float3)]


PATH_SUMMARY_DTYPE = [("pixel", "<i4"), ("sampleIndex", "<i4"), ("sampleCount", "<i4"), ("segmentCount", "<i4"), ("flags", "<u4"), ("time", "<f4"),
                      ("luminance", "<f4"), ("randomEvents", "<f4"), ("color", "<f4", (3,)), ("normal", "<f4", (3,)), ("albedo", "<f4", (3,))]


class RecordPathsParams(C.Structure):
    """RtowRecordPathsParams (16 bytes): select (PATH_SELECT_*), sampleIndex (0 under BRIGHTEST); flags and reserved are 0."""
    _fields_ = [("select", C.c_int32), ("sampleIndex", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class SurfaceBuffers(C.Structure):
    """RtowSurfaceBuffers (48 bytes): device pointers, any may be NULL (not written), not all six."""
    _fields_ = [("albedo", C.c_void_p), ("emission", C.c_void_p), ("texCoord", C.c_void_p), ("metallicGlossiness", C.c_void_p),
                ("materialIndex", C.c_void_p), ("materialInfo", C.c_void_p)]


class ShadeHitsParams(C.Structure):
    """RtowShadeHitsParams (36 bytes): the sky a miss takes its albedo from; flags and reserved are 0."""
    _fields_ = [("environment", Environment), ("flags", C.c_int32), ("reserved", C.c_int32)]


# numpy element type and shape of every RtowSurfaceBuffers member, in the struct's order
SURFACE_OUTPUTS = {"albedo": ("<f4", 3), "emission": ("<f4", 3), "texCoord": ("<f4", 2), "metallicGlossiness": ("<f4", 2),
                   "materialIndex": ("<i4", 1), "materialInfo": ("<u4", 1)}
# RtowSurfaceBuffers.materialInfo
MATERIAL_INFO_TYPE_MASK = 0xFF
MATERIAL_INFO_PERFECT_SPECULAR = 0x100
MATERIAL_INFO_MISS = 0xFFFFFFFF


# rtowTraceGuideRaysDevice / rtowTraceGuideViewDevice (include/rtow.h)
GUIDE_MAX_BOUNCES = 64          # RTOW_GUIDE_MAX_BOUNCES
GUIDE_DEFAULT_MAX_BOUNCES = 8
# RtowGuideBuffers.end
GUIDE_END_SKY, GUIDE_END_SURFACE, GUIDE_END_CUT = 0, 1, 2


class GuideParams(C.Structure):
    """RtowGuideParams (12 bytes): maxBounces 0..64; flags and reserved are 0."""
    _fields_ = [("maxBounces", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class GuideBuffers(C.Structure):
    """RtowGuideBuffers (64 bytes): device pointers, any may be NULL (not written), not all.  hits / rays: the last segment of the specular chain."""
    _fields_ = [("hits", HitBuffers), ("rays", C.c_void_p), ("throughput", C.c_void_p), ("pathDistance", C.c_void_p), ("bounces", C.c_void_p), ("end", C.c_void_p)]


# numpy element type and shape of every RtowGuideBuffers member, in the struct's order ("rays": abi.RAY_DTYPE)
GUIDE_OUTPUTS = {"distance": ("<f4", 1), "entityIndex": ("<i4", 1), "normal": ("<f4", 3), "rays": (RAY_DTYPE, 1), "throughput": ("<f4", 3),
                 "pathDistance": ("<f4", 1), "bounces": ("<i4", 1), "end": ("u1", 1)}


def guide_buffers(pointers):
    """RtowGuideBuffers from {name of GUIDE_OUTPUTS: device address}; a name that is missing (or None) is NULL"""
    at = lambda k: pointers.get(k) or None
    return GuideBuffers(HitBuffers(at("distance"), at("entityIndex"), at("normal")), at("rays"), at("throughput"), at("pathDistance"), at("bounces"), at("end"))


def denoise_scratch_bytes(width, height):
    """RTOW_DENOISE_SCRATCH_BYTES(w, h): the ping-pong float3 colour buffer of the levels"""
    return int(width) * int(height) * 12


# rtowAccumulateMomentsDevice / rtowDenoiseVarianceDevice (include/rtow.h)
MOMENTS_MAX_BATCHES = 16                 # colour buffers one rtowAccumulateMomentsDevice call reads
DENOISE_VARIANCE_UNKNOWN = -1.0          # outVariance where a pixel has no variance estimate
# recommended settings of rtowDenoiseVarianceDevice: the best point of profiles/denoise_variance_timing.py's grid on tests/test_gpu_denoise_variance.py's two
# quality frames (profiles/r12_denoise_variance.json); colorSigma multiplies the local standard deviation here
DENOISE_VARIANCE_DEFAULT_ITERATIONS = 5
DENOISE_VARIANCE_DEFAULT_NORMAL_SHARPNESS = 2
DENOISE_VARIANCE_DEFAULT_COLOR_SIGMA = 2.0
DENOISE_VARIANCE_DEFAULT_ALBEDO_SIGMA = 0.125
DENOISE_VARIANCE_DEFAULT_FLAGS = RTOW_DENOISE_DEMODULATE_ALBEDO


def moments_bytes(pixel_count):
    """RTOW_MOMENTS_BYTES(pixelCount): (s1, s2, n) float3 per pixel"""
    return int(pixel_count) * 12


def denoise_variance_scratch_bytes(width, height):
    """RTOW_DENOISE_VARIANCE_SCRATCH_BYTES(w, h): the ping-pong float3 colour plane and two float variance planes"""
    return int(width) * int(height) * 20


# rtowReprojectMomentsDevice / rtowEstimateMomentsDevice (include/rtow.h): the moments carried across a camera move, and estimated where there is no history
# RtowEstimateMomentsFlags
RTOW_ESTIMATE_MOMENTS_MATCH_ENTITY = 1
ESTIMATE_MOMENTS_MATCH_ENTITY = RTOW_ESTIMATE_MOMENTS_MATCH_ENTITY
ESTIMATE_MOMENTS_RADIUS = 3              # the neighbourhood is 7 x 7
ESTIMATE_MOMENTS_BATCHES = 2.0           # n of an estimated triple: the neighbourhood's weighted moments as two batches
# recommended settings: the point profiles/temporal_moments_timing.py's grid picks on tests/test_gpu_temporal_moments.py's two quality frames
# (profiles/r13_temporal_moments.json)
REPROJECT_MOMENTS_DEFAULT_MAX_BATCHES = 16
ESTIMATE_MOMENTS_DEFAULT_MIN_BATCHES = 8
ESTIMATE_MOMENTS_DEFAULT_MIN_TAPS = 2
ESTIMATE_MOMENTS_DEFAULT_NORMAL_SHARPNESS = 4
ESTIMATE_MOMENTS_DEFAULT_DEPTH_TOLERANCE = 0.01
ESTIMATE_MOMENTS_DEFAULT_FLAGS = RTOW_ESTIMATE_MOMENTS_MATCH_ENTITY


class EstimateMomentsParams(C.Structure):
    """RtowEstimateMomentsParams (32 bytes)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("minBatches", C.c_int32), ("minTaps", C.c_int32), ("normalSharpness", C.c_int32),
                ("depthTolerance", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


# rtowNoiseMaskDevice (include/rtow.h): from the moments to the mask of the pixels that get the next batches
# RtowNoiseMaskFlags
RTOW_NOISE_MASK_ABSOLUTE = 1
RTOW_NOISE_MASK_UNKNOWN_QUALIFIES = 2
NOISE_MASK_ABSOLUTE, NOISE_MASK_UNKNOWN_QUALIFIES = RTOW_NOISE_MASK_ABSOLUTE, RTOW_NOISE_MASK_UNKNOWN_QUALIFIES
NOISE_MASK_HISTOGRAM_BINS = 64           # RtowNoiseStats.histogram: one bin per binade of the filtered error g
NOISE_MASK_MAX_DILATE = 3
NOISE_MASK_UNKNOWN = -1.0                # outError where a pixel has no estimate
# recommended settings: the best point of profiles/noise_mask_timing.py's grid (profiles/r14_noise_mask.json): the refined frame has 0.82 of the squared error and
# 0.74 of the relative squared error of a uniform frame with at least as many samples (starting point 0.01 / 2^-6 / 1 / n / 4: 0.90 and 0.78)
NOISE_MASK_DEFAULT_ERROR_THRESHOLD = 0.0025
NOISE_MASK_DEFAULT_LUMINANCE_FLOOR = 2.0 ** -4
NOISE_MASK_DEFAULT_DILATE = 1
NOISE_MASK_DEFAULT_BUDGET_DIVISOR = 2    # maxQualifying = width * height // this
NOISE_MASK_DEFAULT_FLAGS = RTOW_NOISE_MASK_UNKNOWN_QUALIFIES


class NoiseMaskParams(C.Structure):
    """RtowNoiseMaskParams (32 bytes)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("errorThreshold", C.c_float), ("luminanceFloor", C.c_float), ("dilate", C.c_int32),
                ("maxQualifying", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class NoiseStats(C.Structure):
    """RtowNoiseStats (288 bytes): what the device leaves in outStats"""
    _fields_ = [("known", C.c_uint32), ("unknown", C.c_uint32), ("qualifying", C.c_uint32), ("masked", C.c_uint32), ("threshold", C.c_float),
                ("maxError", C.c_float), ("reserved", C.c_uint32 * 2), ("histogram", C.c_uint32 * NOISE_MASK_HISTOGRAM_BINS)]


def noise_mask_scratch_bytes():
    """RTOW_NOISE_MASK_SCRATCH_BYTES: one record"""
    return 288


def noise_bin_lower_bound(b):
    """L(b): the smallest g of histogram bin b - 0 for bin 0, else 2^(b-31)"""
    b = int(b)
    if not 0 <= b < NOISE_MASK_HISTOGRAM_BINS:
        raise ValueError("bin %d is not in 0..63" % b)
    return 0.0 if b == 0 else 2.0 ** (b - 31)


# rtowRectifyHistoryDevice (include/rtow.h): carried history the new view's first batches refute is cut down or dropped
# RtowRectifyFlags
RTOW_RECTIFY_MATCH_ENTITY = 1
RECTIFY_MATCH_ENTITY = RTOW_RECTIFY_MATCH_ENTITY
RECTIFY_MAX_RADIUS = 3
# recommended settings: the point profiles/rectify_history_timing.py's grid picks on tests/test_gpu_rectify_history.py's quality frames
# (profiles/r15_rectify_history.json): a narrow band judged only where all nine taps of a 3 x 3 neighbourhood lie on the pixel's own surface; the guides as
# rtowEstimateMomentsDevice's.  The gain is small: 0.977 of the carried frame's squared error on the metal and glass pixels after a 4 degree orbit, none after a 2 % dolly
RECTIFY_DEFAULT_RADIUS = 1
RECTIFY_DEFAULT_MIN_TAPS = 9
RECTIFY_DEFAULT_NORMAL_SHARPNESS = 4
RECTIFY_DEFAULT_DEPTH_TOLERANCE = 0.01
RECTIFY_DEFAULT_SIGMA_SCALE = 0.5
RECTIFY_DEFAULT_RELATIVE_TOLERANCE = 0.125
RECTIFY_DEFAULT_FLAGS = RTOW_RECTIFY_MATCH_ENTITY


class RectifyParams(C.Structure):
    """RtowRectifyParams (40 bytes)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("radius", C.c_int32), ("minTaps", C.c_int32), ("normalSharpness", C.c_int32),
                ("depthTolerance", C.c_float), ("sigmaScale", C.c_float), ("relativeTolerance", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


class RectifyStats(C.Structure):
    """RtowRectifyStats (16 bytes): what the device leaves in outStats; judged = kept + cut + dropped"""
    _fields_ = [("judged", C.c_uint32), ("kept", C.c_uint32), ("cut", C.c_uint32), ("dropped", C.c_uint32)]


# rtowMeterExposureDevice / rtowFinalizeToneMappedDevice (include/rtow.h): auto-exposure metering on the device and the finalize pass with an exposure and a tone curve
# RtowToneCurve
RTOW_TONE_CLAMP = 0
RTOW_TONE_ACES_FITTED = 1
RTOW_TONE_ACES_FILM = 2
TONE_CLAMP, TONE_ACES_FITTED, TONE_ACES_FILM = RTOW_TONE_CLAMP, RTOW_TONE_ACES_FITTED, RTOW_TONE_ACES_FILM
TONE_CURVES = (TONE_CLAMP, TONE_ACES_FITTED, TONE_ACES_FILM)
TONE_DEFAULT_CURVE = TONE_ACES_FITTED          # the curve of the line the reference left commented out (JOBS/FinalizeTexturesJob.cs:28)
TONE_DEFAULT_EXPOSURE = 1.0
EXPOSURE_BINS = 256                            # eight per octave from 2^-16; bin 255 also takes everything from 2^16 up
# recommended metering: the upper half of the metered pixels without the brightest 5 % (a sun, a lamp) mapped to middle grey, within eight stops either way, at once
EXPOSURE_DEFAULT_LOW_PERMILLE = 500
EXPOSURE_DEFAULT_HIGH_PERMILLE = 950
EXPOSURE_DEFAULT_COMPENSATION = C.c_float(-2.4739311883324124).value      # log2(0.18) as float32: the trimmed mean lands on middle grey
EXPOSURE_DEFAULT_MIN_STOPS = -8.0
EXPOSURE_DEFAULT_MAX_STOPS = 8.0
EXPOSURE_DEFAULT_RATE = 1.0


def exposure_scratch_bytes():
    """RTOW_EXPOSURE_SCRATCH_BYTES: a 256-bin partial histogram for each of at most 256 workgroups"""
    return 256 * 256 * 4


class ExposureParams(C.Structure):
    """RtowExposureParams (40 bytes)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("lowPermille", C.c_int32), ("highPermille", C.c_int32), ("compensation", C.c_float),
                ("minStops", C.c_float), ("maxStops", C.c_float), ("rate", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


class ExposureState(C.Structure):
    """RtowExposureState (1056 bytes): DEVICE memory of the caller's that lives across frames; zero-filled = no history"""
    _fields_ = [("exposure", C.c_float), ("stops", C.c_float), ("targetStops", C.c_float), ("meanLog2", C.c_float), ("valid", C.c_uint32), ("metered", C.c_uint32),
                ("ignored", C.c_uint32), ("reserved", C.c_uint32), ("histogram", C.c_uint32 * 256)]


class ToneMapParams(C.Structure):
    """RtowToneMapParams (24 bytes)"""
    _fields_ = [("pixelCount", C.c_int32), ("curve", C.c_int32), ("exposure", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


# rtowBloomDevice (include/rtow.h): HDR bloom on the scene-referred colour, between the upsample and the meter
RTOW_BLOOM_KARIS_AVERAGE = 1                   # RtowBloomFlags: the first downsample weights its taps by 1 / (1 + exposed luminance)
BLOOM_KARIS_AVERAGE = RTOW_BLOOM_KARIS_AVERAGE
BLOOM_MAX_LEVELS = 8
BLOOM_DEFAULT_LEVELS = 6
BLOOM_DEFAULT_THRESHOLD = 1.0                  # in exposed units: where the tone curve starts to compress
BLOOM_DEFAULT_KNEE = 0.5
BLOOM_DEFAULT_SCATTER = 0.7
BLOOM_DEFAULT_INTENSITY = 0.05                 # the host's taste; a low share keeps a frame without highlights as it is
BLOOM_DEFAULT_EXPOSURE = 1.0
BLOOM_DEFAULT_FLAGS = RTOW_BLOOM_KARIS_AVERAGE


def bloom_levels(w, h, levels=BLOOM_MAX_LEVELS):
    """the sizes of mip 1 .. levels: mip k is ceil(w / 2^k) x ceil(h / 2^k)"""
    return [(-(-int(w) // (1 << k)), -(-int(h) // (1 << k))) for k in range(1, int(levels) + 1)]


def bloom_scratch_bytes(w, h):
    """RTOW_BLOOM_SCRATCH_BYTES(w, h): the pyramid, 16 bytes per texel, bounded for eight levels of every size"""
    return 16 * (int(w) * int(h) // 3 + int(w) + int(h) + 9)


class BloomParams(C.Structure):
    """RtowBloomParams (40 bytes)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32), ("threshold", C.c_float), ("knee", C.c_float), ("scatter", C.c_float),
                ("intensity", C.c_float), ("exposure", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


class CameraRayListStats(C.Structure):
    """RtowCameraRayListStats (96 bytes)"""
    _fields_ = [("pixelsWithEntries", C.c_uint64 * 9), ("pixelsWithoutList", C.c_uint64), ("ownedPixels", C.c_uint64), ("pruned", C.c_int32), ("valid", C.c_int32)]


# every symbol include/rtow.h declares (tests/test_abi.py checks the library exports all of them)
EXPORTED_SYMBOLS = [
    "rtowGetApiVersion", "rtowErrorString", "rtowCreateContext", "rtowDestroyContext", "rtowUploadScene",
    "rtowUploadSkyCubemap", "rtowUploadBlueNoise", "rtowUploadStbNoise", "rtowGetSceneInfo", "rtowSampleBatch", "rtowSampleBatchDevice", "rtowGetLastSampleKernelMs",
    "rtowReduceMetricsDevice", "rtowCombineDevice", "rtowFinalizeDevice", "rtowAddAccumDevice", "rtowDeviceAlloc", "rtowDeviceFree",
    "rtowDeviceCopy", "rtowDeviceMemset", "rtowSynchronize", "rtowGetBatchStatus", "rtowRegisterHostBuffer", "rtowUnregisterHostBuffer",
    "rtowSampleBatchChainDevice", "rtowSampleBatchChain", "rtowCommSetLibraryPath", "rtowCommGetUniqueId", "rtowCommInit", "rtowCommDestroy", "rtowGatherRowsDevice",
    "rtowHybridPlan", "rtowExchangeAccumDevice", "rtowSampleBatchGroupDevice",
    "rtowCombineFinalizeDevice", "rtowReduceMetricsDeviceAsync", "rtowProbeNearestHit", "rtowSampleBatchChainAdaptiveDevice",
    "rtowDenoiseDevice", "rtowTraceRaysDevice", "rtowTraceViewDevice", "rtowReprojectAccumDevice", "rtowShadeHitsDevice",
    "rtowTraceRaysIntervalDevice", "rtowTraceOcclusionDevice", "rtowProbeNearestHitInterval", "rtowUpsampleDevice",
    "rtowBuildPixelListDevice", "rtowSamplePixelsDevice", "rtowTraceGuideRaysDevice", "rtowTraceGuideViewDevice",
    "rtowAccumulateMomentsDevice", "rtowDenoiseVarianceDevice", "rtowReprojectMomentsDevice", "rtowEstimateMomentsDevice",
    "rtowNoiseMaskDevice", "rtowRectifyHistoryDevice", "rtowReprojectAccumBilinearDevice",
    "rtowMeterExposureDevice", "rtowFinalizeToneMappedDevice", "rtowRecordPathsDevice", "rtowGetCameraRayListStats",
    "rtowBloomDevice",
]
