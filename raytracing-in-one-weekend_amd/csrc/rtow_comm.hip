// rtow_comm.hip - the multi-GPU row transport of the C ABI (include/rtow.h): the RCCL loader, rtowComm*, rtowGatherRowsDevice, rtowHybridPlan and
// rtowExchangeAccumDevice, with the two kernels that pack / scatter and fold rows.  One process per GPU; rank g owns the rows with row % world == g.
// Every role a rank can play (loop-back, peer, root, exchange) is written in the same few steps: reserveStaging, copyRankRows, postGroup, gatherEnds.
#include <dlfcn.h>

#include <array>
#include <cstring>
#include <string>

#include "rtow_context.h"
#include "rtow_comm_plan.h"

using namespace rtow;

namespace {

// ---- RCCL, loaded on first use: hosts that drive one GPU never map it, and a process that already holds a copy (PyTorch ships its own
// librccl.so.1) shares that copy.  Only the point-to-point calls the row gather needs; types restated from <rccl/rccl.h> (ROCm 7.2:
// NCCL_UNIQUE_ID_BYTES 128, ncclFloat32 = 7, ncclSuccess = 0) so that the library has no link-time dependency on RCCL. ----
struct RcclUniqueId { char internal[128]; };
static_assert(sizeof(RcclUniqueId) == sizeof(RtowCommId), "RtowCommId carries an ncclUniqueId");
struct RcclApi {
    void* handle = nullptr;
    int (*GetUniqueId)(RcclUniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok() const { return handle && GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString; }
};
constexpr int kRcclFloat32 = 7;

std::mutex gRcclMu;
std::string gRcclPath;        // rtowCommSetLibraryPath: the file to load instead of the default search
std::string gRcclLoadError;   // why the last load attempt failed (dlerror() is per thread and may be null by the time it is logged)
bool gRcclLoaded = false;

RcclApi* rccl()
{
    static RcclApi api;
    std::lock_guard<std::mutex> lock(gRcclMu);
    if (api.ok()) return &api;
    static const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    if (!gRcclPath.empty()) {
        h = dlopen(gRcclPath.c_str(), RTLD_NOW | RTLD_LOCAL);
    } else {
        for (const char* n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL))) break;     // a copy this process already holds
        if (!h) for (const char* n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    }
    if (!h) {
        const char* e = dlerror();
        gRcclLoadError = e ? e : "dlopen failed";
        return nullptr;
    }
    api.handle = h;
    api.GetUniqueId = (int (*)(RcclUniqueId*))dlsym(h, "ncclGetUniqueId");
    api.CommInitRank = (int (*)(void**, int, RcclUniqueId, int))dlsym(h, "ncclCommInitRank");
    api.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    api.GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
    api.GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
    api.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclSend");
    api.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclRecv");
    api.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!api.ok()) { gRcclLoadError = "the library does not export the nccl* entry points the row gather needs"; return nullptr; }
    gRcclLoaded = true;
    return &api;
}

#define RCCL_TRY(ctx, api, expr)                                                                       \
    do {                                                                                               \
        const int _r = (expr);                                                                         \
        if (_r != 0) {                                                                                 \
            logf(ctx, 2, "rccl", "%s failed: %s (%s:%d)", #expr, (api)->GetErrorString(_r), __FILE__, __LINE__); \
            return RTOW_ERROR_LAUNCH_FAILURE;                                                          \
        }                                                                                              \
    } while (0)

// ------------------------------------------------------------------------------------------------------------
// rtowGatherRowsDevice: rows first, first + step, ... of a full-frame buffer <-> one contiguous block (what travels over xGMI).
// HBM bound, 4 B read + 4 B written per float; at most 11 floats per owned pixel per batch.
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) copy_rows_kernel(T* frame, T* packed, unsigned rowUnits, unsigned rows, unsigned first, unsigned step, int toFrame)
{
    // one row per blockIdx.y slice, grid-stride inside the row: no division per element
    for (unsigned k = blockIdx.y; k < rows; k += gridDim.y) {
        T* f = frame + ((size_t)first + (size_t)k * step) * rowUnits;
        T* q = packed + (size_t)k * rowUnits;
        for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < rowUnits; j += gridDim.x * blockDim.x) {
            if (toFrame) f[j] = q[j];
            else q[j] = f[j];
        }
    }
}

hipError_t launchCopyRows(float* frame, float* packed, unsigned rowFloats, unsigned rows, unsigned first, unsigned step, bool toFrame, hipStream_t stream)
{
    if ((size_t)rows * rowFloats == 0) return hipSuccess;
    // rows travel as 16-byte units when every row starts on a 16-byte boundary in both buffers
    const bool wide = (rowFloats & 3u) == 0u && ((reinterpret_cast<uintptr_t>(frame) | reinterpret_cast<uintptr_t>(packed)) & 15u) == 0u;
    const unsigned units = wide ? rowFloats / 4u : rowFloats;
    const unsigned bx = units < 256u * 8u ? (units + 255u) / 256u : 8u;
    const unsigned by = rows < 4096u ? rows : 4096u;
    if (wide) hipLaunchKernelGGL(copy_rows_kernel<float4>, dim3(bx, by), dim3(256), 0, stream, reinterpret_cast<float4*>(frame), reinterpret_cast<float4*>(packed), units, rows, first, step, toFrame ? 1 : 0);
    else hipLaunchKernelGGL(copy_rows_kernel<float>, dim3(bx, by), dim3(256), 0, stream, frame, packed, units, rows, first, step, toFrame ? 1 : 0);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------
// rtowExchangeAccumDevice: accum[row] += src_0[row]; accum[row] += src_1[row]; ... for the rows first, first + step, ... of a full-frame buffer,
// in group order with one rounding per addition - what `groups` successive add passes compute - in ONE pass that reads and writes accum once.
// Source g is the rank's own partial sum (frame layout, in place) for g == own, else region g of the receive block (packed rows).
// ------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T add_units(T a, T b);
template <> __device__ __forceinline__ float add_units<float>(float a, float b) { return a + b; }
template <> __device__ __forceinline__ float4 add_units<float4>(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
template <typename T>
__global__ void __launch_bounds__(256) fold_rows_kernel(T* __restrict__ accum, const T* __restrict__ ownPartial, const T* __restrict__ recv, size_t regionUnits, unsigned rowUnits,
                                                        unsigned rows, unsigned first, unsigned step, unsigned groups, unsigned own)
{
    for (unsigned k = blockIdx.y; k < rows; k += gridDim.y) {
        const size_t frameRow = ((size_t)first + (size_t)k * step) * rowUnits, packedRow = (size_t)k * rowUnits;
        for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < rowUnits; j += gridDim.x * blockDim.x) {
            T a = accum[frameRow + j];
            for (unsigned g = 0; g < groups; g++) a = add_units<T>(a, g == own ? ownPartial[frameRow + j] : recv[(size_t)g * regionUnits + packedRow + j]);
            accum[frameRow + j] = a;
        }
    }
}

hipError_t launchFoldRows(float* accum, const float* ownPartial, const float* recv, size_t regionFloats, unsigned rowFloats, unsigned rows, unsigned first, unsigned step,
                          unsigned groups, unsigned own, hipStream_t stream)
{
    if ((size_t)rows * rowFloats == 0 || groups == 0) return hipSuccess;
    const bool wide = (rowFloats & 3u) == 0u && (regionFloats & 3u) == 0u &&
                      ((reinterpret_cast<uintptr_t>(accum) | reinterpret_cast<uintptr_t>(ownPartial) | reinterpret_cast<uintptr_t>(recv)) & 15u) == 0u;
    const unsigned units = wide ? rowFloats / 4u : rowFloats;
    const unsigned bx = units < 256u * 8u ? (units + 255u) / 256u : 8u;
    const unsigned by = rows < 4096u ? rows : 4096u;
    if (wide) hipLaunchKernelGGL(fold_rows_kernel<float4>, dim3(bx, by), dim3(256), 0, stream, reinterpret_cast<float4*>(accum), reinterpret_cast<const float4*>(ownPartial),
                                 reinterpret_cast<const float4*>(recv), regionFloats / 4u, units, rows, first, step, groups, own);
    else hipLaunchKernelGGL(fold_rows_kernel<float>, dim3(bx, by), dim3(256), 0, stream, accum, ownPartial, recv, regionFloats, units, rows, first, step, groups, own);
    return hipGetLastError();
}

// ---- the steps every role of the transport is made of ----
std::array<float*, 4> buffersOf(const RtowAccumBuffers* a) { return a ? std::array<float*, 4>{a->color, a->normal, a->albedo, a->sampleCountWeight} : std::array<float*, 4>{}; }

// The rows of `rank`, selected buffers back to back: full-frame `buffers` -> the region at `packed` (a pack), or back (toFrame: a scatter).  A rank without rows launches nothing.
int copyRankRows(RtowContext ctx, const RowSet& set, float* const buffers[4], int rank, float* packed, bool toFrame, hipStream_t s)
{
    const unsigned rows = set.rows(rank);
    for (int b = 0; b < 4; b++)
        if (set.has(b)) {
            HIP_TRY(ctx, launchCopyRows(buffers[b], packed, (unsigned)(set.width * kAccumComponents[b]), rows, (unsigned)rank, (unsigned)set.world, toFrame, s), RTOW_ERROR_LAUNCH_FAILURE);
            packed += (size_t)rows * set.width * kAccumComponents[b];
        }
    return RTOW_SUCCESS;
}

// The packed-row staging is one send and one receive block per context: a call repacks them only after the previous call's transfers and scatter / fold are over,
// whatever stream that one was given, and frees a block that must grow only when nothing can still be travelling out of or into it.  `s` waits for evGatherDone
// first, so the end of `s` lies behind the end of the previous call: synchronising `s` covers both, and no host wait for the event itself is needed.
int reserveStaging(RtowContext ctx, hipStream_t s, size_t sendFloats, size_t recvFloats)
{
    if (ctx->haveGatherDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evGatherDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
    if (sendFloats * 4u > ctx->dGatherSend.bytes() || recvFloats * 4u > ctx->dGatherRecv.bytes()) HIP_TRY(ctx, hipStreamSynchronize(s), RTOW_ERROR_LAUNCH_FAILURE);
    RTOW_TRY(growDevice(ctx, {{&ctx->dGatherSend, sendFloats * 4u}}));
    RTOW_TRY(growDevice(ctx, {{&ctx->dGatherRecv, recvFloats * 4u}}));
    return RTOW_SUCCESS;
}

// One RCCL group: every transfer in it runs at once, each on its own xGMI link.  post() posts the sends and receives and returns the first code that is not 0.
// A failed ncclSend / ncclRecv must not leave the communicator's group open: it is closed on every path.  `failed` ends with the calls post() makes.
// Ranks without rows (rank >= height) are in nobody's group: RCCL hangs on a zero-count pair that only one side posts, so both sides skip it.
template <typename Post>
int postGroup(RtowContext ctx, RcclApi* api, const char* failed, Post post)
{
    RCCL_TRY(ctx, api, api->GroupStart());
    const int posted = post();
    const int closed = api->GroupEnd();
    if (posted != 0 || closed != 0) {
        logf(ctx, 2, "rccl", "%s %s, ncclGroupEnd %s", failed, api->GetErrorString(posted), api->GetErrorString(closed));
        return RTOW_ERROR_LAUNCH_FAILURE;
    }
    return RTOW_SUCCESS;
}

// the end of a call that used the staging blocks: what the next reserveStaging, on whatever stream, waits for
int gatherEnds(RtowContext ctx, hipStream_t s)
{
    HIP_TRY(ctx, hipEventRecord(ctx->evGatherDone, s), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->haveGatherDone = true;
    return RTOW_SUCCESS;
}

} // namespace

void rtow::releaseComm(RtowContext ctx)
{
    if (ctx->comm) { if (RcclApi* api = rccl()) (void)api->CommDestroy(ctx->comm); ctx->comm = nullptr; }
}

extern "C" {

RTOW_API int rtowCommSetLibraryPath(const char* path)
{
    std::lock_guard<std::mutex> lock(gRcclMu);
    if (gRcclLoaded) return RTOW_ERROR_INVALID_VALUE;              // loaded once per process: the choice comes before the first rtowComm* call
    gRcclPath = path ? path : "";
    return RTOW_SUCCESS;
}

RTOW_API int rtowCommGetUniqueId(RtowCommId* outId)
{
    if (!outId) return RTOW_ERROR_INVALID_VALUE;
    RcclApi* api = rccl();
    if (!api) return RTOW_ERROR_UNSUPPORTED;                       // no librccl.so in this process or on the loader path
    RcclUniqueId id;
    if (api->GetUniqueId(&id) != 0) return RTOW_ERROR_LAUNCH_FAILURE;
    memcpy(outId->bytes, id.internal, sizeof(id.internal));
    return RTOW_SUCCESS;
}

RTOW_API int rtowCommInit(RtowContext ctx, const RtowCommId* id, int32_t rank, int32_t worldSize)
{
    if (!ctx || !id || worldSize < 1 || rank < 0 || rank >= worldSize) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->comm) return RTOW_ERROR_INVALID_VALUE;                // one communicator per context; rtowCommDestroy first
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    RcclApi* api = rccl();
    if (!api) {
        std::lock_guard<std::mutex> l2(gRcclMu);
        logf(ctx, 2, "rccl", "the RCCL library could not be loaded: %s", gRcclLoadError.c_str());
        return RTOW_ERROR_UNSUPPORTED;
    }
    RcclUniqueId uid;
    memcpy(uid.internal, id->bytes, sizeof(uid.internal));
    void* comm = nullptr;
    RCCL_TRY(ctx, api, api->CommInitRank(&comm, worldSize, uid, rank));
    ctx->comm = comm;
    ctx->commRank = rank;
    ctx->commWorld = worldSize;
    logf(ctx, 4, "rccl", "rank %d of %d joined", rank, worldSize);
    return RTOW_SUCCESS;
}

RTOW_API int rtowCommDestroy(RtowContext ctx)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->comm) return RTOW_SUCCESS;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    (void)hipDeviceSynchronize();
    RcclApi* api = rccl();
    if (api) (void)api->CommDestroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->commRank = 0;
    ctx->commWorld = 1;
    return RTOW_SUCCESS;
}

RTOW_API int rtowGatherRowsDevice(RtowContext ctx, int32_t width, int32_t height, int32_t sliceDivider, const RtowAccumBuffers* mine,
                                  const RtowAccumBuffers* frame, int32_t what, int32_t root, void* stream)
{
    if (!ctx || !mine || width <= 0 || height <= 0 || sliceDivider < 1 || (what & ~(RTOW_GATHER_ALL | RTOW_GATHER_NO_BATCH_WAIT | RTOW_GATHER_LOOPBACK)) || !(what & RTOW_GATHER_ALL)) return RTOW_ERROR_INVALID_VALUE;
    const bool waitForBatch = !(what & RTOW_GATHER_NO_BATCH_WAIT);
    const bool wantLoopback = (what & RTOW_GATHER_LOOPBACK) != 0;
    what &= RTOW_GATHER_ALL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int world = ctx->comm ? ctx->commWorld : 1, rank = ctx->comm ? ctx->commRank : 0;
    const bool loopback = wantLoopback && ctx->comm && world == 1;      // one rank sending its rows to itself through the transport (RTOW_GATHER_LOOPBACK)
    if (sliceDivider != world || root < 0 || root >= world) return RTOW_ERROR_INVALID_VALUE;   // rank g owns the rows of slice g: one slice per rank
    if (rank == root && !frame) return RTOW_ERROR_INVALID_VALUE;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // the rows being gathered were written by the last sample batch, whatever stream that was enqueued on (RTOW_GATHER_NO_BATCH_WAIT: they were not)
    if (waitForBatch && ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);

    const RowSet set(width, height, world, what);
    const std::array<float*, 4> mineBuf = buffersOf(mine), frameBuf = buffersOf(frame);
    if (!set.allGiven(mineBuf.data()) || (rank == root && !set.allGiven(frameBuf.data()))) return RTOW_ERROR_INVALID_VALUE;

    if (!loopback && (world == 1 || rank == root)) {
        // the root's own rows: already in place when frame == mine, else copied row by row on the device
        for (int b = 0; b < 4; b++)
            if (set.has(b) && frameBuf[b] != mineBuf[b]) {
                const size_t rowBytes = (size_t)width * kAccumComponents[b] * 4u;
                HIP_TRY(ctx, hipMemcpy2DAsync((uint8_t*)frameBuf[b] + (size_t)rank * rowBytes, (size_t)world * rowBytes, (const uint8_t*)mineBuf[b] + (size_t)rank * rowBytes,
                                              (size_t)world * rowBytes, rowBytes, set.rows(rank), hipMemcpyDeviceToDevice, s), RTOW_ERROR_LAUNCH_FAILURE);
            }
        if (world == 1) return RTOW_SUCCESS;
    }
    RcclApi* api = rccl();
    if (!api) return RTOW_ERROR_UNSUPPORTED;

    if (loopback) {
        // the whole transport path of a peer AND of the root, against itself as rank 0 of 1: pack -> {ncclSend, ncclRecv} in one group -> scatter
        const size_t need = set.packedFloats(0);
        RTOW_TRY(reserveStaging(ctx, s, need, need));
        RTOW_TRY(copyRankRows(ctx, set, mineBuf.data(), 0, ctx->dGatherSend, false, s));
        RTOW_TRY(postGroup(ctx, api, "loop-back gather failed: ncclSend / ncclRecv", [&] {
            const int posted = api->Send(ctx->dGatherSend, need, kRcclFloat32, 0, ctx->comm, s);
            return posted != 0 ? posted : api->Recv(ctx->dGatherRecv, need, kRcclFloat32, 0, ctx->comm, s);
        }));
        RTOW_TRY(copyRankRows(ctx, set, frameBuf.data(), 0, ctx->dGatherRecv, true, s));
    } else if (rank != root) {
        // pack this rank's rows of the selected buffers back to back, one send to the root over this GPU's own xGMI link to it
        const size_t need = set.packedFloats(rank);
        RTOW_TRY(reserveStaging(ctx, s, need, 0));
        RTOW_TRY(copyRankRows(ctx, set, mineBuf.data(), rank, ctx->dGatherSend, false, s));
        if (need) RCCL_TRY(ctx, api, api->Send(ctx->dGatherSend, need, kRcclFloat32, root, ctx->comm, s));
    } else {
        // root: one receive per peer into its own region of the staging block (posted as one group: all seven links run at once), then scatter
        const Regions recv = gatherRegions(set, root);
        RTOW_TRY(reserveStaging(ctx, s, 0, recv.total));
        RTOW_TRY(postGroup(ctx, api, "gather on the root failed: ncclRecv", [&] {
            int posted = 0;
            for (int r = 0; r < world && posted == 0; r++)
                if (r != root && set.packedFloats(r)) posted = api->Recv(ctx->dGatherRecv + recv.offset[(size_t)r], set.packedFloats(r), kRcclFloat32, r, ctx->comm, s);
            return posted;
        }));
        for (int r = 0; r < world; r++)
            if (r != root) RTOW_TRY(copyRankRows(ctx, set, frameBuf.data(), r, ctx->dGatherRecv + recv.offset[(size_t)r], true, s));
    }
    return gatherEnds(ctx, s);
}

RTOW_API int rtowHybridPlan(int32_t worldSize, int32_t rank, int32_t tileCount, uint32_t samplesPerBatch, uint32_t step, RtowHybridPlan* out)
{
    if (!out || worldSize < 1 || rank < 0 || rank >= worldSize || tileCount < 1 || worldSize % tileCount != 0 || step < 1u) return RTOW_ERROR_INVALID_VALUE;
    const int32_t groups = worldSize / tileCount;
    RtowHybridPlan p{};
    p.tileCount = tileCount;
    p.groupCount = groups;
    p.tile = rank % tileCount;
    p.group = rank / tileCount;
    p.sliceOffset = p.tile;
    p.sliceDivider = tileCount;
    p.samples = samplesPerBatch / (uint32_t)groups + ((uint32_t)p.group < samplesPerBatch % (uint32_t)groups ? 1u : 0u);
    p.seed = (step - 1u) * (uint32_t)groups + (uint32_t)p.group + 1u;
    *out = p;
    return RTOW_SUCCESS;
}

RTOW_API int rtowExchangeAccumDevice(RtowContext ctx, int32_t width, int32_t height, int32_t tileCount, const RtowAccumBuffers* partial, const RtowAccumBuffers* accum,
                                     int32_t what, void* stream)
{
    if (!ctx || !partial || !accum || width <= 0 || height <= 0 || tileCount < 1 || (what & ~(RTOW_GATHER_ALL | RTOW_GATHER_NO_BATCH_WAIT)) || !(what & RTOW_GATHER_ALL))
        return RTOW_ERROR_INVALID_VALUE;
    const bool waitForBatch = !(what & RTOW_GATHER_NO_BATCH_WAIT);
    what &= RTOW_GATHER_ALL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int world = ctx->comm ? ctx->commWorld : 1, rank = ctx->comm ? ctx->commRank : 0;
    if (world % tileCount != 0) return RTOW_ERROR_INVALID_VALUE;                      // G = T x B
    const int groups = world / tileCount, tile = rank % tileCount, own = rank / tileCount;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // the partial sums were written by the last sample batch, whatever stream that was enqueued on (RTOW_GATHER_NO_BATCH_WAIT: the caller ordered it)
    if (waitForBatch && ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);

    // rank p folds the rows with row % G == p; they all lie in the tile p % T, i.e. in what every rank of that tile rendered
    const RowSet set(width, height, world, what);
    const std::array<float*, 4> partBuf = buffersOf(partial), accBuf = buffersOf(accum);
    if (!set.allGiven(partBuf.data()) || !set.allGiven(accBuf.data())) return RTOW_ERROR_INVALID_VALUE;
    for (int b = 0; b < 4; b++) if (set.has(b) && partBuf[b] == accBuf[b]) return RTOW_ERROR_INVALID_VALUE;      // the fold reads partial rows while it writes accum rows
    const size_t regionFloats = set.packedFloats(rank);                                 // what every peer of the tile sends here: this rank's rows of ITS partial

    if (groups > 1) {
        RcclApi* api = rccl();
        if (!api) return RTOW_ERROR_UNSUPPORTED;
        // staging (shared with rtowGatherRowsDevice, ordered by the same event): packed rows for every peer | one region per group for what arrives
        const Regions send = exchangeSendRegions(set, rank, tileCount), recv = exchangeRecvRegions(set, rank, tileCount);
        RTOW_TRY(reserveStaging(ctx, s, send.total, recv.total));
        for (int g = 0; g < groups; g++)
            if (g != own) RTOW_TRY(copyRankRows(ctx, set, partBuf.data(), tile + tileCount * g, ctx->dGatherSend + send.offset[(size_t)g], false, s));
        // a send and a receive per peer of the tile
        RTOW_TRY(postGroup(ctx, api, "exchange of partial sums failed: ncclSend / ncclRecv", [&] {
            int posted = 0;
            for (int g = 0; g < groups && posted == 0; g++) {
                if (g == own) continue;
                const int peer = tile + tileCount * g;
                if (set.packedFloats(peer)) posted = api->Send(ctx->dGatherSend + send.offset[(size_t)g], set.packedFloats(peer), kRcclFloat32, peer, ctx->comm, s);
                if (posted == 0 && regionFloats) posted = api->Recv(ctx->dGatherRecv + recv.offset[(size_t)g], regionFloats, kRcclFloat32, peer, ctx->comm, s);
            }
            return posted;
        }));
    }
    // the fold: this rank's rows, group order, own partial in place
    size_t at = 0;
    for (int b = 0; b < 4; b++)
        if (set.has(b)) {
            HIP_TRY(ctx, launchFoldRows(accBuf[b], partBuf[b], groups > 1 ? ctx->dGatherRecv + at : partBuf[b], regionFloats, (unsigned)(width * kAccumComponents[b]), set.rows(rank), (unsigned)rank,
                                        (unsigned)world, (unsigned)groups, (unsigned)own, s), RTOW_ERROR_LAUNCH_FAILURE);
            at += (size_t)set.rows(rank) * width * kAccumComponents[b];
        }
    return groups > 1 ? gatherEnds(ctx, s) : RTOW_SUCCESS;
}

} // extern "C"
