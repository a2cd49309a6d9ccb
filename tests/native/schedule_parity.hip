// Test-only library: the product's scheduling launchers (launchBuildChunkOrder, launchInitTicketMap, launchRegroupTickets of
// raytracing-in-one-weekend_amd/csrc/rtow_schedule.hip.h) run on the device over caller-supplied costs and maps, and what they leave is copied back.  The LAUNCHERS
// are called, not the kernels: they choose between the one-workgroup and the several-workgroup order, the grids and the dynamic LDS size.
// tests/test_gpu_schedule.py compares the results with tests/schedule_reference.py word for word.
//
// Every function returns the HIP error of the first step that failed (0 = hipSuccess).  Two results are not HIP errors: -2 = a launcher wrote outside the words it
// was given (every device array here has kGuardWords untouched words behind it), -3 = a ticket map came back holding a pixel number it did not start with.
#include "../../raytracing-in-one-weekend_amd/csrc/rtow_schedule.hip.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace {

constexpr size_t kGuardWords = 64;
constexpr unsigned kGuardWord = 0xa5a5a5a5u;

#define SCHED_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

// device array of `count` elements of T followed by the guard words, all bytes 0xa5 to begin with
template <typename T> struct Guarded {
    T* p = nullptr;
    size_t count = 0;
    ~Guarded() { (void)hipFree(p); }
    size_t bytes() const { return (count * sizeof(T) + 3u) / 4u * 4u; }              // the guard starts at a word
    hipError_t alloc(size_t n)
    {
        count = n;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes() + kGuardWords * 4u);
        if (e == hipSuccess) e = hipMemset(p, 0xa5, bytes() + kGuardWords * 4u);
        return e;
    }
    hipError_t guardIntact(bool* intact) const
    {
        unsigned g[kGuardWords];
        const hipError_t e = hipMemcpy(g, reinterpret_cast<const char*>(p) + bytes(), sizeof(g), hipMemcpyDeviceToHost);
        *intact = true;
        for (unsigned w : g) if (w != kGuardWord) *intact = false;
        return e;
    }
};

} // namespace

#define SCHED_EXPORT extern "C" __attribute__((visibility("default")))

// pixelCost: 64 * n ray counts in ticket order.  costOut: 2 * n words (sums, then maxima), orderOut: n words.  The cost array has kChunkOrderScratchWords behind
// its two columns, as the context allocates it; the order starts as 0xa5a5a5a5 everywhere, so a position nobody wrote shows.
SCHED_EXPORT int schedule_chunk_order(const unsigned short* pixelCost, unsigned n, int byMax, unsigned* costOut, unsigned* orderOut)
{
    Guarded<unsigned short> dPixelCost;
    Guarded<unsigned> dCost, dOrder;
    SCHED_TRY(dPixelCost.alloc((size_t)n * 64u));
    SCHED_TRY(dCost.alloc(2u * (size_t)n + rtow::kChunkOrderScratchWords));
    SCHED_TRY(dOrder.alloc(n));
    SCHED_TRY(hipMemcpy(dPixelCost.p, pixelCost, (size_t)n * 64u * sizeof(unsigned short), hipMemcpyHostToDevice));
    SCHED_TRY(rtow::launchBuildChunkOrder(dPixelCost.p, dCost.p, n, dOrder.p, byMax, nullptr));
    SCHED_TRY(hipDeviceSynchronize());
    SCHED_TRY(hipMemcpy(costOut, dCost.p, 2u * (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    SCHED_TRY(hipMemcpy(orderOut, dOrder.p, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    bool a = true, b = true, c = true;
    SCHED_TRY(dPixelCost.guardIntact(&a));
    SCHED_TRY(dCost.guardIntact(&b));
    SCHED_TRY(dOrder.guardIntact(&c));
    return a && b && c ? 0 : -2;
}

// `rounds` regroupings in a row over tickets = 64 * tilesPerRow * tileRows tickets.  pixelCost / ticketMap: the state before round 0, in ticket order.  Before round
// r >= 1 the costs are written afresh IN TICKET ORDER under the map as it then is, the way a sample launch leaves them: pixelCost[t] = nextCosts[(r - 1) * tickets + s],
// s = the ticket the pixel ticketMap[t] held at the start (the pixel numbers of the starting map must be distinct).  costOut / mapOut: rounds x tickets, the state behind
// every round.  A launcher error ends the call behind that round's copy (which then shows the state the refused call left); later rounds stay as the caller passed them.
SCHED_EXPORT int schedule_regroup(const unsigned short* pixelCost, const unsigned* ticketMap, unsigned tilesPerRow, unsigned tileRows, unsigned side, const unsigned* classes,
                                  unsigned rounds, const unsigned short* nextCosts, unsigned short* costOut, unsigned* mapOut)
{
    const size_t tickets = (size_t)tilesPerRow * tileRows * 64u;
    Guarded<unsigned short> dCost;
    Guarded<unsigned> dMap;
    SCHED_TRY(dCost.alloc(tickets));
    SCHED_TRY(dMap.alloc(tickets));
    SCHED_TRY(hipMemcpy(dCost.p, pixelCost, tickets * sizeof(unsigned short), hipMemcpyHostToDevice));
    SCHED_TRY(hipMemcpy(dMap.p, ticketMap, tickets * sizeof(unsigned), hipMemcpyHostToDevice));
    std::vector<std::pair<unsigned, unsigned>> start(tickets);                      // (pixel, the ticket it started at), by pixel
    for (size_t t = 0; t < tickets; t++) start[t] = {ticketMap[t], (unsigned)t};
    std::sort(start.begin(), start.end());
    std::vector<unsigned short> fresh(tickets);
    for (unsigned r = 0; r < rounds; r++) {
        if (r > 0) {
            const unsigned* map = mapOut + (size_t)(r - 1) * tickets;
            for (size_t t = 0; t < tickets; t++) {
                const auto it = std::lower_bound(start.begin(), start.end(), std::make_pair(map[t], 0u));
                if (it == start.end() || it->first != map[t]) return -3;
                fresh[t] = nextCosts[(size_t)(r - 1) * tickets + it->second];
            }
            SCHED_TRY(hipMemcpy(dCost.p, fresh.data(), tickets * sizeof(unsigned short), hipMemcpyHostToDevice));
        }
        const hipError_t launched = rtow::launchRegroupTickets(dCost.p, dMap.p, tilesPerRow, tileRows, side, classes, nullptr);
        SCHED_TRY(hipDeviceSynchronize());
        SCHED_TRY(hipMemcpy(costOut + (size_t)r * tickets, dCost.p, tickets * sizeof(unsigned short), hipMemcpyDeviceToHost));
        SCHED_TRY(hipMemcpy(mapOut + (size_t)r * tickets, dMap.p, tickets * sizeof(unsigned), hipMemcpyDeviceToHost));
        bool a = true, b = true;
        SCHED_TRY(dCost.guardIntact(&a));
        SCHED_TRY(dMap.guardIntact(&b));
        if (!(a && b)) return -2;
        if (launched != hipSuccess) return (int)launched;                           // (the state copied back shows whether the refused call touched anything)
    }
    return 0;
}

// mapOut: n words, the map launchInitTicketMap leaves
SCHED_EXPORT int schedule_init_map(unsigned n, unsigned* mapOut)
{
    Guarded<unsigned> dMap;
    SCHED_TRY(dMap.alloc(n));
    SCHED_TRY(rtow::launchInitTicketMap(dMap.p, n, nullptr));
    SCHED_TRY(hipDeviceSynchronize());
    SCHED_TRY(hipMemcpy(mapOut, dMap.p, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    bool a = true;
    SCHED_TRY(dMap.guardIntact(&a));
    return a ? 0 : -2;
}
