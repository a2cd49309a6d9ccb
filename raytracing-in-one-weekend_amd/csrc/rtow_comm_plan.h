// rtow_comm_plan.h - which rows a rank owns and where every peer's packed rows lie in the two staging blocks of the multi-GPU row transport (rtow_comm.hip).
// Pure arithmetic with no HIP in it, so that the CPU suite can hold it to its contract (tests/test_comm_plan.py through tests/native/comm_plan_shim.cpp).
#pragma once
#include <stddef.h>

#include <vector>

namespace rtow {

// rows of the frame owned by `rank` under the reference's interlacing (row % divider == rank, JOBS/SampleBatchJob.cs:69-70)
inline unsigned rowsOwnedBy(int rank, int divider, int height) { return rank >= height ? 0u : (unsigned)((height - rank + divider - 1) / divider); }

constexpr int kAccumComponents[4] = {4, 3, 3, 1};      // floats per pixel of colour | normal | albedo | sample-count weight (RtowAccumBuffers, the bits of RTOW_GATHER_ALL)

// The accumulators a call moves (`what`: bits of RTOW_GATHER_ALL) of a width x height frame whose rows are dealt out to `world` ranks.  The rows of one rank travel as
// one packed region: all its rows of the first selected buffer, then all of the second, ... - buffer b begins rows * width * (components of the selected b' < b) floats in.
struct RowSet {
    int width, height, world, what;
    unsigned floatsPerPixel = 0;
    RowSet(int width, int height, int world, int what) : width(width), height(height), world(world), what(what) { for (int b = 0; b < 4; b++) if (has(b)) floatsPerPixel += (unsigned)kAccumComponents[b]; }
    bool has(int b) const { return (what & (1 << b)) != 0; }
    bool allGiven(float* const buffers[4]) const { for (int b = 0; b < 4; b++) if (has(b) && !buffers[b]) return false; return true; }
    unsigned rows(int rank) const { return rowsOwnedBy(rank, world, height); }
    size_t packedFloats(int rank) const { return (size_t)rows(rank) * (size_t)width * floatsPerPixel; }
};

// Regions of one staging block, in floats: where region k begins, and the end of the last one.  Region k holds the rows of rank first + stride * k, `count` of them
// end to end; the region of `skip` takes no room (nothing travels from a rank to itself).
struct Regions { std::vector<size_t> offset; size_t total = 0; };
inline Regions layOut(const RowSet& set, int count, int first, int stride, int skip)
{
    Regions g;
    for (int k = 0; k < count; k++) { g.offset.push_back(g.total); if (k != skip) g.total += set.packedFloats(first + stride * k); }
    return g;
}
// rtowGatherRowsDevice, the root's receive block: the rows of every other rank, in rank order
inline Regions gatherRegions(const RowSet& set, int root) { return layOut(set, set.world, 0, 1, root); }
// rtowExchangeAccumDevice of `rank` among world = tileCount x groups ranks; its peers are the ranks tile + tileCount * g of its own tile, one per group g.
// Send block: what each peer owns of this rank's partial sum, in group order.  Receive block: this rank's own rows once per group - the region of its own group
// stays unused (fold_rows_kernel reads that partial sum in place), so that region g begins at g x the region size.
inline Regions exchangeSendRegions(const RowSet& set, int rank, int tileCount) { return layOut(set, set.world / tileCount, rank % tileCount, tileCount, rank / tileCount); }
inline Regions exchangeRecvRegions(const RowSet& set, int rank, int tileCount) { return layOut(set, set.world / tileCount, rank, 0, -1); }

} // namespace rtow
