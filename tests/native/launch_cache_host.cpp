// Stand-alone host program (tests/test_launch_cache.py builds it with -fsanitize=address,undefined): csrc/rtow_launch_cache.h without a device.  A fresh Keyed holds
// nothing - not the key of all zeros either -, holds exactly the key it was given, stops holding it when any single member of the launch changes alone (the scene serial,
// each of the view's 22 floats - +0 against -0 too -, the frame and slice, each Size word for 64 against 64.9 and against the float just below 65, jitter, pruning, groups
// per pixel, mapped), and is empty after drop; decodeSchedulerKnob over every word from -1 to 65 536 against the unpacking written out again.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../raytracing-in-one-weekend_amd/csrc/rtow_launch_cache.h"

using namespace rtow;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// the fields of SampleKernelArgs the builders read
struct Launch {
    RtowView view;
    int32_t width, height, sliceOffset, sliceDivider;
    float sizeX, sizeY;
    int32_t subPixelJitter;
    uint32_t groupsPerPixel;
};

static Launch baseLaunch()
{
    Launch a{};
    float v[22];
    for (int i = 0; i < 22; i++) v[i] = 0.25f * (float)(i + 1);
    memcpy(&a.view, v, sizeof v);
    a.width = 64; a.height = 36; a.sliceOffset = 1; a.sliceDivider = 2;
    a.sizeX = 64.0f; a.sizeY = 36.0f;
    a.subPixelJitter = 1;
    a.groupsPerPixel = 3;
    return a;
}

static Launch withViewFloat(Launch a, int i, float value)
{
    float v[22];
    memcpy(v, &a.view, sizeof v);
    v[i] = value;
    memcpy(&a.view, v, sizeof v);
    return a;
}

// one Keyed through its life: nothing held, the key held, `other` (one member changed) not held and the other way round, empty again after drop
template <typename Key> static bool heldApart(const Key& key, const Key& other)
{
    Keyed<Key> k;
    if (k.holds(key) || k.holds(other) || k.get()) return false;
    k.set(key);
    if (!k.holds(key) || k.holds(other) || !k.get() || !(*k.get() == key)) return false;
    k.set(other);
    if (!k.holds(other) || k.holds(key)) return false;
    k.drop();
    return !k.holds(key) && !k.holds(other) && !k.get();
}

static int keyedHoldsNothingAtFirst()
{
    Keyed<CameraListKey> lists;
    Keyed<ChunkOrderKey> order;
    const CameraListKey zeroLists{};
    const ChunkOrderKey zeroOrder{};
    CHECK(!lists.get() && !lists.holds(zeroLists));
    CHECK(!order.get() && !order.holds(zeroOrder));
    const Launch zero{};
    CHECK(cameraListKey(0, zero, false) == zeroLists && chunkOrderKey(0, zero, false) == zeroOrder);     // what a fresh context's first launch could ask for, field by field
    CHECK(!lists.holds(cameraListKey(0, zero, false)) && !order.holds(chunkOrderKey(0, zero, false)));
    lists.set(zeroLists); order.set(zeroOrder);
    CHECK(lists.holds(zeroLists) && lists.get() && order.holds(zeroOrder) && order.get());
    lists.drop(); order.drop();
    CHECK(!lists.get() && !lists.holds(zeroLists) && !order.get() && !order.holds(zeroOrder));
    return 0;
}

static int cameraListKeys()
{
    const Launch a = baseLaunch();
    const CameraListKey key = cameraListKey(7, a, true);
    CHECK(key == cameraListKey(7, a, true));
    CHECK(key.frame.width == 64 && key.frame.height == 36 && key.frame.sliceOffset == 1 && key.frame.sliceDivider == 2 && key.pruned && key.jitter && key.sceneSerial == 7);
    CHECK(heldApart(key, cameraListKey(8, a, true)));
    CHECK(heldApart(key, cameraListKey(7, a, false)));
    for (int i = 0; i < 22; i++) {
        CHECK(heldApart(key, cameraListKey(7, withViewFloat(a, i, 100.0f), true)));
        CHECK(heldApart(cameraListKey(7, withViewFloat(a, i, 0.0f), true), cameraListKey(7, withViewFloat(a, i, -0.0f), true)));
    }
    Launch b;
    b = a; b.width = 65; CHECK(heldApart(key, cameraListKey(7, b, true)));
    b = a; b.height = 37; CHECK(heldApart(key, cameraListKey(7, b, true)));
    b = a; b.sliceOffset = 0; CHECK(heldApart(key, cameraListKey(7, b, true)));
    b = a; b.sliceDivider = 3; CHECK(heldApart(key, cameraListKey(7, b, true)));
    // the fraction of Size: (int) of all three is 64
    const float justBelow65 = nextafterf(65.0f, 0.0f);
    CHECK((int)64.9f == 64 && (int)justBelow65 == 64 && justBelow65 < 65.0f);
    for (const float s : {64.9f, justBelow65}) {
        b = a; b.sizeX = s; CHECK(heldApart(key, cameraListKey(7, b, true)));
        b = a; b.sizeY = s; CHECK(heldApart(key, cameraListKey(7, b, true)));
    }
    b = a; b.sizeX = 36.0f; b.sizeY = 64.0f; CHECK(heldApart(key, cameraListKey(7, b, true)));      // the two words are not interchangeable
    b = a; b.subPixelJitter = 0; CHECK(heldApart(key, cameraListKey(7, b, true)));
    b = a; b.subPixelJitter = 2; CHECK(key == cameraListKey(7, b, true));                             // the kernel reads it as a truth value
    b = a; b.groupsPerPixel = 4; CHECK(key == cameraListKey(7, b, true));                             // the lists are per pixel whatever the work units are
    return 0;
}

static int chunkOrderKeys()
{
    const Launch a = baseLaunch();
    const ChunkOrderKey key = chunkOrderKey(7, a, true);
    CHECK(key == chunkOrderKey(7, a, true));
    CHECK(heldApart(key, chunkOrderKey(8, a, true)));
    CHECK(heldApart(key, chunkOrderKey(7, a, false)));
    Launch b;
    b = a; b.width = 65; CHECK(heldApart(key, chunkOrderKey(7, b, true)));
    b = a; b.height = 37; CHECK(heldApart(key, chunkOrderKey(7, b, true)));
    b = a; b.sliceOffset = 0; CHECK(heldApart(key, chunkOrderKey(7, b, true)));
    b = a; b.sliceDivider = 3; CHECK(heldApart(key, chunkOrderKey(7, b, true)));
    b = a; b.groupsPerPixel = 4; CHECK(heldApart(key, chunkOrderKey(7, b, true)));
    b = withViewFloat(a, 0, 100.0f); b.sizeX = 64.9f; b.subPixelJitter = 0; CHECK(key == chunkOrderKey(7, b, true));      // the order does not depend on the view
    return 0;
}

static int schedulerKnob()
{
    int refused = 0;
    for (int given = -1; given <= 65536; given++) {
        // the unpacking written out again: <= 0 is the default word 3; a zero low nibble takes the default side
        int word = given > 0 ? given : 3;
        if ((word & 15) == 0) word |= 3;
        const int side = word & 15;
        const bool good = (side == 1 || side == 2 || side == 3 || side == 4 || side == 8) && word < 65536;
        SchedulerKnob k;
        memset(&k, 0x5a, sizeof k);
        SchedulerKnob untouched;
        memcpy(&untouched, &k, sizeof k);
        CHECK(decodeSchedulerKnob(given, &k) == good);
        if (!good) { refused++; CHECK(memcmp(&k, &untouched, sizeof k) == 0); continue; }
        CHECK(k.word == word);
        CHECK(k.ticketMapSide == (side == 1 ? 0u : side == 3 ? 1u : (unsigned)side));
        CHECK(k.regroupMode == (unsigned)((word / 16) % 4));
        CHECK(k.orderByTotal == ((word / 64) % 2 == 1));
        CHECK(k.slotBlockOverride == (unsigned)((word / 256) % 16));
        CHECK(k.pixelGateOverride == (word / 4096) % 16);
    }
    // 10 of the 16 low nibbles are refused in each of the 4 096 blocks of sixteen words below 65 536 (the nibble of 65 536 itself is 0: refused for its size)
    CHECK(refused == 4096 * 10 + 1);
    SchedulerKnob d, z;
    CHECK(decodeSchedulerKnob(0, &d) && decodeSchedulerKnob(-1, &z) && d.word == RTOW_DEFAULT_REGROUP_SIDE && z.word == d.word && d.ticketMapSide == 1u);
    return 0;
}

int main()
{
    if (keyedHoldsNothingAtFirst() || cameraListKeys() || chunkOrderKeys() || schedulerKnob()) return 1;
    printf("ok\n");
    return 0;
}
