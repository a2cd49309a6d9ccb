// rtow_device_mem.h - who owns the library's device memory: one hipMalloc block per object, freed by its destructor.  Needs the HIP runtime API alone.
// A block is grow-only.  ensure(bytes) does nothing while bytes <= bytes(); otherwise it frees the old block FIRST and then allocates the new one at exactly `bytes`:
// the contents are not kept, and the old and the new block never exist side by side.  A failed allocation leaves the object empty (null, 0 bytes), so the next call
// allocates again.  `grew` (optional) is set exactly when the old pointer is gone - after a failure too: callers do around the call what the old block needs first
// (a batch in flight may still read it) and drop what described its contents when `grew` says so.  release() frees now.  The size is kept in bytes; a caller that
// needs a capacity in its own unit derives it from bytes().
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <initializer_list>

namespace rtow {

class DeviceBlock {
public:
    struct Need { DeviceBlock* block; size_t bytes; };
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
    ~DeviceBlock() { release(); }
    size_t bytes() const { return bytes_; }
    hipError_t ensure(size_t bytes, bool* grew = nullptr) { return ensureAll({{this, bytes}}, grew); }
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; bytes_ = 0; }
    // Blocks that grow together, each to its own size: every block that is too small is freed before the first new one is requested (the most memory held at a time
    // is the new sizes, never old + new), then they are allocated in order.  A failure stops there: the blocks after it stay empty, the ones before it are valid.
    static hipError_t ensureAll(std::initializer_list<Need> needs, bool* grew = nullptr)
    {
        if (grew) *grew = false;
        for (const Need& n : needs)
            if (n.bytes > n.block->bytes_) { n.block->release(); if (grew) *grew = true; }
        for (const Need& n : needs)
            if (n.bytes > n.block->bytes_) {
                const hipError_t e = hipMalloc(&n.block->p_, n.bytes);
                if (e != hipSuccess) { n.block->p_ = nullptr; return e; }
                n.block->bytes_ = n.bytes;
            }
        return hipSuccess;
    }
protected:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// The block as a T*: use sites read `ctx->dScene + offset`, `if (!ctx->dTieRedo)`, `a.pixelCost = co.dPixelCost` as they would a raw pointer
template <typename T> class DeviceMem : public DeviceBlock {
public:
    operator T*() const { return static_cast<T*>(p_); }
    T* get() const { return static_cast<T*>(p_); }
};

// One pinned host block (hipHostMalloc), allocated once
class PinnedBlock {
public:
    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock&) = delete;
    PinnedBlock& operator=(const PinnedBlock&) = delete;
    ~PinnedBlock() { if (p_) (void)hipHostFree(p_); }
    hipError_t allocate(size_t bytes, unsigned flags) { const hipError_t e = p_ ? hipErrorInvalidValue : hipHostMalloc(&p_, bytes, flags); if (e != hipSuccess) p_ = nullptr; return e; }
    void* get() const { return p_; }
private:
    void* p_ = nullptr;
};

} // namespace rtow
