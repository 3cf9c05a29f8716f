// hip_handles.hpp -- move-only owners of the front end's HIP resources, on the C ABI of include/vkmr_hip.h.
//
// Every device buffer, pinned buffer, event and stream the host layer creates is owned by exactly one of these, and the
// pools (Batches, SlicePool, the spare events and reduction sets) hold handles: what is not given back to a pool is
// released where it goes out of scope, on the error paths too.  A release may replace the text of
// vkmr_hip_last_error(): report a failed call before the handles around it are destroyed, reset or assigned to.
#pragma once
#include <cstddef>

#include "vkmr_hip.h"

namespace vkmr {

// Status of the last failed ABI call, in the role VkResult has in the reference.
typedef vkmr_status HipResult;

namespace detail {
inline vkmr_status host_free(int, void* p) { return vkmr_hip_host_free(p); }

template <class Raw, vkmr_status (*Release)(int, Raw)>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : m_dev(o.m_dev), m_raw(o.m_raw) { o.m_raw = nullptr; }
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) {
            reset();
            m_dev = o.m_dev;
            m_raw = o.m_raw;
            o.m_raw = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }

    explicit operator bool() const { return m_raw != nullptr; }
    int device() const { return m_dev; }
    Raw get() const { return m_raw; }
    void reset()
    {
        if (m_raw) Release(m_dev, m_raw);
        m_raw = nullptr;
    }

protected:
    // make(&raw) is the alloc / create call: what it produced is taken over when it succeeded, its status returned unchanged.
    template <class Make> HipResult Acquire(int dev, Make make)
    {
        Raw raw = nullptr;
        const HipResult st = make(&raw);
        if (st == VKMR_OK) *this = Owned(dev, raw);
        return st;
    }

private:
    Owned(int dev, Raw raw) : m_dev(dev), m_raw(raw) {}
    int m_dev = -1;
    Raw m_raw = nullptr;
};

template <vkmr_status (*Release)(int, void*)>
struct Memory : Owned<void*, Release> {
    template <class T> T* as() const { return static_cast<T*>(this->get()); }
};
}  // namespace detail

struct DeviceMem : detail::Memory<vkmr_hip_device_free> {
    static HipResult Alloc(int dev, size_t bytes, DeviceMem* out) { return out->Acquire(dev, [&](void** p) { return vkmr_hip_device_alloc(dev, bytes, p); }); }
};
struct PinnedMem : detail::Memory<detail::host_free> {
    static HipResult Alloc(size_t bytes, PinnedMem* out) { return out->Acquire(-1, [&](void** p) { return vkmr_hip_host_alloc(bytes, p); }); }
};
struct EventHandle : detail::Owned<vkmr_event, vkmr_hip_event_destroy> {
    static HipResult Create(int dev, EventHandle* out) { return out->Acquire(dev, [&](vkmr_event* e) { return vkmr_hip_event_create(dev, e); }); }
};
struct StreamHandle : detail::Owned<vkmr_stream, vkmr_hip_stream_destroy> {
    static HipResult Create(int dev, StreamHandle* out) { return out->Acquire(dev, [&](vkmr_stream* s) { return vkmr_hip_stream_create(dev, s); }); }
};

}  // namespace vkmr
