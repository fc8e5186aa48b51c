// devmem.hpp -- who owns device memory. One rule: an allocation belongs either to a DeviceArena (many buffers freed
// together, their bytes summed: a handle's arena is what cwf_hip_system_memory reports) or to a DevicePtr (one buffer,
// freed when its holder goes, counted nowhere). Both round a request up to device_bytes(); nothing else in csrc/ calls
// hipMalloc or hipFree, besides the PEER communicator's mailboxes (peer.hip) and the two diagnostic trace buffers.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace cwf
{

// what an allocation of count T really asks for: never less than one 16-B granule
template <class T> constexpr size_t device_bytes(size_t count) { return std::max<size_t>(count * sizeof(T), 16); }

// Pure bookkeeping (no HIP call): the pointers an arena holds in the order it took them, the size recorded for
// each, and their sum
class DeviceLedger
{
  public:
    void adopt(void *p, size_t bytes)
    {
        entries_.push_back({p, bytes});
        total_ += bytes;
    }
    // the bytes recorded for p; 0 for a pointer the ledger does not hold
    size_t size_of(const void *p) const
    {
        const auto it = find(p);
        return it == entries_.end() ? 0 : it->bytes;
    }
    // forgets p and returns its recorded bytes; 0, and nothing changes, for a pointer the ledger does not hold
    size_t release(const void *p)
    {
        const auto it = find(p);
        const size_t bytes = it == entries_.end() ? 0 : it->bytes;
        if (it != entries_.end())
            entries_.erase(it);
        total_ -= bytes;
        return bytes;
    }
    size_t total() const { return total_; }
    size_t count() const { return entries_.size(); }
    void *at(size_t i) const { return entries_[i].ptr; }

  private:
    struct Entry
    {
        void *ptr;
        size_t bytes;
    };
    std::vector<Entry>::const_iterator find(const void *p) const
    {
        return std::find_if(entries_.begin(), entries_.end(), [p](const Entry &e) { return e.ptr == p; });
    }
    std::vector<Entry> entries_;
    size_t total_ = 0;
};

// The ledger plus hipMalloc / hipFree: every buffer it allocated, until free() or clear() (the destructor's too).
// Moves, never copies (the move constructor is the only one declared).
class DeviceArena
{
  public:
    DeviceArena() = default;
    DeviceArena(DeviceArena &&o) noexcept : ledger_(std::move(o.ledger_)) { o.ledger_ = DeviceLedger(); }
    ~DeviceArena() { clear(); }

    // count T, recorded at device_bytes<T>(count); NULL when the device refuses
    template <class T> T *alloc(size_t count)
    {
        void *q = nullptr;
        if (hipMalloc(&q, device_bytes<T>(count)) != hipSuccess)
            return nullptr;
        ledger_.adopt(q, device_bytes<T>(count));
        return static_cast<T *>(q);
    }
    // frees one of the arena's buffers (anything else, NULL included, is left alone)
    void free(void *p)
    {
        if (p && ledger_.release(p))
            (void)hipFree(p);
    }
    void clear()
    {
        for (size_t i = 0; i < ledger_.count(); ++i)
            (void)hipFree(ledger_.at(i));
        ledger_ = DeviceLedger();
    }
    size_t size_of(const void *p) const { return ledger_.size_of(p); }
    size_t total() const { return ledger_.total(); }

  private:
    DeviceLedger ledger_;
};

// One uncounted device buffer, freed when the holder leaves its scope or takes another buffer. Reads as a T *.
// Moves, never copies.
template <class T> class DevicePtr
{
  public:
    DevicePtr() = default;
    DevicePtr(DevicePtr &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevicePtr &operator=(DevicePtr &&o) noexcept
    {
        std::swap(p_, o.p_);  // o, a temporary or a scope's local, frees what this held
        return *this;
    }
    ~DevicePtr() { reset(); }

    // drops what it held, then holds count T (hipMalloc's error otherwise, holding nothing)
    hipError_t alloc(size_t count)
    {
        reset();
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, device_bytes<T>(count));
        p_ = e == hipSuccess ? static_cast<T *>(q) : nullptr;
        return e;
    }
    void reset()
    {
        if (p_)
            (void)hipFree(p_);
        p_ = nullptr;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }

  private:
    T *p_ = nullptr;
};

}  // namespace cwf
