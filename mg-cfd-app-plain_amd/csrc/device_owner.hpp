// device_owner.hpp — who frees what on the device.
//
// DeviceOwner holds device allocations and frees them in its destructor; Event, Stream, GraphExec and IpcMapping are
// std::unique_ptr aliases of the runtime's handle types.  The structs of solver.cpp keep naming device arrays by raw
// pointers (DevicePlan is a kernel argument); an owner sits beside them.  Nothing here is for a launch path: an allocation
// or a free synchronises the device.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace mgcfd {

struct HipError : std::runtime_error {
    explicit HipError(const std::string &m) : std::runtime_error(m) {}
};

#define HIP_CHECK(expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            throw ::mgcfd::HipError(std::string(#expr) + " failed: " + hipGetErrorString(_e));       \
    } while (0)

// what is alive in this process of everything made below (mgcfd_live_device_resources)
struct LiveResources { std::atomic<int64_t> allocations{0}, bytes{0}, handles{0}; };
inline LiveResources g_live;

class DeviceOwner {
    std::vector<std::pair<void *, size_t>> held;        // every allocation made and not released: pointer, bytes
    void *keep(void *p, size_t bytes)
    {
        try { held.emplace_back(p, bytes); } catch (...) { (void)hipFree(p); throw; }
        g_live.allocations++;
        g_live.bytes += static_cast<int64_t>(bytes);
        return p;
    }
    void free_all()
    {
        for (auto &a : held) { (void)hipFree(a.first); g_live.allocations--; g_live.bytes -= static_cast<int64_t>(a.second); }
        held.clear();
    }
public:
    DeviceOwner() = default;
    DeviceOwner(DeviceOwner &&o) noexcept : held(std::move(o.held)) { o.held.clear(); }
    DeviceOwner &operator=(DeviceOwner &&o) noexcept
    {
        if (this != &o) { free_all(); held = std::move(o.held); o.held.clear(); }
        return *this;
    }
    ~DeviceOwner() { free_all(); }

    void *alloc_bytes(size_t bytes)
    {
        void *p = nullptr;
        bytes = bytes ? bytes : 1;
        HIP_CHECK(hipMalloc(&p, bytes));
        return keep(p, bytes);
    }
    // memory another agent writes and this device polls: fine-grained (not cached across those writes) where the runtime
    // grants it, ordinary device memory otherwise
    void *alloc_fine_grained(size_t bytes)
    {
        void *p = nullptr;
        if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) != hipSuccess || !p) { (void)hipGetLastError(); return alloc_bytes(bytes); }
        return keep(p, bytes);
    }
    template <typename T> T *alloc(size_t n) { return static_cast<T *>(alloc_bytes((n ? n : 1) * sizeof(T))); }
    template <typename T> T *upload(const std::vector<T> &v)
    {
        T *p = alloc<T>(v.size());
        if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
    // frees one allocation early, forgets it and nulls the caller's pointer (a null pointer: nothing to do)
    template <typename T> void release(T *&p)
    {
        if (!p) return;
        const void *key = p;
        for (auto it = held.begin(); it != held.end(); ++it) {
            if (it->first != key) continue;
            (void)hipFree(it->first);
            g_live.allocations--;
            g_live.bytes -= static_cast<int64_t>(it->second);
            held.erase(it);
            p = nullptr;
            return;
        }
        throw std::logic_error("DeviceOwner::release: not an allocation of this owner");
    }
    // takes over what another owner holds (arrays built under a local owner, handed over once nothing can throw any more)
    void absorb(DeviceOwner &&o)
    {
        held.insert(held.end(), o.held.begin(), o.held.end());
        o.held.clear();
    }
};

struct EventDeleter { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); g_live.handles--; } };
struct StreamDeleter { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); g_live.handles--; } };
struct GraphExecDeleter { void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); g_live.handles--; } };
struct IpcUnmap { void operator()(void *m) const { (void)hipIpcCloseMemHandle(m); g_live.handles--; } };
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDeleter>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDeleter>;
using GraphExec = std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, GraphExecDeleter>;
using IpcMapping = std::unique_ptr<void, IpcUnmap>;

inline Event make_event(unsigned flags = hipEventDefault)
{
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreateWithFlags(&e, flags));
    g_live.handles++;
    return Event(e);
}
inline Stream make_stream()
{
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    g_live.handles++;
    return Stream(s);
}
// (an instantiation reports through its status; the caller checks it and hands the handle over)
inline GraphExec adopt_graph_exec(hipGraphExec_t g)
{
    if (g) g_live.handles++;
    return GraphExec(g);
}
// the executable of a captured graph; the graph itself goes either way
inline GraphExec instantiate(hipGraph_t graph)
{
    hipGraphExec_t e = nullptr;
    const hipError_t rc = hipGraphInstantiate(&e, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (rc != hipSuccess) throw HipError(std::string("hipGraphInstantiate failed: ") + hipGetErrorString(rc));
    return adopt_graph_exec(e);
}
inline IpcMapping open_ipc_mapping(const hipIpcMemHandle_t &h)
{
    void *m = nullptr;
    HIP_CHECK(hipIpcOpenMemHandle(&m, h, hipIpcMemLazyEnablePeerAccess));
    g_live.handles++;
    return IpcMapping(m);
}

} // namespace mgcfd
