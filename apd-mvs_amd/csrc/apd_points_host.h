// apd_points_host.h -- what the host side of the calls on a points object shares (apd_points.hip, apd_points_merge.hip): the
// device of one call, and the device memory of one call.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace apd_points_host {

// Selects a device for one call and puts the caller's back
struct DeviceScope {
    int previous = -1;
    explicit DeviceScope(bool active)
    {
        if (active && hipGetDevice(&previous) != hipSuccess) {
            previous = -1;
        }
    }
    ~DeviceScope()
    {
        if (previous >= 0) {
            hipSetDevice(previous);
        }
    }
};

// Device memory of one call: freed when the call returns, but for what it hands over
struct Scratch {
    std::vector<void *> owned;
    ~Scratch()
    {
        for (void *q : owned) {
            hipFree(q);
        }
    }
    template <typename T> hipError_t alloc(size_t bytes, T **out)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes > 0 ? bytes : 1);
        if (e == hipSuccess) {
            owned.push_back(q);
            *out = static_cast<T *>(q);
        }
        return e;
    }
    // a device copy of `bytes` host bytes
    template <typename T> hipError_t upload(const T *host, size_t bytes, const T **out)
    {
        T *copy = nullptr;
        hipError_t e = alloc(bytes, &copy);
        if (e == hipSuccess) {
            *out = copy;
            e = bytes > 0 ? hipMemcpy(copy, host, bytes, hipMemcpyHostToDevice) : hipSuccess;
        }
        return e;
    }
    void keep(void *q) { owned.erase(std::find(owned.begin(), owned.end(), q)); }
};

}  // namespace apd_points_host
