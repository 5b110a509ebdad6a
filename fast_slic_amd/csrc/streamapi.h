// streamapi.h -- what the entries without an engine share (poolapi.cpp, ragapi.cpp, compareapi.cpp, crfapi.cpp): the caller names the
// device and the stream and owns every buffer.  Internal to the library.
#pragma once
#include "engine_internal.h"
#include "pairtable.h"
#include "pool.h"

namespace fslic {

inline int check_label_type(int label_type) {
    if (label_type != kLabelU16 && label_type != kLabelI32 && label_type != kLabelI64) return fail(FSLIC_E_INVALID, "unknown label type");
    return FSLIC_OK;
}
inline int check_label_map(int N, int H, int W, int label_type) {
    if (H < 1 || W < 1) return fail(FSLIC_E_INVALID, "H and W must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail(FSLIC_E_INVALID, "H * W must be below 2^31");
    if ((long long)N * ((long long)H * W / 1024 + 1) >= (1ll << 31)) return fail(FSLIC_E_INVALID, "too many frames");
    return check_label_type(label_type);
}

// the device, the frames and the capacity of a label pair table (pairtable.h)
inline int check_pair_table(int device, int N, long long capacity) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (capacity < (long long)kPairMinCapacity || capacity > (long long)kPairMaxCapacity || (capacity & (capacity - 1)) != 0)
        return fail(FSLIC_E_INVALID, "capacity must be a power of two in [64, 2^31]");
    if ((long long)N * capacity >= (1ll << 40)) return fail(FSLIC_E_INVALID, "N * capacity must be below 2^40");
    return FSLIC_OK;
}

// the last step of an entry: have its launches been accepted?  `what`: "pool launch", ...
inline int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FSLIC_OK : fail(FSLIC_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Makes `device` current for the scope of a call and restores the calling thread's device afterwards.
struct DeviceScope {
    int prev = -1;
    int enter(int device) {
        int n = 0;
        HIPCHK(hipGetDeviceCount(&n));
        if (device >= n) return fail(FSLIC_E_INVALID, "no such HIP device");
        HIPCHK(hipGetDevice(&prev));
        HIPCHK(hipSetDevice(device));
        (void)hipGetLastError();               // a stale error of an earlier call on this thread is not ours to report
        return FSLIC_OK;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace fslic
