// streamapi.h -- what the stream entries share: the fslic_hip_* functions that take (device, stream, ...) and their *_workspace_size
// companions (poolapi.cpp, ragapi.cpp, compareapi.cpp, crfapi.cpp, softapi.cpp, connectapi.cpp, mergeapi.cpp, regionapi.cpp,
// ingestapi.cpp, aggregateapi.cpp, attendapi.cpp, knnapi.cpp, messageapi.cpp, pixelapi.cpp).  No engine: the caller names the device and the stream and owns every buffer.  Every
// argument is checked before the first HIP call.  An entry is its checks, in the order it refuses in (tests/test_stream_refusals_cpu.py pins the
// order and the words), and then on_stream() around what it enqueues.  Internal to the library.
#pragma once
#include "engine_internal.h"
#include "labels.h"
#include "pairtable.h"

namespace fslic {

// ---- the checks that more than one file states ----
inline int check_device(int device) { return device < 0 ? fail(FSLIC_E_INVALID, "device must be >= 0") : FSLIC_OK; }
// nodes of a frame, groups, labels: what = "K", "K2", "M"
inline int check_node_count(int K, const char* what) {
    return K < 1 || K > 65534 ? fail(FSLIC_E_INVALID, std::string(what) + " must be in [1, 65534]") : FSLIC_OK;
}
// edges of a graph, entries of neighbour lists: what = "E", "nnz"
inline int check_entry_count(long long v, const char* what) {
    return v < 0 || v >= (1ll << 31) ? fail(FSLIC_E_INVALID, std::string(what) + " must be in [0, 2^31)") : FSLIC_OK;
}
// the frames, the channels and the nodes (or groups) of a [N][C][K] array: what = "K" or "K2"
inline int check_cells(int N, int C, int K, const char* what) {
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (C < 1) return fail(FSLIC_E_INVALID, "C must be positive");
    const int rc = check_node_count(K, what);
    if (rc) return rc;
    if ((long long)N * K >= (1ll << 31) || (long long)N * K * C >= (1ll << 31))
        return fail(FSLIC_E_INVALID, std::string("N * C * ") + what + " must be below 2^31");
    return FSLIC_OK;
}
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
    const int rc = check_device(device);
    if (rc) return rc;
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (capacity < (long long)kPairMinCapacity || capacity > (long long)kPairMaxCapacity || (capacity & (capacity - 1)) != 0)
        return fail(FSLIC_E_INVALID, "capacity must be a power of two in [64, 2^31]");
    if ((long long)N * capacity >= (1ll << 40)) return fail(FSLIC_E_INVALID, "N * capacity must be below 2^40");
    return FSLIC_OK;
}
// `need`: what the entry's *_workspace_size answers
inline int check_workspace(size_t bytes, size_t need) {
    return bytes < need ? fail(FSLIC_E_INVALID, "workspace too small: " + std::to_string(need) + " bytes needed") : FSLIC_OK;
}

// A *_workspace_size entry: `bytes` is looked at first, then check() has the sizes checked, and need() is the bytes for sizes that
// passed (it is not called for others: a size function need not be defined there).
template <class Check, class Need>
int workspace_size(size_t* bytes, Check check, Need need) {
    if (!bytes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const int rc = check();
    if (rc) return rc;
    *bytes = need();
    return FSLIC_OK;
}

// int64 arrays of the ABI as the kernels' long long
inline const long long* i64(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
inline unsigned long long* u64(int64_t* p) { return reinterpret_cast<unsigned long long*>(p); }

// ---- the tail of an entry ----
// have its launches been accepted?  `what`: "pool launch", ...
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

// What an entry does once its arguments have passed: with `device` current, body(stream) enqueues (an int status: HIPCHK works in it),
// and the entry's answer is whether the launches were accepted.
template <class Body>
int on_stream(int device, void* stream, const char* what, Body body) {
    DeviceScope scope;
    int rc = scope.enter(device);
    if (rc || (rc = body(reinterpret_cast<hipStream_t>(stream)))) return rc;
    return launched(what);
}

}  // namespace fslic
