// labels.h -- the element types of a label map given by pointer, and a label as an index (pool.hip, rag.hip, compare.hip, connect.hip,
// merge.hip; region.hip names the type of its counts with it).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fslic {

enum LabelType { kLabelU16 = 0, kLabelI32 = 1, kLabelI64 = 2 };

// (kernels) a label as an index: K when it is not in [0, K) (the int16 map's -1 is 0xFFFF >= K, K <= 65534)
static __device__ __forceinline__ uint32_t canon(uint16_t v, uint32_t K) { return (uint32_t)v < K ? (uint32_t)v : K; }
static __device__ __forceinline__ uint32_t canon(int32_t v, uint32_t K) { return (uint32_t)v < K ? (uint32_t)v : K; }
static __device__ __forceinline__ uint32_t canon(int64_t v, uint32_t K) { return (unsigned long long)v < (unsigned long long)K ? (uint32_t)v : K; }

// (launches) calls f(const L* map) with the map as its label type L; compare.hip nests two of them for its two maps
template <class F>
static inline void with_label_type(const void* map, int label_type, F f) {
    if (label_type == kLabelU16) f(reinterpret_cast<const uint16_t*>(map));
    else if (label_type == kLabelI32) f(reinterpret_cast<const int32_t*>(map));
    else f(reinterpret_cast<const int64_t*>(map));
}

}  // namespace fslic
