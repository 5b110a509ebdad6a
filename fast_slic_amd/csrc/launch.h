// launch.h -- one launch call for the stream and for the graph of a group
// A slot replays its group (about 30 kernels at 10 iterations) from a hipGraph.  The graph is BUILT node by node from the very
// launch calls that enqueue a group directly: while a GraphRecorder is current on the calling thread, fslic::launch() adds a
// kernel node (chained behind the previous one: program order, like the stream) instead of launching.  No stream capture:
// for as long as any stream of the process captures, hipDeviceSynchronize and other calls of OTHER threads (a framework
// synchronising, allocating) fail with "operation not permitted when stream is capturing", whatever the capture mode.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cassert>
#include <tuple>
#include <type_traits>
#include <utility>

namespace fslic {

struct GraphRecorder {
    hipGraph_t graph = nullptr;
    hipGraphNode_t last = nullptr;     // the chain's tail
    hipError_t err = hipSuccess;       // first failure; the group is then enqueued directly and the graph dropped
    int nodes = 0;
    void chain(hipGraphNode_t n) { last = n; nodes++; }
};
// The recorder of the calling thread (nullptr: launches go to the stream).  Defined in group.cpp.
GraphRecorder*& current_recorder();

template <typename Tuple, size_t... I>
static inline void add_kernel_node(GraphRecorder& r, void* func, dim3 grid, dim3 block, unsigned shmem, Tuple& a, std::index_sequence<I...>) {
    void* ptrs[sizeof...(I) + 1] = {(void*)&std::get<I>(a)..., nullptr};     // the values are copied into the node here
    hipKernelNodeParams p{};
    p.func = func; p.gridDim = grid; p.blockDim = block; p.sharedMemBytes = shmem; p.kernelParams = ptrs; p.extra = nullptr;
    hipGraphNode_t node = nullptr;
    const hipError_t e = hipGraphAddKernelNode(&node, r.graph, r.last ? &r.last : nullptr, r.last ? 1 : 0, &p);
    if (e != hipSuccess) { if (r.err == hipSuccess) r.err = e; return; }
    r.chain(node);
}

template <typename... KArgs, typename... Args>
static inline void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, unsigned shmem, hipStream_t st, Args&&... args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count of the kernel");
    GraphRecorder* r = current_recorder();
    if (!r) {
        hipLaunchKernelGGL(kernel, grid, block, shmem, st, static_cast<KArgs>(args)...);
        return;
    }
    if (r->err != hipSuccess) return;
    std::tuple<std::remove_cv_t<std::remove_reference_t<KArgs>>...> a(static_cast<KArgs>(args)...);
    add_kernel_node(*r, reinterpret_cast<void*>(kernel), grid, block, shmem, a, std::index_sequence_for<KArgs...>{});
}

// One 256-thread block per item for item counts the runtime cannot launch at once (soft.h has the rule and why; ingest.h follows it): the
// launch goes out in slices of at most kMaxLaunchBlocks blocks, in order on the stream, each with the flat index of its first block as the
// kernel's last argument.  Below that count there is one launch.
constexpr unsigned long long kMaxLaunchBlocks = (1ull << 24) - 1ull;     // 2^32 - 256 threads: the largest launch the runtime supports
template <typename... KArgs, typename... Args>
static inline void launch_sliced(void (*kernel)(KArgs...), unsigned long long blocks, hipStream_t st, Args... args) {
    for (unsigned long long first = 0; first < blocks; first += kMaxLaunchBlocks) {
        const unsigned long long nb = blocks - first < kMaxLaunchBlocks ? blocks - first : kMaxLaunchBlocks;
        launch(kernel, dim3((uint32_t)nb), dim3(256), 0, st, args..., (uint32_t)first);
    }
}

// Blocks of a grid-stride kernel over `items` of which a block takes `per_block` a round: enough for one round, at most 32 a CU.
static inline int tile_grid(unsigned long long items, unsigned long long per_block) {
    const unsigned long long want = (items + per_block - 1) / per_block;
    return (int)(want < 1ull ? 1ull : want > 256ull * 32ull ? 256ull * 32ull : want);
}
// The grid of a grid-stride kernel that takes one element a thread and round: at most the 2048 blocks of 256 threads the chip holds at
// once (8 a CU).
static inline dim3 entry_grid(unsigned long long elements) {
    const int blocks = tile_grid(elements, 256);
    return dim3((unsigned)(blocks < 2048 ? blocks : 2048));
}
// The same as a dim3 (merge.hip, connect.hip): at most tile_grid's 8192 blocks, far below the 2^24 blocks past which the runtime runs
// only a part of a grid (soft.h).
static inline dim3 tile_grid_dim(unsigned long long items, unsigned long long per_block) {
    const int g = tile_grid(items, per_block);
    assert(g >= 1 && (unsigned long long)g < (1ull << 24));
    return dim3((unsigned)g);
}

// Row-wise clear of `rows` rows of `width_bytes` at `pitch` (both multiples of 4, dst 4-byte aligned; the LSC accumulators): a kernel, on
// the stream and as a node of the graph alike.  It was hipMemset2DAsync / a memset node until a one-frame LSC group over device pointers,
// replayed by one slot, came back from its third replay with the result of accumulators that had not been cleared (measured on the
// MI355X, every time, 61 x 83 K = 20; groups of several frames and the direct path never did): tests/test_gpu_frames.py.
static __global__ void k_clear_rows(uint32_t* dst, size_t pitch_words, uint32_t width_words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < width_words) dst[(size_t)blockIdx.y * pitch_words + i] = 0u;
}
static inline hipError_t clear_rows(void* dst, size_t pitch, size_t width_bytes, size_t rows, hipStream_t st) {
    const uint32_t words = (uint32_t)(width_bytes / 4);
    launch(k_clear_rows, dim3((words + 255u) / 256u, (uint32_t)rows), dim3(256), 0, st, static_cast<uint32_t*>(dst), pitch / 4, words);
    return hipSuccess;
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the DEVICE that is current when it is set, and a process may hold an engine per
// GPU (the patched reference binding: arch "hip/gfx950:N"): set once per device and call site, result kept (`state`: 64 zero-initialised
// words of the call site; 1 set, -1 refused).  false: the kernel must not be launched with more than 64 KB of dynamic LDS on this device.
template <class F> static inline bool max_dynamic_lds_on_this_device(F* kernel, int bytes, std::atomic<int>* state) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev = dev < 0 || dev >= 64 ? 0 : dev;
    int s = state[dev].load(std::memory_order_acquire);
    if (s == 0) {
        s = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 1 : -1;
        state[dev].store(s, std::memory_order_release);
    }
    return s > 0;
}

// A stream operation the recorder has no node for: direct launches only for such a group.
static inline bool recording_unsupported() {
    GraphRecorder* r = current_recorder();
    if (!r) return false;
    if (r->err == hipSuccess) r->err = hipErrorNotSupported;
    return true;
}

}  // namespace fslic
