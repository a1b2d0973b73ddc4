// Optional per-kernel timing for bench.py's roofline line: when enabled, the instrumented launches go through
// hipExtLaunchKernelGGL with a (start, stop) event pair that brackets exactly the kernel on its own stream, and the
// algorithmic work (flops or bytes) of each launch is recorded next to it.  Disabled (the default) it costs nothing.
#pragma once
#include <hip/hip_ext.h>

#include "common.h"

namespace cf {

enum ProfileKernel {
    PK_CONV_MT1 = 0, PK_CONV_MT2 = 1, PK_CONV_MT4 = 2,      // work = flops
    PK_CORRVOL_S1 = 3, PK_CORRVOL_S2 = 4, PK_CORRVOL_S4 = 5, // work = algorithmic bytes
    PK_CONV_F16S = 6,                                        // work = flops
    PK_ALLPAIRS = 7,                                         // RAFT all-pairs volume + pyramid pooling; work = algorithmic bytes
    PK_CORR_LOOKUP = 8,                                      // RAFT correlation lookup; work = algorithmic bytes
    PK_CONVEX_UP = 9,                                        // RAFT convex upsampling; work = algorithmic bytes
    PK_GN_APPLY = 10,                                        // GroupNorm apply passes; work = algorithmic bytes
    PK_WARP = 11, PK_WARP_LABELS = 12, PK_JACOBIAN = 13,     // VoxelMorph warp family (2-D); work = algorithmic bytes
    PK_CONV_SMALL_COUT = 14,                                 // direct 3x3 convolution to <= 4 output channels (flow heads); work = algorithmic bytes
    PK_CONV_STREAM = 15,                                     // conv_stream_kernel (same arithmetic as PK_CONV_F16S); work = flops
    PK_CONV_WINO = 16,                                       // conv_wino_kernel (row Winograd F(2,3), 3-term split); work = direct-form flops
    PK_COUNT = 17
};

bool profile_on();
// returns false when the event pool is exhausted (the launch then goes out un-timed)
bool profile_events(int kid, double work, hipEvent_t* start, hipEvent_t* stop);

template <typename K, typename... Args>
static inline void launch_profiled(int kid, double work, K kernel, dim3 grid, dim3 block, hipStream_t s, Args... args) {
    hipEvent_t e0, e1;
    if (profile_on() && profile_events(kid, work, &e0, &e1)) {
        hipExtLaunchKernelGGL(kernel, grid, block, 0, s, e0, e1, 0, args...);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    }
}

// The same for a kernel with dynamic LDS, with what every such launcher repeated around it: the kernel's opt-in to the 160 KiB of LDS, once
// per device (a second GPU driven by the same process needs it too), the timed (kid >= 0) or plain launch, and the launch error turned into
// "<family> launch failed: ...".  KERNEL is a template argument so that every instantiation has its own opt-in table.  Returns CF_OK / CF_ERR_LAUNCH.
constexpr size_t LDS_LIMIT = 160 * 1024;

template <auto KERNEL, typename... Args>
static inline int launch_lds(const char* family, int kid, double work, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, Args... args) {
    static bool opted_in[64] = {};
    const int dev = current_device_slot();
    if (!opted_in[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
        opted_in[dev] = true;
    }
    hipEvent_t e0, e1;
    if (kid >= 0 && profile_on() && profile_events(kid, work, &e0, &e1))
        hipExtLaunchKernelGGL(KERNEL, grid, block, lds_bytes, s, e0, e1, 0, args...);
    else
        hipLaunchKernelGGL(KERNEL, grid, block, lds_bytes, s, args...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string(family) + " launch failed: " + hipGetErrorString(e)); return CF_ERR_LAUNCH; }
    return CF_OK;
}

}  // namespace cf
