// dfl_trees.hip -- TEST HARNESS ONLY (tests/test_gpu_deflate_trees.py): the block pricing of the gzip / zlib kernel,
// dfl_block_lengths_small (lane-array trees) and dfl_block_lengths (the workgroup's LDS trees, under G_LOCK), run on
// given histograms.  Built at test time with hipcc; never part of the product library.
#include "snk_deflate.hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

// One histogram (DFL_HIST u32: literal/length counts at 0..285, distance counts at DFL_DOFF..DFL_DOFF+29) per wave,
// DFL_WAVES waves per workgroup, the LDS layout of the parse kernels.  mode 0: as dfl_flush_body (lane arrays when
// they can take the block, else the LDS builder under the lock); mode 1: the LDS builder for every histogram.
// out[3 * i ..]: opt_len, static_len, builder used (0 lane arrays, 1 LDS).
__global__ void __launch_bounds__(64 * DFL_WAVES) dfl_trees_kernel(const uint32_t *hists, uint32_t nh, uint32_t mode,
                                                                   int64_t *out)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    DflLds L;
    dfl_lds_pointers(L, wave);
    if (threadIdx.x == 0) *L.lock = 0u;
    __syncthreads();
    const uint32_t idx = blockIdx.x * DFL_WAVES + wave;
    if (idx >= nh) return;                                   // wave-uniform
    for (uint32_t i = lane; i < DFL_HIST; i += 64u) L.hist[i] = hists[(size_t)idx * DFL_HIST + i];
    __builtin_amdgcn_wave_barrier();
    long opt_len = 0, static_len = 0;
    const bool small = mode == 0u && dfl_block_lengths_small(L, lane, opt_len, static_len);
    if (lane == 0) {
        if (!small) {
            while (atomicCAS(L.lock, 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(8);
            dfl_block_lengths(L, opt_len, static_len);
            __threadfence_block();
            atomicExch(L.lock, 0u);
        }
        out[3 * (size_t)idx] = opt_len;
        out[3 * (size_t)idx + 1] = static_len;
        out[3 * (size_t)idx + 2] = small ? 0 : 1;
    }
}

// Host side: copies nh histograms in, runs the kernel, copies 3 * nh results out.  Returns 0 or the HIP error code.
extern "C" int dfl_trees_run(const uint32_t *hists, uint32_t nh, uint32_t mode, int64_t *out)
{
    uint32_t *dh = nullptr;
    int64_t *dout = nullptr;
    hipError_t e = hipMalloc((void **)&dh, (size_t)nh * DFL_HIST * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&dout, (size_t)nh * 3 * sizeof(int64_t));
    if (e == hipSuccess) e = hipMemcpy(dh, hists, (size_t)nh * DFL_HIST * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xff, (size_t)nh * 3 * sizeof(int64_t));
    if (e == hipSuccess) {
        const uint32_t groups = (nh + DFL_WAVES - 1u) / DFL_WAVES;
        hipLaunchKernelGGL(dfl_trees_kernel, dim3(groups), dim3(64 * DFL_WAVES), L_GROUP, 0, dh, nh, mode, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)nh * 3 * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (dh) (void)hipFree(dh);
    if (dout) (void)hipFree(dout);
    return (int)e;
}
