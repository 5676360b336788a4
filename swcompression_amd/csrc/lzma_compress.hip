// lzma_compress.hip -- LZMA2 compression (lzma_comp.h): one unit per wavefront, the model, the hash table and the payload's stage in
// LDS (25,200 bytes: six waves per CU).
//
// A translation unit of its own, as inflate_team.hip is: the kernel shares lzma_wave.h's constants and job_kernels.h with the
// kernels of kernels.hip, and in one module with them a new caller changes what the inliner does with the others.  Here the code
// objects of all other kernels stay what they were (profiles/lzma2_compress_codegen.txt).
#include <hip/hip_runtime.h>
#include <cstddef>
#include "swc_common.h"
#include "job_kernels.h"
#include "launch.h"

namespace swc {

__global__ __launch_bounds__(64) void swc_lzma2_compress_kernel(Job* __restrict__ jobs, uint32_t n, const uint32_t* __restrict__ order) {
    __shared__ __attribute__((aligned(16))) lzmac::Lds lds;
    const uint32_t g = order ? order[blockIdx.x] : xcd_job(blockIdx.x, n);
    if (g >= n) return;
    jobk::lzma2_compress<kWave>(jobs, g, &lds, (int)threadIdx.x);
}

hipError_t launch_lzma2_compress(Job* jobs, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t* order = job_order(jobs, n, stream);
    hipLaunchKernelGGL(swc_lzma2_compress_kernel, dim3((unsigned)n), dim3(kWave), 0, stream, jobs, (uint32_t)n, order);
    return hipGetLastError();
}

}  // namespace swc
