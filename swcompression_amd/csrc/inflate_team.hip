// inflate_team.hip -- Deflate phase 1 for launches of FEW streams: a workgroup of kTeamWaves wavefronts per stream (inflate_sync.h,
// "a team of wavefronts on one stream").  Block (64, kTeamWaves): threadIdx.x is the lane, threadIdx.y the wavefront -- the master on
// the job, the helpers on the rounds behind the master's.
//
// A translation unit of its own ON PURPOSE: in one module with swc_inflate_sync_kernel the second caller of the job's helper functions
// changes what the inliner does with them in the FIRST, and the throughput kernel -- 128 registers, none spilled -- came out with three
// spills (measured on the assembly; profiles/r06_experiments.txt).  Here nothing the other kernels are made of changes.
#include <hip/hip_runtime.h>
#include <cstddef>
#include "swc_common.h"
#include "job_kernels.h"
#include "launch.h"

namespace swc {

// `scratch`: (kTeamWaves - 1) * kTeamProvBytes per stream, the helpers' rows
__global__ __launch_bounds__(64 * inflate::kTeamWaves) void swc_inflate_team_kernel(Job* __restrict__ jobs, uint32_t n, WsMap wm, uint8_t* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) inflate::SyncLds team_lds[inflate::kTeamWaves];
    __shared__ __attribute__((aligned(16))) inflate::TeamShared team_shared;
    const uint32_t g = blockIdx.x;
    if (g >= n) return;
    jobk::inflate_team<kWave>(jobs, g, wm, scratch, team_lds, &team_shared, (int)threadIdx.x, (int)threadIdx.y);
}

size_t inflate_team_scratch_bytes(size_t n) { return n * jobk::kTeamScratchBytes; }

hipError_t launch_inflate_team(Job* jobs, size_t n, uint8_t* ws, size_t stride, const uint64_t* ws_off, uint8_t* scratch, hipStream_t stream) {
    const WsMap wm{ws, stride, ws_off};
    hipLaunchKernelGGL(swc_inflate_team_kernel, dim3((unsigned)n), dim3(kWave, inflate::kTeamWaves), 0, stream, jobs, (uint32_t)n, wm, scratch);
    return hipGetLastError();
}

}  // namespace swc
