// bsw_stage.hip -- the launchers of bsw_stage_k.h: each read's run of seed slots (bsw_chain.hip's rounds and
// region selection start from it) and the scans that turn counts into offsets.  Plain C++, vector stores only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "bsw_stage_k.h"

namespace bsw {

__global__ void seed_runs_kernel(const int32_t *__restrict__ sr, int32_t ns, int32_t n_reads,
                                 int32_t *__restrict__ sbeg, int32_t *__restrict__ send, int32_t *__restrict__ err)
{
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    const int32_t r = sr[k];
    if (r < 0 || r >= n_reads || (k > 0 && sr[k - 1] > r)) {
        atomicOr(err, 1);
        return;
    }
    if (k == 0 || sr[k - 1] != r) sbeg[r] = k;
    if (k == ns - 1 || sr[k + 1] != r) send[r] = k + 1;
}

hipError_t launch_seed_runs(const int32_t *seed_read, int32_t n_seeds, int32_t n_reads, int32_t *sbeg, int32_t *send,
                            int32_t *err_word, hipStream_t s)
{
    if (n_seeds <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_runs_kernel, grid_for(n_seeds, 256), dim3(256), 0, s, seed_read, n_seeds, n_reads, sbeg,
                       send, err_word);
    return hipGetLastError();
}

hipError_t launch_scan32(void *tmp, size_t *tmp_bytes, const int32_t *in, int32_t *out, int32_t n, hipStream_t s)
{
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, in, out, n + 1, s);
}

hipError_t launch_scan64(void *tmp, size_t *tmp_bytes, const int64_t *in, int64_t *out, int32_t n, hipStream_t s)
{
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, in, out, n + 1, s);
}

}  // namespace bsw
