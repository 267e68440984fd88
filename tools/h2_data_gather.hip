// frm_gather_kernel (h2o_amd/csrc/hhuff_gather.h) behind one C symbol, for tools/h2_data_rate.py: the de-framers'
// copy given one job per DATA frame's payload, as a yardstick for the framer's copy on the same bytes.  The tool
// builds it into build/libh2_data_gather.so; it is no part of the library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff_gather.h"

extern "C" __attribute__((visibility("default"))) int h2_data_gather(const uint8_t* in, uint8_t* out, const void* jobs, uint32_t njobs,
                                                                     void* stream) {
    using namespace hhuff;
    if (njobs == 0) return 0;
    hipLaunchKernelGGL(frm_gather_kernel, dim3((uint32_t)(((uint64_t)njobs + kGatherThreads - 1u) / kGatherThreads)), dim3(kGatherThreads),
                       0, (hipStream_t)stream, in, out, (const uint4*)jobs, njobs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
