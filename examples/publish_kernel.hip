// A node's own kernel writes its output into the sample in place and publishes it itself:
// one launch, no pack, no second stream operation.  Compiles with
//   hipcc --offload-arch=gfx950 -c -I include examples/publish_kernel.hip
//
//   dora_node_allocate_data_sample(node, n * sizeof(float), &sample);
//   dora_sample_fill_ticket(node, sample, workgroups, DORA_FILL_WRITE_THROUGH, &ticket);
//   launch_scale(in, (float*)dora_sample_data(sample), n, 0.5f, ticket, my_stream);
//   dora_node_send_output_sample(node, "out", type_info, type_info_len, NULL, 0, sample);
#include <hip/hip_runtime.h>

#include "dora_gpu_device.h"

// out[i] = in[i] * k, four floats per lane, stored write-through (n a multiple of 4, `out`
// 16-byte aligned: a sample's data is).
__global__ void scale_into_sample(const float* __restrict__ in, float* out, uint64_t n, float k,
                                  dora_fill_ticket ticket) {
  const uint64_t t_start = dora_fill_clock();
  for (uint64_t i = 4 * (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x); i + 4 <= n;
       i += 4 * uint64_t(gridDim.x) * blockDim.x) {
    const float4 v = *reinterpret_cast<const float4*>(in + i);
    const dora_u32x4 w = {__float_as_uint(v.x * k), __float_as_uint(v.y * k),
                          __float_as_uint(v.z * k), __float_as_uint(v.w * k)};
    dora_st16(out + i, w);
  }
  // every thread of every workgroup, after its last store, in uniform control flow
  dora_fill_publish(ticket, blockIdx.x, gridDim.x, t_start);
}

// The grid is the ticket's workgroup count: a launch of another size publishes nothing.
void launch_scale(const float* in, float* out, uint64_t n, float k, const dora_fill_ticket& ticket,
                  hipStream_t stream) {
  hipLaunchKernelGGL(scale_into_sample, dim3(ticket.workgroups), dim3(256), 0, stream, in, out, n,
                     k, ticket);
}
