// replica.hip -- the swap kernel of a replica-exchange round (replica_kernels.hpp) in a translation unit of its own: the code
// objects of the step kernels and of the sampler's host file stay what they are without it.
#include <hip/hip_runtime.h>

#define MCMCPP_DEFINE_REPLICA_KERNEL
#include "replica_kernels.hpp"

namespace mcmcpp
{
void launch_replica_swap(const ReplicaSwapArgs<double>& a, const ReplicaShape& s, hipStream_t stream)
{
    hipLaunchKernelGGL(replica_swap_kernel<double>, dim3(s.grid_x, s.grid_y), dim3(kReplicaBlockThreads), 0, stream, a);
}
void launch_replica_swap(const ReplicaSwapArgs<float>& a, const ReplicaShape& s, hipStream_t stream)
{
    hipLaunchKernelGGL(replica_swap_kernel<float>, dim3(s.grid_x, s.grid_y), dim3(kReplicaBlockThreads), 0, stream, a);
}
}  // namespace mcmcpp
