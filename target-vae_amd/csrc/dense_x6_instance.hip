// libtvae_hip.so: ONE instance of dense_x6_kernel<XV, NP, EPI> and its launcher, chosen on the command line
// (-DTVAE_DX6I_XV= -DTVAE_DX6I_EPI= -DTVAE_DX6I_NP=, set by the Makefile's pattern rule from the object's name).  The kernel is the
// slowest to compile in the library, so every instance of dense_x6_instances.def is an object of its own and they build in parallel.
#include "abi_dense_x6.hpp"

#define TVAE_DX6(XV_, E_, NP_) || (XV_ == TVAE_DX6I_XV && E_ == TVAE_DX6I_EPI && NP_ == TVAE_DX6I_NP)
static_assert(false
#include "dense_x6_instances.def"
              , "this instance is not listed in dense_x6_instances.def");
#undef TVAE_DX6

namespace tvae {
template <int XV, int EPI, int NP>
int dense_x6_launch(TVAE_DX6_LAUNCH_ARGS) {
    hipLaunchKernelGGL((dense_x6_kernel<XV, NP, EPI>), dim3(tm.grid()), dim3(DX6_THREADS), 0, st, a3, X, ldx, ep, M,
                       Mpad, N, K, K8pad, tm, bt, cd, it, vg, va, hs);
    return (int)hipGetLastError();
}
template int dense_x6_launch<TVAE_DX6I_XV, TVAE_DX6I_EPI, TVAE_DX6I_NP>(TVAE_DX6_LAUNCH_ARGS);
}  // namespace tvae
