// The direct gather kernels with 4 column tiles of 16 (C_out <= 64): sparse_conv_direct_kernels.hpp behind the launcher
#include "sparse_conv_direct_launch.hpp"

namespace epconv {
int launch_direct16_ct4(const ConvParams &p, hipStream_t st) { return launch_ct<4>(p, st); }
}  // namespace epconv
