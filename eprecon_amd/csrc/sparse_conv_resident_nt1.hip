// The group-resident gather kernel with 1 column tile of 32 per workgroup: see sparse_conv_resident_impl.hpp
#include "sparse_conv_resident_impl.hpp"

namespace epconv {
int launch_resident_nt1(const ConvParams &p, bool vec4, int cin_pad, hipStream_t st) { return launch_resident<1>(p, vec4, cin_pad, st); }
}  // namespace epconv
