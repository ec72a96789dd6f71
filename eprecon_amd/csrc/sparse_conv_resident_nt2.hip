// The group-resident gather kernel with 2 column tiles of 32 per workgroup: see sparse_conv_resident_impl.hpp
#include "sparse_conv_resident_impl.hpp"

namespace epconv {
int launch_resident_nt2(const ConvParams &p, bool vec4, int cin_pad, hipStream_t st) { return launch_resident<2>(p, vec4, cin_pad, st); }
}  // namespace epconv
