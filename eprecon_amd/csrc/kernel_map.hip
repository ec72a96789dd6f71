// Kernel maps of the sparse layers on gfx950: stride-1 and strided neighbour tables over a hash grid (hash_unique.hip builds it),
// the rank volume of a voxel set on a dense grid and the closed-form map of a dense 2D convolution.  (The transposed k2s2 map
// is in hash_unique.hip, which says why.)
//
// Replaces (reference call sites; implementations are in the un-vendored torchsparse / spconv):
//   spnn.Conv3d kernel maps (k3 s1, k2 s2), spconv SubMConv3d indice pairs
//                                       models/modules.py:19-64,90-122,181,252,444
// All kernels are atomic-free in their outputs (grid_rank counts off-grid voxels with an atomicAdd).
#include "hashgrid.hpp"

namespace {
using namespace ep;

// nbr[k][i] = row of the voxel at coords[i] + offset_k * stride (or -1).
// ksize 3: 27 offsets, x fastest (k = ((dz+1)*3 + (dy+1))*3 + (dx+1));
// ksize 2: 8 offsets in {0,1}^3, z fastest (k = 4*bx + 2*by + bz)   
__global__ void kernel_map_kernel(HashTable t, const int4 *coords, int n, int ksize, int stride,
                                  int32_t *nbr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    const int4 c = coords[i];
    int dx, dy, dz;
    if (ksize == 3) {
        dx = k % 3 - 1;
        dy = (k / 3) % 3 - 1;
        dz = k / 9 - 1;
    } else {
        dx = (k >> 2) & 1;
        dy = (k >> 1) & 1;
        dz = k & 1;
    }
    const int x = c.y + dx * stride, y = c.z + dy * stride, z = c.w + dz * stride;
    nbr[(size_t)k * n + i] = key_in_range(c.x, x, y, z) ? hash_lookup(t, pack_key(c.x, x, y, z)) : -1;
}

// The same 3x3x3 map for a voxel set queried against ITS OWN table (row i of `coords` is the table's value for its key: the sets
// the unique numbering produces): offset -o from voxel j leads to voxel i exactly when offset +o from i leads to j, so only the 13
// offsets below the centre (and the centre) are looked up and every hit also fills the mirrored entry nbr[26 - k][j] = i.  The
// upper half is pre-filled with -1 by the caller (hipMemsetAsync); a kernel map is injective per offset, so no two threads write
// the same mirrored entry.  Half the hash probes of kernel_map_kernel (the probes, random reads of a table of tens of MB, are
// what that kernel costs: 0.6 ms per cfg4 fragment), the same table bit for bit.
__global__ void kernel_map_self_kernel(HashTable t, const int4 *coords, int n, int stride, int32_t *nbr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;      // 0 .. 13
    if (i >= n) return;
    const int4 c = coords[i];
    const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
    const int x = c.y + dx * stride, y = c.z + dy * stride, z = c.w + dz * stride;
    const int j = key_in_range(c.x, x, y, z) ? hash_lookup(t, pack_key(c.x, x, y, z)) : -1;
    nbr[(size_t)k * n + i] = j;
    if (k < 13 && j >= 0) nbr[(size_t)(26 - k) * n + j] = i;
}

// rank volume of a voxel set on a dense grid: rank[(x/stride * gy + y/stride) * gz + z/stride] = row (cells start at -1)
__global__ void grid_rank_kernel(const int4 *coords, int n, int stride, int gx, int gy, int gz, int32_t *rank, int32_t *bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = coords[i];
    const int x = c.y / stride, y = c.z / stride, z = c.w / stride;
    const bool ok = c.y >= 0 && c.z >= 0 && c.w >= 0 && x < gx && y < gy && z < gz && x * stride == c.y && y * stride == c.z &&
                    z * stride == c.w;
    if (ok) rank[((size_t)x * gy + y) * gz + z] = i;
    else atomicAdd(bad, 1);
}

// Kernel map of a dense 2D 'same' convolution over `maps` images of h x w pixels stored row-major
// ([maps][h][w] rows of a channels-last tensor): nbr[(ky * ks + kx)][i] = row of pixel
// (y + ky - ks/2, x + kx - ks/2) of the same image, -1 outside it (zero padding).  Closed form, no
// hash grid: lets the 2D fusion convolutions of Occupancy_Initialization
// (models/occupancy_initialization.py:22-31, models/modules.py:313-399) run on the gather-GEMM kernel.
__global__ __launch_bounds__(256) void pixel_map_kernel(int maps, int h, int w, int ks, int32_t *nbr)
{
    const int n = maps * h * w;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = blockIdx.y;
    const int dy = k / ks - ks / 2, dx = k % ks - ks / 2;
    const int x = i % w, y = (i / w) % h;
    const int yy = y + dy, xx = x + dx;
    nbr[(size_t)k * n + i] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? i + dy * w + dx : -1;
}

}  // namespace

namespace ep {
// the region of a self map that must hold -1 before kernel_map_self runs: offsets 14 .. 26
FillRegion kernel_map_self_fill_region(int32_t *nbr, int64_t n)
{
    return FillRegion{nbr + (size_t)14 * n, (size_t)13 * n * sizeof(int32_t), 0xFFFFFFFFu};
}

int kernel_map_self(const void *table, uint32_t capacity, const int32_t *coords, int64_t n, int stride, int32_t *nbr, bool prefilled,
                    void *stream)
{
    if (!table || !table_capacity_ok(capacity) || n < 0 || stride < 1 || (n > 0 && (!coords || !nbr))) return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    HashTable t = make_table(table, capacity);
    if (!prefilled)
        EP_HIP_CHECK(hipMemsetAsync(nbr + (size_t)14 * n, 0xFF, (size_t)13 * n * sizeof(int32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(kernel_map_self_kernel, dim3((unsigned)ceil_div(n, 256), 14), dim3(256), 0, (hipStream_t)stream, t,
                       reinterpret_cast<const int4 *>(coords), (int)n, stride, nbr);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
}  // namespace ep

extern "C" {

int eprecon_kernel_map_async(const void *table, uint32_t capacity, const int32_t *coords, int64_t n,
                             int ksize, int stride, int32_t *nbr, void *stream)
{
    if (!table || !table_capacity_ok(capacity) || n < 0 || (ksize != 2 && ksize != 3) || stride < 1 ||
        (n > 0 && (!coords || !nbr)))
        return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    HashTable t = make_table(table, capacity);
    const int kvol = ksize * ksize * ksize;
    hipLaunchKernelGGL(kernel_map_kernel, dim3((unsigned)ceil_div(n, 256), kvol), dim3(256), 0,
                       (hipStream_t)stream, t, reinterpret_cast<const int4 *>(coords), (int)n, ksize,
                       stride, nbr);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_kernel_map_self_async(const void *table, uint32_t capacity, const int32_t *coords, int64_t n, int stride, int32_t *nbr,
                                  void *stream)
{
    return ep::kernel_map_self(table, capacity, coords, n, stride, nbr, false, stream);
}

int eprecon_grid_rank_async(const int32_t *coords, int64_t n, int stride, int grid_x, int grid_y, int grid_z, int32_t *rank,
                            void *stream)
{
    if (n < 0 || stride < 1 || grid_x <= 0 || grid_y <= 0 || grid_z <= 0 || !rank || (n > 0 && !coords) ||
        (int64_t)grid_x * grid_y * grid_z > 0x7ffffff0 || n > 0x7fffffff)
        return EPRECON_ERR_ARG;
    // rank[cells] then one int32: voxels off the grid (must stay 0; the caller may read it back)
    const size_t cells = (size_t)grid_x * grid_y * grid_z;
    EP_HIP_CHECK(hipMemsetAsync(rank, 0xff, cells * sizeof(int32_t), (hipStream_t)stream));
    EP_HIP_CHECK(hipMemsetAsync(rank + cells, 0, sizeof(int32_t), (hipStream_t)stream));
    if (n == 0) return EPRECON_OK;
    hipLaunchKernelGGL(grid_rank_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4 *>(coords), (int)n, stride, grid_x, grid_y, grid_z, rank, rank + cells);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_pixel_map_async(int maps, int height, int width, int ksize, int32_t *nbr, void *stream)
{
    if (maps <= 0 || height <= 0 || width <= 0 || ksize < 1 || ksize > 7 || !(ksize & 1) || !nbr ||
        (int64_t)maps * height * width > 0x7fffffff)
        return EPRECON_ERR_ARG;
    const int n = maps * height * width;
    hipLaunchKernelGGL(pixel_map_kernel, dim3((unsigned)ceil_div(n, 256), ksize * ksize), dim3(256), 0,
                       (hipStream_t)stream, maps, height, width, ksize, nbr);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
