// Ray casting of a sparse TSDF scene on gfx950, straight from its voxel rows: no dense volume, no mesh.
//
// The reference shows a scene by meshing it (tools/render.py, VIS_INCREMENTAL: marching cubes, then pyrender); the rule here is
// this project's (DESIGN.md §5b "ray-cast surface") and is what eprecon_amd/raycast.py previews, labels and shades with.
//
//   field   F = the trilinear interpolation of the samples at the integer lattice points (world = origin + c * voxel_size);
//           a sample that is no row reads 1.  A cell (the unit cube above sample c) is ACTIVE when one of its 8 corners is a row
//           with tsdf <= 0: F > 0 on every other cell.
//   build   clear, then ONE launch over the rows: row key -> row (hashgrid.hpp, first occurrence), and every row with
//           tsdf <= 0 ORs the bits of the 8 cells it corners into the 64-bit words of the 4x4x4-cell bricks they lie in
//           (brick = cell >> 2, arithmetic; bit = x + 4 y + 16 z of cell & 3), and widens the box of the active cells.
//   cast    one lane per pixel, one 8x8 pixel tile per wave.  The ray p(t) = P0 + t D in lattice units (t: camera-z metres) is
//           cut at the integer planes, t_plane(n) = (n - P0) * (1 / D) per axis: every boundary parameter is that expression
//           or t_0 / t_end, whichever way the walk got there, so skipping changes no value.  Bricks first (an absent brick or
//           a zero word costs one look-up and one slab exit), then the cells of a present brick, of which only those whose bit
//           is set are evaluated: 8 row look-ups, F at both ends of the segment, regula falsi, gradient, nearest row corner.
//
// The camera block is render.py's (K, K^-1, world -> camera per view, fp64) followed by origin[3] and 1 / voxel_size; P0 and D
// are formed in fp64 from it and carried in fp32 from there, as tests/raycast_ref.py's float32 twin does.  -ffp-contract=off
// holds for this unit as for the library: the expressions below are evaluated as written.
//
// Bounds: brick steps <= the sum of the box's brick extents + 3, cell steps <= 10 per brick visit (a line crosses at most 9
// inner planes of a 4x4x4 brick); an overrun stores into the status word (plain stores of one value per cause: the cast has no
// atomics) and the Python side raises.  Results are a function of the pixel alone: bit-identical from run to run and however
// the views are split into calls.
#include "hashgrid.hpp"

namespace {
using namespace ep;

constexpr int kBlock = 256;
constexpr int kTile = 8;                      // 8 x 8 pixels per wave
constexpr int kMaxRefine = 16;
constexpr int kCellsPerBrickVisit = 10;
constexpr int kStatusKeyRange = 1;            // build: a row (or a neighbour a cast would look up) outside the key range
constexpr int kStatusTableFull = 2;           // build: a probe sequence wrapped
constexpr int kStatusCellOverrun = 1;         // cast: more than kCellsPerBrickVisit cells inside one brick
constexpr int kStatusBrickOverrun = 2;        // cast: more brick steps than the box allows

// header words (int32) at the start of the grid memory
constexpr int kHeadStatus = 0, kHeadLo = 1, kHeadHi = 4, kHeadWords = 8;
constexpr size_t kHeadBytes = 256;

struct Bricks {
    unsigned long long *keys;   // [capacity]
    unsigned long long *words;  // [capacity]
    uint32_t mask;
};

struct Layout {
    uint32_t row_capacity, brick_capacity;
    size_t row_table, brick_keys, brick_words, total;
};

Layout layout_for(int64_t m)
{
    m = m > 0 ? m : 0;
    Layout L;
    L.row_capacity = hash_capacity_for(m);
    L.brick_capacity = hash_capacity_for(4 * m);      // a row corners cells of at most 8 bricks: load <= 1/2 at 4 per row, < 1 always
    L.row_table = kHeadBytes;
    L.brick_keys = L.row_table + align_up(table_bytes(L.row_capacity), 256);
    L.brick_words = L.brick_keys + (size_t)L.brick_capacity * 8;
    L.total = L.brick_words + (size_t)L.brick_capacity * 8;
    return L;
}

__global__ __launch_bounds__(kBlock) void raycast_clear_kernel(HashTable rows, Bricks bricks, int32_t *head)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i <= rows.mask) {
        rows.keys[i] = kEmptyKey;
        rows.vals[i] = 0x7fffffff;
    }
    if (i <= bricks.mask) {
        bricks.keys[i] = kEmptyKey;
        bricks.words[i] = 0ull;
    }
    if (i < kHeadWords) head[i] = i == kHeadStatus ? 0 : i >= kHeadLo && i < kHeadLo + 3 ? 0x7fffffff : i >= kHeadHi && i < kHeadHi + 3 ? (int32_t)0x80000000 : 0;
}

// the 4-bit set of the positions (c - 1) & 3 and c & 3 that lie in brick b of one axis
__device__ __forceinline__ unsigned axis_bits(int c, int b)
{
    return ((((c - 1) >> 2) == b) ? 1u << ((c - 1) & 3) : 0u) | (((c >> 2) == b) ? 1u << (c & 3) : 0u);
}

__device__ __forceinline__ bool brick_or(const Bricks &t, unsigned long long key, unsigned long long bits)
{
    uint32_t s = hash_slot(key, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long prev = atomicCAS(&t.keys[s], kEmptyKey, key);
        if (prev == kEmptyKey || prev == key) {
            atomicOr(&t.words[s], bits);
            return true;
        }
        s = (s + 1) & t.mask;
    }
    return false;
}

__global__ __launch_bounds__(kBlock) void raycast_build_kernel(HashTable rows, Bricks bricks, const int32_t *__restrict__ coords,
                                                               const float *__restrict__ tsdf, int32_t m, int32_t *head)
{
    __shared__ int32_t box[6];
    if (threadIdx.x < 3) box[threadIdx.x] = 0x7fffffff;
    else if (threadIdx.x < 6) box[threadIdx.x] = (int32_t)0x80000000;
    __syncthreads();
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < m) {
        const int x = coords[3 * (size_t)i], y = coords[3 * (size_t)i + 1], z = coords[3 * (size_t)i + 2];
        // the cast looks up the corners of the cells c - 1 .. c: c - 1 .. c + 1 must be keys
        if (!key_in_range(0, x, y, z) || !key_in_range(0, x - 1, y - 1, z - 1) || !key_in_range(0, x + 1, y + 1, z + 1)) {
            atomicOr(head + kHeadStatus, kStatusKeyRange);
        } else {
            if (!hash_insert(rows, pack_key(0, x, y, z), i)) atomicOr(head + kHeadStatus, kStatusTableFull);
            if (tsdf[i] <= 0.0f) {
                for (int sx = 0; sx < 2; ++sx) {
                    const int bx = sx ? x >> 2 : (x - 1) >> 2;
                    if (sx && bx == ((x - 1) >> 2)) continue;
                    for (int sy = 0; sy < 2; ++sy) {
                        const int by = sy ? y >> 2 : (y - 1) >> 2;
                        if (sy && by == ((y - 1) >> 2)) continue;
                        for (int sz = 0; sz < 2; ++sz) {
                            const int bz = sz ? z >> 2 : (z - 1) >> 2;
                            if (sz && bz == ((z - 1) >> 2)) continue;
                            const unsigned long long mx = axis_bits(x, bx);
                            const unsigned my = axis_bits(y, by), mz = axis_bits(z, bz);
                            unsigned long long bits = 0ull;
                            for (int cz = 0; cz < 4; ++cz)
                                for (int cy = 0; cy < 4; ++cy)
                                    if (((mz >> cz) & 1u) && ((my >> cy) & 1u)) bits |= mx << (4 * cy + 16 * cz);
                            if (!brick_or(bricks, pack_key(0, bx, by, bz), bits)) atomicOr(head + kHeadStatus, kStatusTableFull);
                        }
                    }
                }
                atomicMin(&box[0], x - 1);
                atomicMin(&box[1], y - 1);
                atomicMin(&box[2], z - 1);
                atomicMax(&box[3], x);
                atomicMax(&box[4], y);
                atomicMax(&box[5], z);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        if (box[threadIdx.x] != 0x7fffffff) atomicMin(head + kHeadLo + threadIdx.x, box[threadIdx.x]);
    } else if (threadIdx.x < 6) {
        if (box[threadIdx.x] != (int32_t)0x80000000) atomicMax(head + kHeadHi + threadIdx.x - 3, box[threadIdx.x]);
    }
}

struct CastParams {
    HashTable rows;
    Bricks bricks;
    const int32_t *head;
    const float *tsdf;
    const double *cams;
    int n_views, height, width;
    float pixel_center, znear, zfar;
    int refine;
    float *depth, *normal;
    int32_t *row, *status;
};

struct Axis {
    float p0, d, inv;       // inv = 1 / d, never used when d == 0
};

__device__ __forceinline__ float plane_t(int n, const Axis &a) { return ((float)n - a.p0) * a.inv; }

// the cell of one axis at parameter t: a plane whose parameter is <= t has been crossed
__device__ __forceinline__ int cell_at(float t, const Axis &a)
{
    int c = (int)floorf(a.p0 + t * a.d);
    if (a.d > 0.0f) {
        if (plane_t(c + 1, a) <= t) ++c;
        else if (plane_t(c, a) > t) --c;
    } else if (a.d < 0.0f) {
        if (plane_t(c, a) <= t) --c;
        else if (plane_t(c + 1, a) > t) ++c;
    }
    return c;
}

// the parameter at which the ray leaves [lo, hi + 1) of one axis (cells lo .. hi), +inf for a ray parallel to it
__device__ __forceinline__ float next_plane(int lo, int hi, const Axis &a)
{
    return a.d > 0.0f ? plane_t(hi + 1, a) : a.d < 0.0f ? plane_t(lo, a) : __builtin_inff();
}

__device__ __forceinline__ unsigned long long brick_word(const Bricks &t, int bx, int by, int bz)
{
    const unsigned long long key = pack_key(0, bx, by, bz);
    uint32_t s = hash_slot(key, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long k = t.keys[s];
        if (k == key) return t.words[s];
        if (k == kEmptyKey) return 0ull;
        s = (s + 1) & t.mask;
    }
    return 0ull;
}

struct Corners {
    float v[8];     // k = 4 dx + 2 dy + dz
    int32_t r[8];
};

__device__ __forceinline__ float trilinear(const Corners &c, float fx, float fy, float fz)
{
    const float ux = 1.0f - fx, uy = 1.0f - fy, uz = 1.0f - fz;
    const float x00 = c.v[0] * ux + c.v[4] * fx, x01 = c.v[1] * ux + c.v[5] * fx;
    const float x10 = c.v[2] * ux + c.v[6] * fx, x11 = c.v[3] * ux + c.v[7] * fx;
    const float y0 = x00 * uy + x10 * fy, y1 = x01 * uy + x11 * fy;
    return y0 * uz + y1 * fz;
}

__global__ __launch_bounds__(kBlock) void raycast_kernel(CastParams P)
{
    const int tiles_x = (P.width + kTile - 1) / kTile, tiles_y = (P.height + kTile - 1) / kTile;
    const long long wave = (long long)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const long long per_view = (long long)tiles_x * tiles_y;
    const int view = (int)(wave / per_view);
    if (view >= P.n_views) return;
    const int tile = (int)(wave - (long long)view * per_view), lane = threadIdx.x & (kWave - 1);
    const int u = (tile % tiles_x) * kTile + (lane & (kTile - 1)), v = (tile / tiles_x) * kTile + lane / kTile;
    if (u >= P.width || v >= P.height) return;
    const size_t pix = ((size_t)view * P.height + v) * P.width + u;

    float depth = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    int32_t row = -1;
    int over = 0;

    const int lox = P.head[kHeadLo], loy = P.head[kHeadLo + 1], loz = P.head[kHeadLo + 2];
    const int hix = P.head[kHeadHi], hiy = P.head[kHeadHi + 1], hiz = P.head[kHeadHi + 2];
    Axis X, Y, Z;
    {
        const double *kinv = P.cams + 9, *w = P.cams + 18 + 12 * (size_t)view, *ext = P.cams + 18 + 12 * (size_t)P.n_views;
        const double px = (double)u + (double)P.pixel_center, py = (double)v + (double)P.pixel_center;
        const double cx = kinv[0] * px + kinv[1] * py + kinv[2], cy = kinv[3] * px + kinv[4] * py + kinv[5];
        const double s = ext[3];
        // w = [R | t] world -> camera: the direction is R^T (cx, cy, 1), the centre -R^T t
        X.d = (float)((w[0] * cx + w[4] * cy + w[8]) * s);
        Y.d = (float)((w[1] * cx + w[5] * cy + w[9]) * s);
        Z.d = (float)((w[2] * cx + w[6] * cy + w[10]) * s);
        X.p0 = (float)((-(w[0] * w[3] + w[4] * w[7] + w[8] * w[11]) - ext[0]) * s);
        Y.p0 = (float)((-(w[1] * w[3] + w[5] * w[7] + w[9] * w[11]) - ext[1]) * s);
        Z.p0 = (float)((-(w[2] * w[3] + w[6] * w[7] + w[10] * w[11]) - ext[2]) * s);
        // (a component below 1e-20 cells per metre moves the ray by nothing a float holds: it walks as an exact zero)
        if (fabsf(X.d) < 1e-20f) X.d = 0.0f;
        if (fabsf(Y.d) < 1e-20f) Y.d = 0.0f;
        if (fabsf(Z.d) < 1e-20f) Z.d = 0.0f;
        X.inv = 1.0f / X.d;
        Y.inv = 1.0f / Y.d;
        Z.inv = 1.0f / Z.d;
    }

    // the slab of the active box [lo, hi + 1] per axis
    float t0 = P.znear, t_end = P.zfar;
    bool alive = lox <= hix;
    {
        const Axis *ax[3] = {&X, &Y, &Z};
        const int lo[3] = {lox, loy, loz}, hi[3] = {hix, hiy, hiz};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const Axis &a = *ax[k];
            if (a.d != 0.0f) {
                const float ta = plane_t(lo[k], a), tb = plane_t(hi[k] + 1, a);
                t0 = fmaxf(t0, fminf(ta, tb));
                t_end = fminf(t_end, fmaxf(ta, tb));
            } else if (!(a.p0 >= (float)lo[k] && a.p0 <= (float)(hi[k] + 1))) {
                alive = false;
            }
        }
    }
    alive = alive && t0 < t_end;

    if (alive) {
        const int max_bricks = ((hix >> 2) - (lox >> 2) + 1) + ((hiy >> 2) - (loy >> 2) + 1) + ((hiz >> 2) - (loz >> 2) + 1) + 3;
        float t = t0;
        bool first = true, done = false;
        int cx = cell_at(t, X), cy = cell_at(t, Y), cz = cell_at(t, Z);
        for (int bs = 0; !done; ++bs) {
            if (bs >= max_bricks) {
                over = kStatusBrickOverrun;
                break;
            }
            const int bx = cx >> 2, by = cy >> 2, bz = cz >> 2;
            const unsigned long long word = brick_word(P.bricks, bx, by, bz);
            if (word == 0ull) {
                const float te = fminf(fminf(next_plane(4 * bx, 4 * bx + 3, X), next_plane(4 * by, 4 * by + 3, Y)),
                                       next_plane(4 * bz, 4 * bz + 3, Z));
                if (!(te < t_end)) break;
                t = te;
                first = false;
                cx = cell_at(t, X);
                cy = cell_at(t, Y);
                cz = cell_at(t, Z);
                continue;
            }
            bool left = false;
            for (int cs = 0; cs < kCellsPerBrickVisit && !done && !left; ++cs) {
                const float tx = next_plane(cx, cx, X), ty = next_plane(cy, cy, Y), tz = next_plane(cz, cz, Z);
                const float tn = fminf(fminf(tx, ty), tz);
                const float tb = fminf(tn, t_end);
                if ((word >> ((cx & 3) + 4 * (cy & 3) + 16 * (cz & 3))) & 1ull) {
                    Corners c;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        c.r[k] = hash_lookup(P.rows, pack_key(0, cx + (k >> 2), cy + ((k >> 1) & 1), cz + (k & 1)));
                        c.v[k] = c.r[k] < 0 ? 1.0f : P.tsdf[c.r[k]];
                    }
                    const float ox = X.p0 - (float)cx, oy = Y.p0 - (float)cy, oz = Z.p0 - (float)cz;   // (exact or one rounding; the twin's too)
                    float a = t, ga = trilinear(c, ox + a * X.d, oy + a * Y.d, oz + a * Z.d);
                    bool hit = false;
                    float x = 0.0f;
                    if (ga <= 0.0f) {
                        if (first) done = true;     // the walk starts inside: empty
                        else {
                            hit = true;             // (only rounding between two cells' views of one face gets here)
                            x = a;
                        }
                    } else {
                        float b = tb, gb = trilinear(c, ox + b * X.d, oy + b * Y.d, oz + b * Z.d);
                        if (gb <= 0.0f) {
                            hit = true;
                            x = a + (b - a) * (ga / (ga - gb));
                            for (int it = 0; it < P.refine; ++it) {
                                const float f = trilinear(c, ox + x * X.d, oy + x * Y.d, oz + x * Z.d);
                                if (f <= 0.0f) {
                                    b = x;
                                    gb = f;
                                } else {
                                    a = x;
                                    ga = f;
                                }
                                x = a + (b - a) * (ga / (ga - gb));
                            }
                        }
                    }
                    if (hit) {
                        done = true;
                        depth = x;
                        const float fx = ox + x * X.d, fy = oy + x * Y.d, fz = oz + x * Z.d;
                        const float ux = 1.0f - fx, uy = 1.0f - fy, uz = 1.0f - fz;
                        const float gx = ((c.v[4] - c.v[0]) * uy + (c.v[6] - c.v[2]) * fy) * uz + ((c.v[5] - c.v[1]) * uy + (c.v[7] - c.v[3]) * fy) * fz;
                        const float gy = ((c.v[2] - c.v[0]) * ux + (c.v[6] - c.v[4]) * fx) * uz + ((c.v[3] - c.v[1]) * ux + (c.v[7] - c.v[5]) * fx) * fz;
                        const float gz = ((c.v[1] - c.v[0]) * ux + (c.v[5] - c.v[4]) * fx) * uy + ((c.v[3] - c.v[2]) * ux + (c.v[7] - c.v[6]) * fx) * fy;
                        const float len = sqrtf(gx * gx + gy * gy + gz * gz);
                        if (len > 0.0f) {
                            nx = gx / len;
                            ny = gy / len;
                            nz = gz / len;
                        }
                        float best = __builtin_inff();
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const float ex = fx - (float)(k >> 2), ey = fy - (float)((k >> 1) & 1), ez = fz - (float)(k & 1);
                            const float d2 = ex * ex + ey * ey + ez * ez;
                            if (c.r[k] >= 0 && d2 < best) {
                                best = d2;
                                row = c.r[k];
                            }
                        }
                    }
                }
                first = false;
                if (done) break;
                if (!(tn < t_end)) {
                    done = true;
                    break;
                }
                t = tn;
                if (tx <= ty && tx <= tz) cx += X.d > 0.0f ? 1 : -1;
                else if (ty <= tz) cy += Y.d > 0.0f ? 1 : -1;
                else cz += Z.d > 0.0f ? 1 : -1;
                left = (cx >> 2) != bx || (cy >> 2) != by || (cz >> 2) != bz;
            }
            if (!done && !left) {
                over = kStatusCellOverrun;
                break;
            }
        }
    }
    if (over) {
        *P.status = over;
        depth = nx = ny = nz = 0.0f;
        row = -1;
    }
    P.depth[pix] = depth;
    P.normal[3 * pix] = nx;
    P.normal[3 * pix + 1] = ny;
    P.normal[3 * pix + 2] = nz;
    P.row[pix] = row;
}

bool tables_of(const void *grid, int64_t m, HashTable &rows, Bricks &bricks)
{
    if (!grid) return false;
    const Layout L = layout_for(m);
    char *g = reinterpret_cast<char *>(const_cast<void *>(grid));
    rows = make_table(g + L.row_table, L.row_capacity);
    bricks = Bricks{reinterpret_cast<unsigned long long *>(g + L.brick_keys), reinterpret_cast<unsigned long long *>(g + L.brick_words),
                    L.brick_capacity - 1};
    return true;
}

}  // namespace

extern "C" {

size_t eprecon_raycast_workspace_bytes(int64_t m) { return layout_for(m).total; }

int eprecon_raycast_build_async(const int32_t *coords, const float *tsdf, int64_t m, void *grid, size_t grid_bytes, void *stream)
{
    if (m < 0 || m > 0x07ffffffll || !grid || (m > 0 && (!coords || !tsdf))) return EPRECON_ERR_ARG;
    if (grid_bytes < layout_for(m).total) return EPRECON_ERR_WORKSPACE;
    HashTable rows;
    Bricks bricks;
    tables_of(grid, m, rows, bricks);
    int32_t *head = reinterpret_cast<int32_t *>(grid);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t span = (rows.mask > bricks.mask ? rows.mask : bricks.mask) + 1;
    hipLaunchKernelGGL(raycast_clear_kernel, dim3((span + kBlock - 1) / kBlock), dim3(kBlock), 0, st, rows, bricks, head);
    EP_LAUNCH_CHECK();
    if (m == 0) return EPRECON_OK;
    hipLaunchKernelGGL(raycast_build_kernel, dim3((unsigned)ceil_div(m, kBlock)), dim3(kBlock), 0, st, rows, bricks, coords, tsdf,
                       (int32_t)m, head);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_raycast_async(const void *grid, int64_t m, const float *tsdf, const double *cams, int n_views, int height, int width,
                          float pixel_center, float znear, float zfar, int refine, float *depth, float *normal, int32_t *row,
                          int32_t *status, void *stream)
{
    if (!grid || m < 1 || m > 0x07ffffffll || !tsdf || !cams || n_views < 1 || height < 1 || width < 1 || !(znear > 0.0f) ||
        !(zfar > znear) || !(zfar < __builtin_inff()) || refine < 0 || refine > kMaxRefine || !depth || !normal || !row || !status)
        return EPRECON_ERR_ARG;
    const int64_t waves = (int64_t)n_views * ceil_div(width, kTile) * ceil_div(height, kTile);
    const int64_t blocks = ceil_div(waves, kBlock / kWave);
    if (blocks > 0x7fffffffll || (int64_t)n_views * height * width > 0x7fffffffll) return EPRECON_ERR_UNSUPPORTED;
    CastParams P;
    tables_of(grid, m, P.rows, P.bricks);
    P.head = reinterpret_cast<const int32_t *>(grid);
    P.tsdf = tsdf;
    P.cams = cams;
    P.n_views = n_views;
    P.height = height;
    P.width = width;
    P.pixel_center = pixel_center;
    P.znear = znear;
    P.zfar = zfar;
    P.refine = refine;
    P.depth = depth;
    P.normal = normal;
    P.row = row;
    P.status = status;
    hipStream_t st = (hipStream_t)stream;
    EP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(raycast_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, P);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
