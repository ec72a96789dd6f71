// Host walk of the search in eprecon_amd/csrc/label_transfer.hip (its helpers are plain host + device C++): on seeded volumes the
// thread form (one walker, shell after shell) and the wave form (64 walkers striding each shell, a minimum after every shell) are
// held against a brute force over all sites, and every shell enumeration against the definition of a shell.  No GPU, no HIP call.
//   hipcc --offload-arch=gfx950 -O1 -ffp-contract=off -I eprecon_amd/csrc -x hip tests/label_transfer_host_walk.cpp -o walk && ./walk
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "label_transfer.hip"

namespace {

struct Scene {
    LtGrid G;
    std::vector<unsigned long long> masks;
    std::vector<int> sites;      // linear indices, ascending
};

Scene make_scene(const int32_t dims[3], const float origin[3], double vs, double density, std::mt19937_64 &rng, int single = -1)
{
    Scene s;
    lt_grid(dims, origin, vs, s.G);
    s.masks.assign((size_t)s.G.nb[0] * s.G.nb[1] * s.G.nb[2], 0ull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int x = 0; x < dims[0]; ++x)
        for (int y = 0; y < dims[1]; ++y)
            for (int z = 0; z < dims[2]; ++z) {
                const int lin = (x * dims[1] + y) * dims[2] + z;
                if (single >= 0 ? lin != single : !(u(rng) < density)) continue;
                s.sites.push_back(lin);
                s.masks[((size_t)(x >> 2) * s.G.nb[1] + (y >> 2)) * s.G.nb[2] + (z >> 2)] |=
                    1ull << (((x & 3) << 4) | ((y & 3) << 2) | (z & 3));
            }
    return s;
}

void brute(const Scene &s, const float *p, double &best, int &bi)
{
    best = INFINITY, bi = 0x7fffffff;
    const LtGrid &G = s.G;
    for (int lin : s.sites) {
        const int z = lin % G.dims[2], y = lin / G.dims[2] % G.dims[1], x = lin / G.dims[2] / G.dims[1];
        const double d2 = lt_d2((double)p[0] - lt_site(G, x, 0), (double)p[1] - lt_site(G, y, 1), (double)p[2] - lt_site(G, z, 2));
        if (d2 < best || (d2 == best && lin < bi)) best = d2, bi = lin;
    }
}

int check_shell(const LtGrid &G, const LtQuery &Q, int r)
{
    const LtShell S = lt_shell_of(G, Q, r);
    std::vector<int> seen((size_t)G.nb[0] * G.nb[1] * G.nb[2], 0);
    for (int t = 0; t < S.total; ++t) {
        int bx, by, bz;
        lt_shell_brick(S, Q, r, t, bx, by, bz);
        if (bx < 0 || by < 0 || bz < 0 || bx >= G.nb[0] || by >= G.nb[1] || bz >= G.nb[2]) return 1;
        ++seen[((size_t)bx * G.nb[1] + by) * G.nb[2] + bz];
    }
    for (int bx = 0; bx < G.nb[0]; ++bx)
        for (int by = 0; by < G.nb[1]; ++by)
            for (int bz = 0; bz < G.nb[2]; ++bz) {
                const int d = std::max(std::max(std::abs(bx - Q.b[0]), std::abs(by - Q.b[1])), std::abs(bz - Q.b[2]));
                if (seen[((size_t)bx * G.nb[1] + by) * G.nb[2] + bz] != (d == r ? 1 : 0)) return 1;
            }
    return 0;
}

// -> shells walked, or -1 when the walk ran past rmax without being done
int walk_thread(const Scene &s, const LtQuery &Q, double &best, int &bi)
{
    best = INFINITY, bi = 0x7fffffff;
    for (int r = 0; r <= Q.rmax; ++r) {
        const LtShell S = lt_shell_of(s.G, Q, r);
        for (int t = 0; t < S.total; ++t) {
            int bx, by, bz;
            lt_shell_brick(S, Q, r, t, bx, by, bz);
            lt_visit(s.G, Q, s.masks.data(), bx, by, bz, best, bi);
        }
        if (lt_done(s.G, Q, r, best)) return r + 1;
    }
    return -1;
}

int walk_wave(const Scene &s, const LtQuery &Q, double &best, int &bi)
{
    best = INFINITY, bi = 0x7fffffff;
    for (int r = 0; r <= Q.rmax; ++r) {
        const LtShell S = lt_shell_of(s.G, Q, r);
        double lb[64];
        int li[64];
        for (int lane = 0; lane < 64; ++lane) {
            lb[lane] = best, li[lane] = bi;
            for (int t = lane; t < S.total; t += 64) {
                int bx, by, bz;
                lt_shell_brick(S, Q, r, t, bx, by, bz);
                lt_visit(s.G, Q, s.masks.data(), bx, by, bz, lb[lane], li[lane]);
            }
        }
        for (int lane = 0; lane < 64; ++lane)
            if (lb[lane] < best || (lb[lane] == best && li[lane] < bi)) best = lb[lane], bi = li[lane];
        if (lt_done(s.G, Q, r, best)) return r + 1;
    }
    return -1;
}

int run(const Scene &s, const std::vector<float> &verts, const char *what, long &shells)
{
    int bad = 0;
    for (size_t i = 0; i + 2 < verts.size(); i += 3) {
        const float *p = &verts[i];
        const LtQuery Q = lt_query_of(s.G, p);
        double b0, b1, b2;
        int i0, i1, i2;
        brute(s, p, b0, i0);
        const int r1 = walk_thread(s, Q, b1, i1), r2 = walk_wave(s, Q, b2, i2);
        shells += r1;
        int wrong = r1 < 0 || r2 < 0 || std::memcmp(&b0, &b1, 8) || std::memcmp(&b0, &b2, 8) || i0 != i1 || i0 != i2;
        if (i == 0)
            for (int r = 0; r <= Q.rmax; ++r) wrong |= check_shell(s.G, Q, r);
        if (wrong && bad++ < 5)
            std::printf("MISMATCH %s vertex %zu (%g %g %g): brute %d %.17g thread %d %.17g wave %d %.17g\n", what, i / 3, p[0], p[1],
                        p[2], i0, b0, i1, b1, i2, b2);
    }
    return bad;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20241019);
    int bad = 0, cases = 0;
    long shells = 0;
    const int32_t shapes[][3] = {{1, 1, 1}, {3, 2, 1}, {4, 4, 4}, {5, 4, 4}, {13, 10, 7}, {37, 21, 9}, {8, 8, 64}};
    const float origin[3] = {-1.23f, 0.57f, 2.01f};
    const double vs = 0.04;
    for (const auto &dims : shapes)
        for (double density : {-1.0, 0.0, 0.02, 0.3, 1.0}) {      // -1: one site, in the last (partial) brick
            const int n_cells = dims[0] * dims[1] * dims[2];
            const Scene s = make_scene(dims, origin, vs, density, rng, density < 0.0 ? n_cells - 1 : -1);
            std::vector<float> verts;
            std::uniform_real_distribution<double> u(-0.3, 1.3);
            for (int k = 0; k < 400; ++k)
                for (int a = 0; a < 3; ++a) verts.push_back((float)(origin[a] + u(rng) * (dims[a] - 1 + 1e-3) * vs));
            for (float far : {100.0f, -100.0f})
                for (int a = 0; a < 3; ++a) verts.push_back(a == 1 ? far : origin[a]);
            bad += run(s, verts, "random", shells);
            ++cases;
        }
    // exact ties: a dyadic lattice, vertices on sites, face midpoints, edge midpoints and cell corners.  Every cell a site: 2-, 4- and
    // 8-way ties around the vertex's own cell; sparse: equally near sites in different bricks, the one of the lower index visited later
    {
        const int32_t dims[3] = {9, 6, 5};
        const float o2[3] = {-1.25f, 0.5f, 2.0f};
        std::vector<float> verts;
        for (int x = -1; x <= 2 * dims[0]; ++x)
            for (int y = -1; y <= 2 * dims[1]; ++y)
                for (int z = -1; z <= 2 * dims[2]; ++z) {
                    verts.push_back(o2[0] + 0.03125f * x);
                    verts.push_back(o2[1] + 0.03125f * y);
                    verts.push_back(o2[2] + 0.03125f * z);
                }
        for (double density : {1.0, 0.12, 0.03}) {
            bad += run(make_scene(dims, o2, 0.0625, density, rng), verts, "ties", shells);
            ++cases;
        }
    }
    std::printf("%d cases, %ld shells walked, %d mismatches\n", cases, shells, bad);
    return bad ? 1 : 0;
}
