"""The distance-field rule (DESIGN.md §5b "distance field") in numpy, for tests/test_distance_field_host.py and
tests/test_distance_field_gpu.py; nothing of the package is imported.

    inside(r)  tsdf[r] <= 0; a coordinate that holds no row is outside; of rows that repeat a coordinate the first counts
    site       a (first) row with a 6-neighbour coordinate whose inside-state differs from its own
    dist2(x)   min over ALL sites s of the integer |x - s|^2, site(x) the smallest row index among the sites that attain it;
               beyond radius^2 (radius None: never): dist2 = FAR, site = -1
    state(x)   0 no row, 1 an outside row, 2 an inside row

The distances are a brute force over all sites per cell, in int64, in chunks of cells: no separable pass, no envelope, nothing
the kernel's decomposition could share a mistake with.
"""
import numpy as np

FAR = 0x7fffffff
STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def first_rows(coords):
    """{(x, y, z): the first row at that coordinate}"""
    rows = {}
    for r, c in enumerate(np.asarray(coords).reshape(-1, 3).tolist()):
        rows.setdefault(tuple(c), r)
    return rows


def site_rows(coords, tsdf):
    """the sorted row indices of the sites"""
    rows = first_rows(coords)
    tsdf = np.asarray(tsdf)

    def inside(c):
        r = rows.get(c)
        return r is not None and bool(tsdf[r] <= 0)

    sites = []
    for c, r in rows.items():
        mine = bool(tsdf[r] <= 0)
        if any(inside((c[0] + dx, c[1] + dy, c[2] + dz)) != mine for dx, dy, dz in STEPS):
            sites.append(r)
    return np.array(sorted(sites), np.int64)


def nearest_sites(cells, coords, sites, radius=None, chunk=4096):
    """cells int[N,3] -> (dist2 int64[N], site int64[N]) by brute force over `sites` (ascending rows)"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    dist2 = np.full(len(cells), FAR, np.int64)
    site = np.full(len(cells), -1, np.int64)
    if len(sites) == 0 or len(cells) == 0:
        return dist2, site
    at = np.asarray(coords, np.int64).reshape(-1, 3)[sites]                  # [S,3], rows ascending
    for s in range(0, len(cells), chunk):
        part = cells[s:s + chunk]
        d = sum((part[:, None, k] - at[None, :, k]) ** 2 for k in range(3))  # [n,S] int64
        best = d.argmin(1)                                                   # the first minimum: the smallest row
        dist2[s:s + chunk] = d[np.arange(len(best)), best]
        site[s:s + chunk] = sites[best]
    if radius is not None:
        far = dist2 > int(radius) ** 2
        dist2[far], site[far] = FAR, -1
    return dist2, site


def box_cells(lo, hi):
    """the cells of [lo, hi) in raster order (z fastest), int64[N,3]"""
    axes = [np.arange(l, h, dtype=np.int64) for l, h in zip(lo, hi)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)


def states(coords, tsdf, lo, hi):
    shape = tuple(int(h - l) for l, h in zip(lo, hi))
    out = np.zeros(shape, np.uint8)
    tsdf = np.asarray(tsdf)
    for c, r in first_rows(coords).items():
        k = tuple(int(v - l) for v, l in zip(c, lo))
        if all(0 <= v < n for v, n in zip(k, shape)):
            out[k] = 2 if tsdf[r] <= 0 else 1
    return out


def distance_field(coords, tsdf, lo, hi, radius=None):
    """-> (dist2 int32, site int32, state uint8) [X,Y,Z] over the cells [lo, hi)"""
    shape = tuple(int(h - l) for l, h in zip(lo, hi))
    dist2, site = nearest_sites(box_cells(lo, hi), coords, site_rows(coords, tsdf), radius)
    return dist2.astype(np.int32).reshape(shape), site.astype(np.int32).reshape(shape), states(coords, tsdf, lo, hi)


def crossed_edge_midpoints(coords, tsdf):
    """float64[E,3]: the midpoints of the lattice edges (unit steps along +x, +y, +z from a row or to a row) whose two ends
    differ in inside-state"""
    rows = first_rows(coords)
    tsdf = np.asarray(tsdf)

    def inside(c):
        r = rows.get(c)
        return r is not None and bool(tsdf[r] <= 0)

    mids = set()
    for c in rows:
        for dx, dy, dz in STEPS:
            n = (c[0] + dx, c[1] + dy, c[2] + dz)
            if inside(c) != inside(n):
                mids.add(tuple((a + b) / 2.0 for a, b in zip(c, n)))
    return np.array(sorted(mids), np.float64).reshape(-1, 3)
