"""Inputs of the stage-0 selection (init_select) shared by tests/test_grid_patterns.py (host: what oracle/grid_ops.py makes of
them) and tests/test_grid_edges_gpu.py (the kernels against the oracle).  Plain numpy.

A pattern is a boolean volume over the D^3 coarse cells.  Its voxel list holds, for every coarse cell, the children at the offsets
{0, cell - 1}^3 (one child for cell = 1); only the LAST child (cell - 1, cell - 1, cell - 1) of a marked cell is above the threshold,
so a cell is found only by OR-pooling over its children.  High logits alternate between 2 and +Inf, low ones between -4, -Inf and
NaN.  Rows with the batch index -1 and `batch`, all of them above the threshold on every coarse cell, are mixed in: they must be
ignored.  The rows of a call are shuffled, so no element's rows are contiguous or in raster order."""
import numpy as np

DIMS = (1, 2, 3, 5, 24, 31, 32)
CELLS = (1, 2, 4)
THRESHOLD = 0.3
PATTERNS = ("empty", "full", "corners", "slab", "plane", "random93", "random50")


def pattern(name, D):
    v = np.zeros((D, D, D), bool)
    if name == "full":
        v[:] = True
    elif name == "corners":                     # a 3^3 block in each of the eight corners
        for x in (slice(0, 3), slice(max(D - 3, 0), D)):
            for y in (slice(0, 3), slice(max(D - 3, 0), D)):
                for z in (slice(0, 3), slice(max(D - 3, 0), D)):
                    v[x, y, z] = True
    elif name == "slab":                        # the three highest z layers: bit D - 1 of a column word (bit 31 at D = 32)
        v[:, :, max(D - 3, 0):] = True
    elif name == "plane":                       # the single plane z = D - 1
        v[:, :, D - 1] = True
    elif name == "random93":
        v = np.random.default_rng(0).random((D, D, D)) < 0.93
    elif name == "random50":
        v = np.random.default_rng(0).random((D, D, D)) < 0.5
    else:
        assert name == "empty"
    return v


def expected_rows(name, D):
    """the row counts the selection (erode, dilate, dilate on zero-padded 3^3 boxes) must give, worked out by hand:
    full      the erosion leaves the (D - 2)^3 core, two dilations restore the volume; nothing survives below D = 3
    corners   each block erodes to its centre, which grows to 5^3 clipped at the corner = 4^3: 8 * 64; at D = 3 and 5 the grown
              blocks cover the volume
    slab      the layer z = D - 2 survives inside the border, grows to all of x and y and to the four layers D - 4 .. D - 1
    plane     one layer never survives an erosion
    None: not worked out by hand (random fills)"""
    if name in ("empty", "plane"):
        return 0
    if D < 3:
        return 0
    if name == "full":
        return D ** 3
    if name == "corners":
        return 512 if D >= 8 else D ** 3 if D in (3, 5) else None
    if name == "slab":
        return 4 * D * D if D >= 5 else 27 if D == 3 else None
    if name == "random93":
        return 31937 if D == 32 else None       # (numpy default_rng(0).random((D, D, D)) < 0.93: by the oracle)
    if name == "random50":
        return 0 if D >= 5 else None
    return None


def voxel_list(names, D, cell, seed=0, strays=True):
    """one pattern per batch element -> logit f32[N], coords int32[N, 4], shuffled"""
    batch = len(names)
    offs = sorted({0, cell - 1})
    child = np.array([(a, b, c) for a in offs for b in offs for c in offs])
    last = np.all(child == cell - 1, axis=1)
    cells = np.argwhere(np.ones((D, D, D), bool))
    hi = np.array([2.0, np.inf], np.float32)
    lo = np.array([-4.0, -np.inf, np.nan], np.float32)
    logits, coords = [], []
    for b, name in enumerate(names):
        on = pattern(name, D).reshape(-1)
        xyz = (cells[:, None, :] * cell + child[None]).reshape(-1, 3)
        above = (on[:, None] & last[None, :]).reshape(-1)
        k = np.arange(xyz.shape[0])
        logits.append(np.where(above, hi[k % 2], lo[k % 3]).astype(np.float32))
        coords.append(np.concatenate([np.full((xyz.shape[0], 1), b), xyz], axis=1))
    if strays:
        for b in (-1, batch):
            xyz = cells * cell + (cell - 1)
            logits.append(np.full(xyz.shape[0], 5.0, np.float32))
            coords.append(np.concatenate([np.full((xyz.shape[0], 1), b), xyz], axis=1))
    logit, coords = np.concatenate(logits), np.concatenate(coords).astype(np.int32)
    perm = np.random.default_rng(seed + 7 * D + cell).permutation(logit.shape[0])
    return logit[perm], np.ascontiguousarray(coords[perm])


def calls(D):
    """the pattern tuples one (D, cell) runs: every pattern alone, and every three cyclic neighbours as a batch of three"""
    single = [(p,) for p in PATTERNS]
    triple = [tuple(PATTERNS[(i + k) % len(PATTERNS)] for k in range(3)) for i in range(len(PATTERNS))]
    return single + triple


def raster_rows(vol, b, cell):
    """a selected coarse volume -> its output rows"""
    xyz = np.argwhere(vol) * cell
    return np.concatenate([np.full((xyz.shape[0], 1), b), xyz], axis=1).astype(np.int32)
